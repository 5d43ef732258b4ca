"""Collection on the device, the host half (muax_amd/vector.py: `ring_plan`, `DeviceVectorCollector`'s and
`fit_vector(device_collect=)`'s refusals) against the plain loops of tests/collect_reference.py.  No GPU."""
import numpy as np
import pytest

import collect_reference as cref
import muax_amd as mx


def _same(done, open_start, step0, min_length):
    got = mx.ring_plan(np.asarray(done, bool), np.asarray(open_start), step0, min_length)
    want = cref.ring_plan(np.asarray(done, bool).tolist(), list(open_start), step0, min_length)
    assert [tuple(int(x) for x in e) for e in got[0]] == want[0]
    assert [tuple(int(x) for x in e) for e in got[1]] == want[1]
    assert [int(x) for x in got[2]] == want[2]
    return want


def test_no_episode_ends():
    fin, drop, new_open = _same(np.zeros((7, 3), bool), [2, 0, 5], 9, 1)
    assert fin == [] and drop == [] and new_open == [2, 0, 5]


def test_every_step_ends_an_episode():
    fin, drop, new_open = _same(np.ones((4, 2), bool), [10, 10], 10, 1)
    assert fin == [(0, 10, 1), (0, 11, 1), (0, 12, 1), (0, 13, 1), (1, 10, 1), (1, 11, 1), (1, 12, 1), (1, 13, 1)]
    assert drop == [] and new_open == [14, 14]
    # an open episode that its first step closes keeps the steps it carried
    fin, _, _ = _same(np.ones((2, 2), bool), [7, 10], 10, 1)
    assert fin[0] == (0, 7, 4) and fin[2] == (1, 10, 1)


def test_an_episode_spanning_three_calls():
    open_start, step0 = [0, 0], 0
    calls = [np.zeros((5, 2), bool), np.zeros((4, 2), bool), np.zeros((6, 2), bool)]
    calls[0][2, 1] = True   # environment 1 ends one at step 2, then stays open
    calls[2][3, 0] = True   # environment 0: steps 0..12, over all three calls
    calls[2][5, 1] = True   # environment 1: steps 3..14
    every = []
    for D in calls:
        fin, drop, open_start = _same(D, open_start, step0, 1)
        every += fin
        step0 += len(D)
    assert every == [(1, 0, 3), (0, 0, 13), (1, 3, 12)] and open_start == [13, 15]


def test_min_length_drops_the_first_the_last_and_all_episodes_of_an_environment():
    D = np.zeros((12, 3), bool)
    D[[1, 6, 11], 0] = True       # lengths 2, 5, 5: the first is dropped
    D[[4, 9, 11], 1] = True       # lengths 5, 5, 2: the last is dropped
    D[[0, 2, 4, 5], 2] = True     # lengths 1, 2, 2, 1: all are dropped
    fin, drop, new_open = _same(D, [0, 0, 0], 0, 3)
    assert fin == [(0, 2, 5), (0, 7, 5), (1, 0, 5), (1, 5, 5)]
    assert drop == [(0, 0, 2), (1, 10, 2), (2, 0, 1), (2, 1, 2), (2, 3, 2), (2, 5, 1)]
    assert new_open == [12, 12, 6]
    # a carried start makes a short tail long enough
    fin, drop, _ = _same(D[:2], [-4, 0, 0], 0, 3)
    assert fin == [(0, -4, 6)] and drop == [(2, 0, 1)]


def test_one_environment():
    D = np.zeros((9, 1), bool)
    D[[0, 3, 8], 0] = True
    fin, drop, new_open = _same(D, [0], 0, 2)
    assert fin == [(0, 1, 3), (0, 4, 5)] and drop == [(0, 0, 1)] and new_open == [9]


@pytest.mark.parametrize("seed", range(6))
def test_random_streams_call_after_call(seed):
    rng = np.random.default_rng(seed)
    N = int(rng.integers(1, 6))
    open_start, step0 = [0] * N, 0
    for _ in range(5):
        T = int(rng.integers(1, 20))
        D = rng.uniform(size=(T, N)) < rng.choice([0.0, 0.1, 0.5, 1.0])
        _, _, open_start = _same(D, open_start, step0, int(rng.integers(1, 5)))
        step0 += T


def test_bad_shapes_are_value_errors():
    with pytest.raises(ValueError):
        mx.ring_plan(np.zeros(4, bool), [0], 0, 1)
    with pytest.raises(ValueError):
        mx.ring_plan(np.zeros((4, 2), bool), [0], 0, 1)


def test_the_order_is_the_host_collectors():
    """The host collector on a scripted environment with a stub model: its trajectories, identified by the
    (environment, step) their first observation carries, come out in ring_plan's order, call after call."""
    rng = np.random.default_rng(11)
    S, N = 60, 4
    done = rng.uniform(size=(S, N)) < 0.15
    done[:, 3] = False
    done[[0, 1, 2], 2] = True  # length-1 episodes
    env = cref.ScriptedVecEnv(done, rng.uniform(-1, 2, (S, N)))
    col = mx.VectorCollector(env, 3, 0.9, 0.5)
    key = mx.prng.PRNGKey(0)
    open_start, step0, total = np.zeros(N, np.int64), 0, 0
    for steps in (7, 1, 19, 13, 20):
        trajs, key, count = col.collect(cref.StubModel(), key, steps, num_simulations=2)
        assert count == steps * N
        got = []
        for tr in trajs:
            first = np.asarray(tr.batched_transitions.obs).reshape(len(tr), -1)[0]
            got.append((int(first[0]), int(first[1]), len(tr)))
        fin, drop, open_start = mx.ring_plan(done[step0:step0 + steps], open_start, step0, 1)
        assert [tuple(int(x) for x in e) for e in fin] == got and drop == []
        step0 += steps
        total += len(got)
    assert total > 10 and env.step_calls == 60


class _NoStore:
    def sample(self, *a, **k):
        raise AssertionError("never sampled")


def test_device_collect_needs_the_device_store():
    with pytest.raises(ValueError, match="device_collect"):
        mx.fit_vector(None, None, None, buffer=mx.TrajectoryReplayBuffer(10), device_collect=True)
    with pytest.raises(ValueError, match="device_collect"):
        mx.fit_vector(None, None, None, device_collect=True)  # the default buffer is the host one
    with pytest.raises(ValueError, match="device store"):
        mx.DeviceVectorCollector(None, _NoStore(), 3, 0.9)
    assert hasattr(mx.DeviceReplayBuffer, "add_steps")
