"""`DeviceVectorCollector` end to end (muax_amd/vector.py, DeviceReplayBuffer.add_steps) on a scripted vector environment
whose `done` schedule and rewards are a fixed table (tests/collect_reference.py), so that no episode depends on the
actions: the device route must leave in its buffer, byte for byte, what `VectorCollector` with the same keys followed
by `add_raw` leaves in a second one.  CartPole's shapes, three environments, a ring of 70 rows that the third call
wraps."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import collect_reference as cref
import muax_amd as mx
from helpers import train_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("obs", "a", "r", "Rn", "v", "done", "pi", "w")
N, OBS_DIM, A, RING, N_STEP, GAMMA, SIMS, K = 3, 4, 2, 70, 5, 0.997, 4, 3
CALLS = (30, 30, 25)  # rows 60..84 of the third call wrap past ring row 69
ENDS = {0: (0, 1, 9, 30, 31, 50, 64, 80, 84, 100), 1: tuple(range(18, 120, 19)), 2: (32, 65, 66, 99)}


def _tables():
    done = np.zeros((120, N), bool)
    for env, ends in ENDS.items():
        done[list(ends), env] = True
    return done, np.random.default_rng(5).uniform(-1, 2, (120, N))


def _env():
    return cref.ScriptedVecEnv(*_tables(), obs_dim=OBS_DIM)


@functools.lru_cache(maxsize=None)
def _model():
    return train_model(A, 8, OBS_DIM, seed=3, support=10)


def _flat(trajs):
    """Host trajectories as add_raw's flat stream."""
    bt = [t.batched_transitions for t in trajs]
    lengths = [len(t) for t in trajs]
    cat = {k: np.concatenate([np.asarray(getattr(b, k))[0].reshape(T, -1) for b, T in zip(bt, lengths)])
           for k in ("obs", "a", "r", "v", "pi")}
    return cat["obs"], cat["a"][:, 0], cat["r"][:, 0], cat["v"][:, 0], cat["pi"], lengths


@functools.lru_cache(maxsize=None)
def _routes(alpha, weight, min_length=1, capacity=64, max_steps=512, calls=CALLS):
    """Route A: DeviceVectorCollector into buffer A.  Route B: VectorCollector with the same keys, its trajectories
    (those of at least min_length steps) flattened into add_raw on buffer B.  C: the same trajectories by add_many."""
    model = _model()
    bufs = [mx.DeviceReplayBuffer(capacity, max_steps, random_seed=0) for _ in range(3)]
    dev = mx.DeviceVectorCollector(_env(), bufs[0], N_STEP, GAMMA, alpha, weight=weight, min_length=min_length,
                                   ring_steps=RING)
    host = mx.VectorCollector(_env(), N_STEP, GAMMA, alpha)
    key_a = key_b = mx.prng.PRNGKey(7)
    finished, trajs = [], []
    for steps in calls:
        fin, key_a, count = dev.collect(model, key_a, steps, num_simulations=SIMS)
        assert count == steps * N
        got, key_b, _ = host.collect(model, key_b, steps, num_simulations=SIMS)
        assert np.array_equal(key_a, key_b)
        keep = [t for t in got if len(t) >= min_length]
        if keep:
            bufs[1].add_raw(*_flat(keep), N_STEP, GAMMA, alpha, weight=weight)
            bufs[2].add_many(keep, [t.weights.mean() if weight == "mean" else t.weights.sum() for t in keep])
        finished.append(fin)
        trajs.append(got)
    torch.cuda.synchronize()
    return bufs, finished, trajs, dev


def _assert_same_episodes(x, y, exact_w=True):
    assert x.serials == y.serials and len(x) > 0 and x.steps == y.steps
    worst = 0.0
    for s in x.serials:
        ex, ey = x.episode(s), y.episode(s)
        for k in FIELDS:
            gx, gy = getattr(ex, k), getattr(ey, k)
            assert gx.dtype == gy.dtype and gx.shape == gy.shape, (s, k)
            if k == "w" and not exact_w:
                err = ((gx - gy).abs() / gy.abs()).max().item()
                worst = max(worst, err)
                assert err <= 1e-12, (s, err)
            else:
                assert torch.equal(gx, gy), (s, k)
    return worst


@pytest.mark.parametrize("alpha,weight", [(0.5, "mean"), (None, "sum"), (1.0, "sum")])
def test_three_calls_equal_the_host_collector_and_add_raw(alpha, weight):
    (a, b, _), finished, trajs, _ = _routes(alpha, weight)
    _assert_same_episodes(a, b)
    assert len(a) == sum(len(t) for t in trajs) == 16 and a._dirty and a._touched == b._touched
    assert (a._head, a._tail, a._steps, a._serial, a._clock) == (b._head, b._tail, b._steps, b._serial, b._clock)
    # what collect() returns: lengths, returns from the host's rewards, serials in the host collector's order
    serial = 0
    for fin, got in zip(finished, trajs):
        assert len(fin) == len(got)
        for (T, G, s), tr in zip(fin, got):
            assert T == len(tr) and G == float(np.sum(tr.rewards)) and s == serial
            serial += 1
    for key in (1, 2):  # the same tables, so the same draws
        ba, ia = a.sample(num_trajectory=50, sample_per_trajectory=2, k_steps=K, key=key, with_indices=True)
        bb, ib = b.sample(num_trajectory=50, sample_per_trajectory=2, k_steps=K, key=key, with_indices=True)
        assert torch.equal(ia[0], ib[0]) and torch.equal(ia[1], ib[1])
        for k in FIELDS:
            assert torch.equal(getattr(ba, k), getattr(bb, k)), k


def test_three_calls_against_add_many_of_the_host_trajectories():
    """The host's NumPy arithmetic: the fp32 fields bit for bit, w (a pow on each side) within 1e-12 relative."""
    (a, _, c), _, _, _ = _routes(0.5, "mean")
    worst = _assert_same_episodes(a, c, exact_w=False)
    print(f"[w against NumPy: worst relative error {worst:.1e}]", end=" ")


def test_min_length_drops_the_references_episodes():
    (a, b, _), finished, trajs, _ = _routes(0.5, "mean", min_length=K)
    _assert_same_episodes(a, b)
    done, _ = _tables()
    open_start, step0, serial, dropped = [0] * N, 0, 0, 0
    for steps, fin in zip(CALLS, finished):
        want_fin, want_drop, open_start = cref.ring_plan(done[step0:step0 + steps].tolist(), open_start, step0, K)
        every = sorted(want_fin + want_drop)
        assert [T for T, _, _ in fin] == [T for _, _, T in every]
        for (T, _, s), ep in zip(fin, every):
            if ep in want_drop:
                assert T < K and s is None
                dropped += 1
            else:
                assert s == serial
                serial += 1
        step0 += steps
    assert dropped == 4 and a.serials == list(range(serial))


def test_a_collection_larger_than_the_buffer_leaves_add_raws_survivors():
    (a, b, _), finished, _, _ = _routes(None, "mean", capacity=3, max_steps=64)
    _assert_same_episodes(a, b)
    assert len(a) <= 3 and a.serials[-1] == 15
    assert [s for fin in finished for _, _, s in fin] == list(range(16))  # evicted again or not, every one had a serial


def test_ring_overflow_is_refused_before_the_first_step_and_a_smaller_call_goes_on():
    (a, b, _), _, _, dev = _routes.__wrapped__(0.5, "sum", calls=(30, 30))  # (not cached: the buffers move on)
    env, calls = dev.venv, dev.venv.step_calls
    before = {k: x.clone() for k, x in dev._fields.items()}
    key = mx.prng.PRNGKey(9)
    with pytest.raises(ValueError, match="ring"):
        dev.collect(_model(), key, 44, num_simulations=SIMS)  # environment 2's episode is open since step 33: 27 + 44 > 70
    assert env.step_calls == calls == 60
    assert all(torch.equal(x, before[k]) for k, x in dev._fields.items())
    # 27 + 43 = 70 fits exactly; the host route from the same state
    host = mx.VectorCollector(_env(), N_STEP, GAMMA, 0.5)
    hkey = mx.prng.PRNGKey(7)
    for steps in (30, 30):
        _, hkey, _ = host.collect(_model(), hkey, steps, num_simulations=SIMS)
    fin, key_a, _ = dev.collect(_model(), key, 43, num_simulations=SIMS)
    got, key_b, _ = host.collect(_model(), key, 43, num_simulations=SIMS)
    assert np.array_equal(key_a, key_b) and len(fin) == len(got) > 0 and env.step_calls == 103
    b.add_raw(*_flat(got), N_STEP, GAMMA, 0.5, weight="sum")
    _assert_same_episodes(a, b)


def test_an_episode_longer_than_max_steps_is_add_raws_value_error():
    buf = mx.DeviceReplayBuffer(8, 16)
    dev = mx.DeviceVectorCollector(_env(), buf, N_STEP, GAMMA, None, ring_steps=RING)
    with pytest.raises(ValueError, match="max_steps"):
        dev.collect(_model(), mx.prng.PRNGKey(0), 30, num_simulations=SIMS)  # environment 0 finishes 21 steps (10..30)
    assert len(buf) == 0


def test_bad_buffers_and_steps():
    with pytest.raises(ValueError, match="device store"):
        mx.DeviceVectorCollector(_env(), mx.TrajectoryReplayBuffer(10), N_STEP, GAMMA)
    dev = mx.DeviceVectorCollector(_env(), mx.DeviceReplayBuffer(8, 64), N_STEP, GAMMA)
    with pytest.raises(ValueError, match="steps"):
        dev.collect(_model(), mx.prng.PRNGKey(0), 0)
    assert dev.venv.step_calls == 0


def _fit_vector_once(device_collect):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from cartpole_env import VectorCartPole
    g = torch.Generator().manual_seed(0)
    net = mx.nn.MZNetwork(mx.nn.Representation(8, generator=g), mx.nn.Prediction(2, 21, generator=g),
                          mx.nn.Dynamic(8, 2, 21, generator=g))
    model = mx.MuZero(net, optimizer=mx.optimizers.create_optimizer("adam", 5e-3))
    buf, rows = mx.DeviceReplayBuffer(64, 4096, random_seed=13), []
    mx.fit_vector(model, VectorCartPole(8, seed=0), VectorCartPole(2, max_episode_steps=20, seed=1), n_step=3, alpha=None,
                  buffer=buf, iterations=2, steps_per_iteration=16, num_simulations=4, k_steps=3, num_trajectory=8,
                  sample_per_trajectory=2, num_update_per_iteration=3, test_interval=10, random_seed=3, metrics=rows,
                  device_collect=device_collect)
    return buf, rows


def test_fit_vector_device_collect_equals_the_host_route():
    """alpha None: the weights are exactly 1 on both routes, so the draws and therefore the losses coincide."""
    buf_d, rows_d = _fit_vector_once(True)
    buf_h, rows_h = _fit_vector_once(False)
    assert len(rows_d) == len(rows_h) == 2 and buf_d.serials == buf_h.serials and len(buf_d) > 0
    for d, h in zip(rows_d, rows_h):
        assert d.get("loss") == h.get("loss")
        assert d["episodes"] == h["episodes"] and d["env_steps"] == h["env_steps"]
        assert d["G"] == h["G"] or (np.isnan(d["G"]) and np.isnan(h["G"]))
    assert np.isfinite(rows_d[-1]["loss"])
    _assert_same_episodes(buf_d, buf_h)
