"""Per-step observations from the device replay, the parts that need no GPU: the loop reference of the all-steps block
(tests/replay_obs_reference.py) on a hand-written case, `fit_vector(all_obs=)` -- what it asks of the buffer and what it
refuses before anything runs -- on stub buffers, and the ABI: `obs_steps` took the place of `reserved0` in
`mzs_replay_sample_args` without moving anything."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import muax_amd as mx
import replay_obs_reference as obsref
import replay_reference as ref
from muax_amd import _lib


# ---- the reference ----
def test_reference_on_a_hand_written_case():
    ep0 = {"obs": np.array([[1, 2], [3, 4], [5, 6], [7, 8], [9, 10]], np.float32)}
    ep1 = {"obs": np.array([[-1, -2], [-3, -4], [-5, -6]], np.float32)}
    assert obsref.window_obs(ep0, 1, 3).tolist() == [[3, 4], [5, 6], [7, 8]]
    assert obsref.window_obs(ep0, 2, 3).tolist() == [[5, 6], [7, 8], [9, 10]]  # up to the episode's last row
    got = obsref.batch_obs([ep0, ep1], [0, 1, 1, 0], [0, 1, -1, 3], 2)
    assert got.dtype == np.float32 and got.shape == (4, 2, 2)
    assert got.tolist() == [[[1, 2], [3, 4]], [[-3, -4], [-5, -6]], [[0, 0], [0, 0]], [[7, 8], [9, 10]]]


def test_reference_first_row_is_the_window_of_the_sampling_reference():
    rng = np.random.default_rng(3)
    eps = [ref.make_episode(rng, T, 2, 3) for T in (4, 9, 6)]
    e, start = ref.sample_indices([5, 6], eps, 11, 3, 2)
    got = obsref.batch_obs(eps, e, start, 3)
    want = ref.batch_fields(eps, e, start, 3)["obs"]  # [B, 1, obs_dim]
    assert np.array_equal(got[:, :1], want)
    for j in range(11):
        assert np.array_equal(got[j], eps[e[j]]["obs"][start[j]:start[j] + 3])


# ---- fit_vector ----
class _VecEnv:
    """Four environments with fixed episode lengths; observation = (env id, step)."""
    lengths = (5, 7, 6, 9)
    spec = SimpleNamespace(max_episode_steps=10)

    def reset(self):
        self.t = [0] * 4
        return np.array([[e, 0] for e in range(4)], np.float32)

    def step(self, actions):
        d = np.zeros(4, bool)
        for e in range(4):
            self.t[e] += 1
            if self.t[e] == self.lengths[e]:
                d[e], self.t[e] = True, 0
        return np.array([[e, self.t[e]] for e in range(4)], np.float32), 1.0 + np.asarray(actions, np.float64), d


class _Model:
    device, _support_size = torch.device("cpu"), 10

    def __init__(self, stochastic):
        self.trains_stochastic, self.batches = stochastic, []

    def init(self, key, sample):
        pass

    def act(self, key, obs, with_pi=False, with_value=False, **kw):
        obs = np.asarray(obs, np.float32)
        a = (obs.sum(1) % 2).astype(np.int64)
        pi = np.stack([a == 0, a == 1], 1).astype(np.float32)
        return (a, pi, obs.sum(1).astype(np.float64)) if with_pi else a

    def update(self, batch):
        self.batches.append(batch)
        return {"loss": float(np.sum(batch.Rn))}


class _AllObsBuffer(mx.TrajectoryReplayBuffer):
    """The host buffer with the device buffer's `all_obs` parameter (and its write-back), recording what it is asked."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.asked = []

    def sample(self, *a, with_indices=False, all_obs=False, **kw):
        self.asked.append(all_obs)
        batch = super().sample(*a, **kw)
        B = np.asarray(batch.Rn).shape[0]
        return (batch, (np.arange(B), np.zeros(B, np.int32))) if with_indices else batch

    def update_priorities(self, indices, priorities, alpha=1.0, eps=0.0, weight="mean"):
        raise AssertionError("not reached")


def _fit(model, buffer, **kw):
    mx.fit_vector(model, _VecEnv(), _VecEnv(), n_step=2, gamma=0.9, buffer=buffer, iterations=2, steps_per_iteration=10,
                  num_simulations=2, k_steps=3, num_trajectory=4, num_update_per_iteration=3, test_interval=10,
                  random_seed=1, **kw)


@pytest.mark.parametrize("stochastic,all_obs,want", [(True, None, True), (False, None, False), (False, True, True),
                                                     (True, False, False)])
def test_fit_vector_asks_for_every_observation_when_the_model_trains_stochastic(stochastic, all_obs, want):
    model, buf = _Model(stochastic), _AllObsBuffer(50, random_seed=4)
    _fit(model, buf, all_obs=all_obs)
    assert len(buf.asked) == len(model.batches) == 6 and buf.asked == [want] * 6


def test_fit_vector_leaves_a_buffer_without_all_obs_alone():
    """The host buffer returns every row already: a stochastic model trains on it as before, `all_obs` never passed."""
    import inspect
    assert "all_obs" not in inspect.signature(mx.TrajectoryReplayBuffer.sample).parameters
    rows = {}
    for stochastic in (False, True):
        model = _Model(stochastic)
        _fit(model, mx.TrajectoryReplayBuffer(50, random_seed=4))
        rows[stochastic] = model.batches
    assert len(rows[True]) == 6
    for x, y in zip(rows[False], rows[True]):
        assert np.array_equal(x.obs, y.obs) and np.array_equal(x.Rn, y.Rn)


def test_fit_vector_refuses_all_obs_on_a_buffer_without_it():
    with pytest.raises(ValueError, match=r"all_obs needs a buffer whose sample\(\) takes all_obs.*TrajectoryReplayBuffer"):
        mx.fit_vector(None, None, None, buffer=mx.TrajectoryReplayBuffer(10), all_obs=True)
    with pytest.raises(ValueError, match="all_obs"):
        mx.fit_vector(None, None, None, all_obs=True)  # the default buffer is the host one


def test_fit_vector_refuses_priority_steps_for_a_stochastic_model():
    """unroll_values is not built for an SMZNetwork: named before the first step, not a NotImplementedError after the
    first update.  Without the write-back priority_steps is ignored, as for any model."""
    buf = _AllObsBuffer(50, random_seed=4)
    with pytest.raises(ValueError, match="priority_steps.*SMZNetwork"):
        mx.fit_vector(_Model(True), None, None, buffer=buf, priority_update=True, priority_steps=2)
    assert buf.asked == []
    model = _Model(True)
    _fit(model, buf, priority_steps=2)
    assert len(model.batches) == 6


def test_muzero_names_the_predicate_update_uses():
    g = torch.Generator().manual_seed(0)
    smz = mx.MuZero(mx.create_stochastic_muzero_network(4, 3, 2, 17, generator=g), support_size=8, device="cpu")
    mz = mx.MuZero(mx.nn.MZNetwork(mx.nn.Representation(8, generator=g), mx.nn.Prediction(2, 21, generator=g),
                                   mx.nn.Dynamic(8, 2, 21, generator=g)), device="cpu")
    assert smz.trains_stochastic is True and mz.trains_stochastic is False


def test_sample_takes_all_obs_and_checks_before_any_device_use():
    import inspect
    p = inspect.signature(mx.DeviceReplayBuffer.sample).parameters
    assert p["all_obs"].default is False
    b = mx.DeviceReplayBuffer(4, 100, random_seed=0)
    with pytest.raises(ValueError, match="empty buffer"):
        b.sample(4, k_steps=3, all_obs=True)


# ---- the ABI ----
def test_obs_steps_sits_where_reserved0_was():
    """(That these are the header's members and the compiler's offsets: tests/test_abi_cpu.py, for every struct.)"""
    S = _lib.MzsReplaySampleArgs
    assert "obs_steps" in dict(S._fields_) and "reserved0" not in dict(S._fields_)
    # 112 bytes as before the field had a name; the int32 behind key[2] at byte 28, the first pointer behind it
    assert (ctypes.sizeof(S), S.obs_steps.offset, S.key.offset, S.obs.offset) == (112, 28, 20, 32)
    assert S.obs_steps.size == 4 and _lib.args(S).obs_steps == 0  # zero-filled: today's behaviour
