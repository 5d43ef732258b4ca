"""CPU tests of the priority write-back's host parts: the plain-loop reference the GPU tests compare the kernels with
(tests/priority_reference.py) on hand-computed cases, the ABI declarations, the checks `update_priorities` makes before
it touches the device, `value_priorities`, and `fit_vector(priority_update=)` on a buffer without the method.  No GPU,
no kernel."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import muax_amd as mx
import priority_reference as pref
from helpers import train_model
from muax_amd import _lib, vector

NAN, INF = float("nan"), float("inf")
# two live episodes: slot 2 holds serial 7 (rows 4..8), slot 0 serial 9 (rows 0..2); slot 1 is not live
LIVE = [(2, 4, 5, 7), (0, 0, 3, 9)]


def _arena():
    w = np.array([1., 2., 3., -9., 1., 1., 1., 1., 1., -9.])
    cw = np.array([1., 3., 6., -9., 1., 2., 3., 4., 5., -9.])
    return w, cw, np.array([0.25, -9., 0.5])  # (t_w: weights given to add(), neither mean nor sum)


def test_reference_single_row_mean_and_sum():
    w, cw, t_w = _arena()
    w1, cw1, tw1, slots = pref.update(w, cw, t_w, LIVE, [7], [1], [[4.0, -2.0]], 1.0, 0.5, "mean")
    assert slots == {2}
    assert w1.tolist() == [1, 2, 3, -9, 1, 4.5, 2.5, 1, 1, -9]
    assert cw1.tolist() == [1, 3, 6, -9, 1, 5.5, 8, 9, 10, -9]
    assert tw1.tolist() == [0.25, -9, 2.0]  # slot 0 keeps the weight it was added with
    _, _, tw2, _ = pref.update(w, cw, t_w, LIVE, [7], [1], [[4.0, -2.0]], 1.0, 0.5, "sum")
    assert tw2.tolist() == [0.25, -9, 10.0]
    assert w.tolist() == _arena()[0].tolist() and cw.tolist() == _arena()[1].tolist()  # the inputs are not modified
    # [B] priorities address the window's first transition only
    w3, _, _, _ = pref.update(w, cw, t_w, LIVE, [7, 9], [4, 0], [3.0, 0.0], 1.0, 0.0, "sum")
    assert w3.tolist() == [0, 2, 3, -9, 1, 1, 1, 1, 3, -9]


def test_reference_power_and_epsilon():
    w, cw, t_w = _arena()
    w1, cw1, tw1, _ = pref.update(w, cw, t_w, LIVE, [9], [0], [[-8.75, 0.0, 15.75]], 0.5, 0.25, "sum")
    assert w1[:3].tolist() == [3.0, 0.5, 4.0] and cw1[:3].tolist() == [3.0, 3.5, 7.5] and tw1[0] == 7.5
    w0, _, _, _ = pref.update(w, cw, t_w, LIVE, [9], [1], [[0.0]], 0.0, 0.0, "sum")
    assert w0[1] == 1.0  # 0 ** 0, NumPy's and the C library's


def test_reference_last_valid_row_wins():
    w, cw, t_w = _arena()
    serial, start = [7, 7, 7, 7], [0, 0, 1, 0]
    prio = [[1.0, 2.0],    # row 0
            [5.0, NAN],    # row 1, the same window: its first element wins over row 0, its NaN does not shadow 2.0
            [INF, 6.0],    # row 2, overlapping: inf skipped (transition 1 stays row 0's 2.0), 6.0 on transition 2
            [-INF, NAN]]   # row 3, the highest: nothing valid, shadows nothing
    w1, cw1, tw1, slots = pref.update(w, cw, t_w, LIVE, serial, start, prio, 1.0, 0.0, "mean")
    assert slots == {2} and w1[4:9].tolist() == [5, 2, 6, 1, 1] and cw1[4:9].tolist() == [5, 7, 13, 14, 15]
    assert tw1[2] == 3.0
    # the same rows in another order: now 1.0 is the last valid assignment to transition 0
    w2, _, _, _ = pref.update(w, cw, t_w, LIVE, serial, start, [prio[1], prio[3], prio[2], prio[0]], 1.0, 0.0, "mean")
    assert w2[4:9].tolist() == [1, 2, 6, 1, 1]


def test_reference_skips_write_nothing():
    w, cw, t_w = _arena()
    rows = [(8, 0, 1.0),    # a serial inside the gap
            (6, 0, 1.0),    # below the oldest
            (10, 0, 1.0),   # above the newest
            (-1, -1, 1.0),  # a zero-filled sample row
            (7, -1, 1.0),   # a live serial with a negative start
            (7, 5, 1.0),    # the first row past the episode's end
            (9, 0, NAN), (9, 1, INF), (9, 2, -INF)]
    serial, start, prio = zip(*rows)
    w1, cw1, tw1, slots = pref.update(w, cw, t_w, LIVE, serial, start, prio, 0.6, 0.1, "sum")
    assert slots == set() and np.array_equal(w1, w) and np.array_equal(cw1, cw) and np.array_equal(tw1, t_w)
    # a window that runs past the end writes the part inside: transitions 3 and 4 of 5
    w2, _, _, slots = pref.update(w, cw, t_w, LIVE, [7], [3], [[2.0, 3.0, 4.0]], 1.0, 0.0, "sum")
    assert slots == {2} and w2.tolist() == [1, 2, 3, -9, 1, 1, 1, 2, 3, -9]  # row 9 (past the end) untouched


def test_header_and_bindings_agree_on_the_priority_entry():
    """(Its declaration, member list, size and offsets: tests/test_abi_cpu.py, for the whole ABI.)"""
    f = _lib.load(build_if_missing=True).mzs_replay_update_priorities
    assert f(None, None, None) == _lib.MZS_E_INVALID  # a null block is refused before any device call


def test_update_priorities_checks_its_arguments_before_any_device_use():
    b = mx.DeviceReplayBuffer(4, 100, random_seed=0)
    serial, start = np.array([0, 1, 1], np.int64), np.array([0, 3, 5], np.int32)
    with pytest.raises(ValueError, match="empty"):
        b.update_priorities((serial, start), np.ones(3))
    for T in (10, 20):
        b._place(T)
    dirty = b._dirty = False
    touched, clock = dict(b._touched), b._clock
    for bad in (np.ones(4), np.ones((4, 2)), np.ones((3, 0)), np.ones((3, 2, 1)), np.float32(1.0)):
        with pytest.raises(ValueError, match="priorities"):
            b.update_priorities((serial, start), bad)
    with pytest.raises(ValueError, match="serial and start"):
        b.update_priorities((serial, start[:2]), np.ones(3))
    with pytest.raises(ValueError, match="serial and start"):
        b.update_priorities((serial.reshape(3, 1), start), np.ones(3))
    with pytest.raises(ValueError, match="pair"):
        b.update_priorities(serial, np.ones(3))
    for alpha in (-0.1, 1.5, NAN):
        with pytest.raises(ValueError, match="alpha"):
            b.update_priorities((serial, start), np.ones(3), alpha=alpha)
    for eps in (-1e-9, INF, NAN):
        with pytest.raises(ValueError, match="eps"):
            b.update_priorities((serial, start), np.ones(3), eps=eps)
    with pytest.raises(ValueError, match="weight"):
        b.update_priorities((serial, start), np.ones(3), weight="median")
    # torch tensors are checked the same way; nothing above changed the bookkeeping or allocated anything
    with pytest.raises(ValueError, match="priorities"):
        b.update_priorities((torch.as_tensor(serial), torch.as_tensor(start)), torch.ones(2, 3))
    assert b._dirty is dirty and b._touched == touched and b._clock == clock and b._prio_scratch is None
    assert b._arena is None


def test_value_priorities_is_the_value_error_of_the_first_transition():
    model = train_model(2, 8, 4, seed=5, device="cpu")
    rng = np.random.default_rng(2)
    B, k = 6, 3
    obs = rng.uniform(-1, 1, (B, 1, 4)).astype(np.float32)
    Rn = rng.uniform(-5, 5, (B, k)).astype(np.float32)
    batch = mx.Transition(obs=obs, a=None, r=None, done=None, Rn=Rn, v=None, pi=None, w=None)
    def params():
        return [p for m in model.network if isinstance(m, torch.nn.Module) for p in m.parameters()]
    before = [p.detach().clone() for p in params()]
    got = vector.value_priorities(model, batch)
    assert isinstance(got, torch.Tensor) and got.shape == (B,) and got.dtype == torch.float32 and not got.requires_grad
    _, v, _ = model._root_inference_eager(torch.as_tensor(obs[:, 0]))
    assert torch.equal(got, (v - torch.as_tensor(Rn[:, 0])).abs()) and float(got.max()) > 0
    assert before and all(torch.equal(p, q) and q.grad is None for p, q in zip(before, params()))
    # the host buffer's batches carry obs as [B, k, obs_dim]: the same first column
    wide = mx.Transition(obs=np.repeat(obs, k, 1) + np.arange(k, dtype=np.float32)[None, :, None], a=None, r=None,
                         done=None, Rn=Rn, v=None, pi=None, w=None)
    assert torch.equal(vector.value_priorities(model, wide), got)


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
    """act() a function of the observation; update() reports what it was given, so the metrics follow the samples."""
    device, _support_size = torch.device("cpu"), 10

    def __init__(self):
        self.batches = []

    def init(self, key, sample):
        pass

    def act(self, key, obs, with_pi=False, with_value=False, **kw):
        obs = np.asarray(obs, np.float32)
        a = (obs.sum(1) % 2).astype(np.int64)
        pi = np.stack([a == 0, a == 1], 1).astype(np.float32)
        return (a, pi, obs.sum(1).astype(np.float64)) if with_pi else a

    def update(self, batch):
        self.batches.append(batch)
        return {"loss": float(np.sum(batch.Rn)) + float(np.sum(batch.obs))}


def _fit(**kw):
    model, rows = _Model(), []
    mx.fit_vector(model, _VecEnv(), _VecEnv(), n_step=2, gamma=0.9, buffer=mx.TrajectoryReplayBuffer(50, random_seed=4),
                  iterations=3, steps_per_iteration=10, num_simulations=2, k_steps=3, num_trajectory=4,
                  num_update_per_iteration=3, test_interval=10, random_seed=1, metrics=rows, **kw)
    for r in rows:
        r.pop("collect_s")
    return model, rows


def test_fit_vector_priority_update_leaves_a_buffer_without_the_method_alone():
    """The host buffer has no update_priorities: priority_update=True must change neither the samples (they are not
    asked for with indices) nor any metric."""
    assert not hasattr(mx.TrajectoryReplayBuffer, "update_priorities")
    m0, rows0 = _fit()
    m1, rows1 = _fit(priority_update=False)
    m2, rows2 = _fit(priority_update=True)
    assert len(rows0) == 3 and all("loss" in r for r in rows0) and len(m0.batches) == 9
    assert rows1 == rows0 and rows2 == rows0
    for x, y in zip(m0.batches, m2.batches):
        assert np.array_equal(x.obs, y.obs) and np.array_equal(x.Rn, y.Rn) and np.array_equal(x.w, y.w)


class _RecordingBuffer(mx.TrajectoryReplayBuffer):
    """The host buffer with the device buffer's two extras, recording what the loop hands over."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.calls = []

    def sample(self, *a, with_indices=False, **kw):
        batch = super().sample(*a, **kw)
        B = np.asarray(batch.Rn).shape[0]
        return (batch, (np.arange(B), np.zeros(B, np.int32))) if with_indices else batch

    def update_priorities(self, indices, priorities, alpha=1.0, eps=0.0, weight="mean"):
        self.calls.append((indices, priorities, alpha, eps, weight))


def test_fit_vector_priority_update_writes_back_after_every_update(monkeypatch):
    monkeypatch.setattr(vector, "value_priorities", lambda model, batch: ("p", len(model.batches), batch))
    for alpha, want in ((0.5, 0.5), (None, 1.0)):
        model, buf = _Model(), _RecordingBuffer(50, random_seed=4)
        mx.fit_vector(model, _VecEnv(), _VecEnv(), n_step=2, gamma=0.9, alpha=alpha, buffer=buf, iterations=2,
                      steps_per_iteration=10, num_simulations=2, k_steps=3, num_trajectory=4, num_update_per_iteration=3,
                      test_interval=10, random_seed=1, trajectory_weight="sum", priority_update=True)
        assert len(buf.calls) == len(model.batches) == 6
        for n, (indices, prio, a, eps, weight) in enumerate(buf.calls):
            # after update n + 1, with that update's own batch and its indices
            assert prio[0] == "p" and prio[1] == n + 1 and prio[2] is model.batches[n]
            assert len(indices[0]) == np.asarray(model.batches[n].Rn).shape[0]
            assert (a, eps, weight) == (want, 0.0, "sum")
        buf.calls.clear()
        mx.fit_vector(_Model(), _VecEnv(), _VecEnv(), n_step=2, gamma=0.9, alpha=alpha, buffer=buf, iterations=1,
                      steps_per_iteration=10, num_simulations=2, k_steps=3, num_trajectory=4, num_update_per_iteration=3,
                      test_interval=10, random_seed=1)
        assert buf.calls == []  # the default is off
