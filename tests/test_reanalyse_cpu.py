"""CPU tests of the reanalysis path's host parts: the stream plan, the NumPy restatement the GPU tests compare the
write-back kernel with (tests/reanalyse_reference.py), the staleness order and the ABI declarations.  No GPU, no kernel."""
import numpy as np
import pytest

import muax_amd as mx
import reanalyse_reference as rref
from muax_amd import _build, _lib, replay_device, vector

NEW = ("mzs_replay_gather_obs", "mzs_replay_reanalyse")


def test_plan_of_episodes_that_straddle_chunks():
    p = replay_device.reanalyse_plan([1, 9, 10, 11, 32, 70], 64)
    assert list(p.offsets) == [0, 1, 10, 20, 31, 63]
    assert (p.stream_rows, p.n_chunks, p.rows_padded) == (133, 3, 192)
    offsets, rows, chunks, padded = p  # (it unpacks in that order)
    assert (rows, chunks, padded) == (133, 3, 192)


def test_plan_at_exact_multiples_and_a_single_row():
    p = replay_device.reanalyse_plan([64], 64)
    assert (list(p.offsets), p.stream_rows, p.n_chunks, p.rows_padded) == ([0], 64, 1, 64)
    p = replay_device.reanalyse_plan([32, 32, 64], 64)
    assert (list(p.offsets), p.stream_rows, p.n_chunks, p.rows_padded) == ([0, 32, 64], 128, 2, 128)
    p = replay_device.reanalyse_plan([65], 64)
    assert (p.stream_rows, p.n_chunks, p.rows_padded) == (65, 2, 128)
    p = replay_device.reanalyse_plan([1], 4096)
    assert (list(p.offsets), p.stream_rows, p.n_chunks, p.rows_padded) == ([0], 1, 1, 4096)
    p = replay_device.reanalyse_plan(np.array([1]), 1)
    assert (list(p.offsets), p.stream_rows, p.n_chunks, p.rows_padded) == ([0], 1, 1, 1)
    for bad in ([], [3, 0]):
        with pytest.raises(ValueError):
            replay_device.reanalyse_plan(bad, 64)
    with pytest.raises(ValueError):
        replay_device.reanalyse_plan([3], 0)


@pytest.mark.parametrize("alpha", [0.5, None])
def test_reference_agrees_with_episode_trajectory(alpha):
    rng = np.random.default_rng(11)
    T, A, n, gamma = 47, 3, 10, 0.997
    r = rng.uniform(-2, 3, T).astype(np.float32)
    v = rng.uniform(-30, 60, T).astype(np.float32)
    pi = rng.dirichlet(np.ones(A), T).astype(np.float32)
    Rn, done, w, cw, weight = rref.targets(r, pi, v, n, gamma, alpha, "mean")
    tr = vector.episode_trajectory(rng.uniform(-1, 1, (T, 4)), rng.integers(0, A, T), r, v, pi, n, gamma, alpha)
    _, _, _, t_done, t_Rn, _, _, t_w = tr._rows
    assert Rn.dtype == np.float32 and np.array_equal(Rn, t_Rn.astype(np.float32))
    assert done.dtype == bool and np.array_equal(done, t_done) and done[-n:].all() and not done[:-n].any()
    assert w.dtype == np.float64 and np.array_equal(w, t_w) and np.array_equal(cw, np.cumsum(t_w))
    assert weight == tr.weights.mean() and rref.targets(r, pi, v, n, gamma, alpha, "sum")[4] == tr.weights.sum()
    if alpha is None:
        assert (w == 1.0).all()


def test_header_and_bindings_agree_on_the_reanalysis_entries():
    """(Declarations, sizes and layouts: tests/test_abi_cpu.py, for the whole ABI.)"""
    assert "mz_replay.hip" in _build.UNITS and "mz_replay.cuh" in _build.UNITS["mz_replay.hip"]
    lib = _lib.load(build_if_missing=True)
    for s in NEW:
        # a null block is refused before any device call
        assert getattr(lib, s)(None, None, None) == _lib.MZS_E_INVALID


def test_stalest_and_argument_checks_need_no_device():
    """The staleness order is host bookkeeping (a counter per serial, advanced by every placement and every
    reanalysis); so are the checks reanalyse() makes before it launches anything."""
    b = mx.DeviceReplayBuffer(4, 100, random_seed=0)
    assert b.stalest(3) == []
    for T in (10, 20, 30):
        b._place(T)
    assert b.stalest(5) == [0, 1, 2] and b.stalest(2) == [0, 1] and b.stalest(0) == []
    with pytest.raises(KeyError):
        b.reanalyse(None, 0, 10, 0.997, serials=[7])
    with pytest.raises(ValueError, match="more than once"):
        b.reanalyse(None, 0, 10, 0.997, serials=[1, 1])
    with pytest.raises(ValueError, match="weight"):
        b.reanalyse(None, 0, 10, 0.997, weight="median")
    b._place(30)
    b._place(40)  # no room after row 90: evicts 0, 1 and 2 (rows 0..60), lands at row 0
    assert b.serials == [3, 4] and b.stalest(9) == [3, 4] and set(b._touched) == {3, 4}
    b.clear()
    assert b.stalest(9) == [] and b.reanalyse(None, 0, 10, 0.997) == 0
