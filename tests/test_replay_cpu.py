"""CPU tests of the device replay's specification (tests/replay_reference.py, the NumPy restatement the GPU tests
compare the kernels with) and of its ABI entries' declarations.  No GPU, no kernel."""
import numpy as np
import pytest

import muax_amd as mx
import replay_reference as ref
from muax_amd import _build, _lib


def test_uniform53_known_answers():
    """Random123's threefry2x32 known answers (20 rounds): key 0, counter 0 -> 6b200159 99ba4efe; key and counter all
    ones -> 1cb996fc bb002be7; the uniform is the top 53 of those 64 bits times 2^-53."""
    u = ref.uniform53([0, 0], 0, 0)
    assert u.dtype == np.float64
    assert float(u) == 0xd64002b333749 * 2.0 ** -53 == float.fromhex("0x1.ac80056666e92p-2")
    ones = 0xFFFFFFFF
    assert float(ref.uniform53([ones, ones], ones, ones)) == 0x39732df976005 * 2.0 ** -53
    u = ref.uniform53([7, 9], np.arange(1000), 1)
    assert u.shape == (1000,) and (u >= 0).all() and (u < 1).all() and len(np.unique(u)) == 1000


def _within_5_sigma(counts, p, n):
    sigma = np.sqrt(n * p * (1 - p))
    assert (np.abs(counts - n * p) <= 5 * sigma).all(), (counts, n * p, sigma)


def test_episode_frequencies_follow_the_weights():
    n, w = 200_000, np.array([1., 2., 3., 4., 6.])
    u0, _ = ref.draws([3, 4], n)
    e = ref.pick_episodes(u0, w, [50] * 5, 5)
    _within_5_sigma(np.bincount(e, minlength=5), w / w.sum(), n)
    # an episode no longer than k carries no probability: its share goes to the others in proportion
    e = ref.pick_episodes(u0, w, [50, 5, 50, 4, 50], 5)
    counts = np.bincount(e, minlength=5)
    assert counts[1] == 0 and counts[3] == 0
    _within_5_sigma(counts[[0, 2, 4]], w[[0, 2, 4]] / 10.0, n)


def test_rows_of_one_trajectory_share_their_episode():
    u0, u1 = ref.draws([1, 2], 12, sample_per_trajectory=3)
    assert (u0.reshape(4, 3) == u0.reshape(4, 3)[:, :1]).all() and len(np.unique(u0)) == 4
    assert len(np.unique(u1)) == 12


def test_start_frequencies_follow_the_transition_weights():
    n, k = 200_000, 5
    w = np.array([1., 0., 2., 5., 0.5, 1.5, 3., 4., 9., 9., 9., 9., 9.])  # the last k can never start a window
    m = len(w) - k
    _, u1 = ref.draws([5, 6], n)
    cw = np.cumsum(w)[:m]
    s = np.searchsorted(cw, u1 * cw[-1], side="right")
    assert s.max() < m and [ref.pick_start(u1[j], w, k) for j in range(50)] == s[:50].tolist()
    counts = np.bincount(s, minlength=m)
    assert counts[1] == 0
    _within_5_sigma(counts, w[:m] / w[:m].sum(), n)
    # all-zero weights: uniform over the m starts
    s0 = np.array([ref.pick_start(x, np.zeros(len(w)), k) for x in u1[:20_000]])
    _within_5_sigma(np.bincount(s0, minlength=m), np.full(m, 1 / m), 20_000)


def test_window_contents_against_direct_slicing():
    rng = np.random.default_rng(0)
    k, A, od = 5, 3, 4
    eps = [ref.make_episode(rng, T, A, od) for T in (6, 7, 37)]
    e, start = ref.sample_indices([0, 1], eps, 64, k)
    b = ref.batch_fields(eps, e, start, k)
    assert b["obs"].shape == (64, 1, od) and b["pi"].shape == (64, k, A) and b["w"].dtype == np.float32
    for j in range(64):
        ep, s = eps[e[j]], start[j]
        assert 0 <= s < len(ep["w"]) - k
        assert np.array_equal(b["obs"][j, 0], ep["obs"][s])
        for n in ("a", "r", "Rn", "v", "done", "pi"):
            assert np.array_equal(b[n][j], ep[n][s:s + k]), n
        assert np.array_equal(b["w"][j], ep["w"][s:s + k].astype(np.float32))
    assert (start[e == 0] == 0).all()  # length k + 1: one possible start


def test_arena_model_evicts_oldest_first_and_keeps_episodes_contiguous():
    m = ref.ArenaModel(5, 300)
    for T in (30, 120, 100):
        m.add(T)
    assert m.serials == [0, 1, 2] and m.steps == 250
    m.add(90)   # no room after row 250 nor below episode 0: 0 and 1 go, the new one starts at row 0
    assert m.serials == [2, 3] and m.live[-1][1] == 0
    for T in (10, 10, 10, 10):
        m.add(T)  # the count, not the room, evicts now
    assert m.serials == [3, 4, 5, 6, 7] and len(m.live) == 5


def test_header_and_bindings_agree_on_the_replay_entries():
    """(Declarations, sizes and layouts: tests/test_abi_cpu.py, for the whole ABI.)"""
    assert "mz_replay.hip" in _build.UNITS
    lib = _lib.load(build_if_missing=True)  # (resolves every entry)
    # a null / mis-sized block is refused before any device call
    assert lib.mzs_replay_sample(None, None, None) == _lib.MZS_E_INVALID


def test_host_bookkeeping_needs_no_device():
    """Placement, eviction, len / steps / capacity are host arithmetic; an oversized episode is a ValueError."""
    b = mx.DeviceReplayBuffer(5, 300, random_seed=0)
    assert len(b) == 0 and not b and b.capacity == 5 and b.steps == 0 and b.max_steps == 300
    model = ref.ArenaModel(5, 300)
    for T in (30, 120, 100, 90, 60, 45, 110, 300, 1):
        b._place(T)
        model.add(T)
        assert b.serials == model.serials and b.steps == model.steps and len(b) == len(model.live)
    with pytest.raises(ValueError, match="max_steps"):
        b._place_all([10, 301])
    assert b.serials == model.serials  # nothing was placed
    b.clear()
    assert len(b) == 0 and b.steps == 0
    with pytest.raises(ValueError, match="empty"):
        b.sample(4)
    assert issubclass(mx.DeviceReplayBuffer, mx.replay_buffer.BaseReplayBuffer)
