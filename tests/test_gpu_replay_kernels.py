"""GPU tests of the five replay kernels (muax_amd/csrc/mz_replay.cuh) through the C ABI alone (tests/replay_abi.py:
guarded buffers, free descriptors), against the plain-loop float64 reference tests/nstep_reference.py for the n-step
fields and tests/replay_reference.py for the draws.

Shapes: the smallest that cross each boundary -- episode lengths around the 64-lane pass (63, 64, 65), two passes (127,
128, 129) and more (200); 9, 8 and 1 episodes for the four-wavefront workgroup's tail; n_step 1, below, at and above the
pass width and above every length; obs_dim / A of 1, small, and one past 128 / 64; the three regimes of the gather
kernel's padding; a table of more than 64 episodes with a wrapped head.  Bars: everything that is copied or that is
float64 arithmetic in a stated order is compared bit for bit; `w` alone goes through pow and is held to 1e-12 relative
(the project's bar for two libms) and to exactly 0 where the reference is 0."""
import functools

import numpy as np
import pytest
import torch

import muax_amd as mx
import nstep_reference as loop
import replay_reference as ref
from muax_amd import _lib
from replay_abi import Replay, layout

pytestmark = pytest.mark.gpu
F32 = np.float32
GAMMA = 0.997
CASES = {"nine": (1, 2, 63, 64, 65, 127, 128, 129, 200), "eight": (64, 1, 129, 2, 65, 63, 128, 127), "one": (129,)}
N_STEPS = (1, 5, 64, 300)
ALPHAS = (None, 0.5, 0.6, 1.0)
SHAPES = ((1, 1), (4, 2), (129, 65))  # (obs_dim, A)
MODES = {1: "mean", 2: "sum"}
CAPACITY = 12


def _u32(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def _u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _spans(lengths):
    first = np.concatenate([[0], np.cumsum(lengths)]).astype(int)
    return [slice(first[i], first[i + 1]) for i in range(len(lengths))]


@functools.lru_cache(maxsize=None)
def _rv(case):
    """(r, v) float64 streams of a case: general values, not representable in float32."""
    rng = np.random.default_rng(40 + len(CASES[case]))
    M = sum(CASES[case])
    return rng.uniform(-2, 3, M), rng.uniform(-30, 60, M)


@functools.lru_cache(maxsize=None)
def _rest(case, od, A):
    rng = np.random.default_rng(1000 * od + A + len(CASES[case]))
    M = sum(CASES[case])
    return (rng.uniform(-1, 1, (M, od)).astype(F32), rng.integers(0, A, M).astype(np.int32),
            rng.dirichlet(np.ones(A), M).astype(F32))


@functools.lru_cache(maxsize=None)
def _raw_reference(case, n, alpha):
    """Per episode (Rn, done, w, cw) of the loop reference on the float64 streams: once per (case, n, alpha)."""
    r, v = _rv(case)
    return [loop.episode(r[s].tolist(), v[s].tolist(), n, GAMMA, alpha)[:4] for s in _spans(CASES[case])]


def _max_steps(lengths, gap=3):
    return sum(lengths) + gap * len(lengths) + 5  # rows 0..4 belong to no episode either


def _assert_nstep_fields(rp, H, desc, want, mode, alpha, where):
    """Rn, done, w, cw and the table weight of every episode of `desc` against `want` [(Rn, done, w, cw)]."""
    worst = 0.0
    for (src, dst, T, slot), (Rn, done, w, cw) in zip(desc, want):
        d = slice(dst, dst + T)
        assert np.array_equal(_u32(H["Rn"][d]), _u32(np.array(Rn))), (where, T, "Rn")
        assert np.array_equal(H["done"][d], np.array(done, np.uint8)), (where, T, "done")
        got, w = H["w"][d], np.array(w)
        zero = w == 0
        assert np.array_equal(_u64(got[zero]), _u64(w[zero])), (where, T, "w where the reference is 0")
        err = np.abs(got[~zero] - w[~zero]) / w[~zero]
        assert (err <= 1e-12).all(), (where, T, "w", err.max())
        worst = max(worst, float(err.max()) if err.size else 0.0)
        if alpha is None:
            assert (got == 1.0).all(), (where, T)
        seq = np.cumsum(got)  # the sequential float64 sum of the device's own w
        assert np.array_equal(_u64(H["cw"][d]), _u64(seq)), (where, T, "cw")
        assert H["t_w"][slot] == (seq[-1] / T if mode == 1 else seq[-1]), (where, T, "t_w")
    rp.max_w_err = max(rp.max_w_err, worst)


# ---- 1. store, raw branch ----
@pytest.mark.parametrize("od,A", SHAPES)
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("n", N_STEPS)
def test_store_raw_equals_the_loop_reference(n, alpha, od, A):
    worst = 0.0
    for case, lengths in CASES.items():
        (r, v), (obs, a, pi) = _rv(case), _rest(case, od, A)
        want = _raw_reference(case, n, alpha)
        for mode in MODES:
            rp = Replay(_max_steps(lengths), CAPACITY, od, A)
            desc = layout(lengths, rp.max_steps, CAPACITY, seed=n + mode)
            serial = 7000 + 13 * np.arange(len(lengths))
            assert rp.store(desc, serial, obs, a, pi, r, v, raw=True, n=n, gamma=GAMMA, alpha=alpha,
                            weight_mode=mode) == _lib.MZS_OK
            H = {k: rp.host(k) for k in rp.f}
            for e, (src, dst, T, slot) in enumerate(desc):
                s, d = slice(src, src + T), slice(dst, dst + T)
                assert np.array_equal(_u32(H["r"][d]), _u32(r[s].astype(F32))) and \
                    np.array_equal(_u32(H["v"][d]), _u32(v[s].astype(F32))), (case, T)
                assert np.array_equal(H["a"][d], a[s]) and np.array_equal(_u32(H["obs"][d]), _u32(obs[s])) and \
                    np.array_equal(_u32(H["pi"][d]), _u32(pi[s])), (case, T)
                assert (H["t_start"][slot], H["t_len"][slot], H["t_serial"][slot]) == (dst, T, serial[e]), (case, T)
            _assert_nstep_fields(rp, H, desc, want, mode, alpha, (case, MODES[mode]))
            worst = max(worst, rp.max_w_err)
    print(f"[w relative error max {worst:.2e}]", end=" ")


def test_store_raw_with_values_equal_to_returns_has_zero_weights():
    """Zero rewards and zero values: v[t] == Rn[t] == 0 for every t, so w = 0 ** alpha = 0, cw = 0 and the table weight
    0 -- what an untrained net on a zero-reward task stores.  The episode between the two zero ones is general."""
    lengths, od, A = (65, 70, 128), 4, 2
    rng = np.random.default_rng(5)
    M = sum(lengths)
    r, v = rng.uniform(-2, 3, M), rng.uniform(-30, 60, M)
    r[:65] = v[:65] = 0.0
    r[135:] = v[135:] = 0.0
    obs, a, pi = rng.uniform(-1, 1, (M, od)), rng.integers(0, A, M), rng.dirichlet(np.ones(A), M)
    for alpha in (0.5, 0.6, 1.0):
        for mode in MODES:
            rp = Replay(_max_steps(lengths), CAPACITY, od, A)
            desc = layout(lengths, rp.max_steps, CAPACITY, seed=mode)
            assert rp.store(desc, [1, 2, 3], obs, a, pi, r, v, raw=True, n=5, gamma=GAMMA, alpha=alpha,
                            weight_mode=mode) == _lib.MZS_OK
            H = {k: rp.host(k) for k in rp.f}
            want = [loop.episode(r[s].tolist(), v[s].tolist(), 5, GAMMA, alpha)[:4] for s in _spans(lengths)]
            _assert_nstep_fields(rp, H, desc, want, mode, alpha, (alpha, mode))
            for e in (0, 2):
                src, dst, T, slot = desc[e]
                assert not H["w"][dst:dst + T].any() and not H["cw"][dst:dst + T].any() and H["t_w"][slot] == 0.0
                assert not H["Rn"][dst:dst + T].any()
            assert H["t_w"][desc[1][3]] > 0.0


# ---- 2. store, copy branch ----
@pytest.mark.parametrize("od,A", SHAPES)
def test_store_copy_branch_copies_and_scans(od, A):
    for case, lengths in CASES.items():
        rng = np.random.default_rng(60 + len(lengths))
        M = sum(lengths)
        obs, a, pi = _rest(case, od, A)
        r, v, Rn = (rng.uniform(-30, 60, M).astype(F32) for _ in range(3))
        done = rng.choice(np.array([0, 0, 1, 2, 128, 255], np.uint8), M)
        w = np.abs(rng.standard_normal(M)) ** 0.6  # general: the partial sums round
        ep_w = rng.uniform(0.1, 9.0, len(lengths))
        rp = Replay(_max_steps(lengths), CAPACITY, od, A)
        desc = layout(lengths, rp.max_steps, CAPACITY, seed=od)
        serial = 2 ** 40 + np.arange(len(lengths))
        assert rp.store(desc, serial, obs, a, pi, r, v, raw=False, ep_w=ep_w, Rn=Rn, done=done, w=w) == _lib.MZS_OK
        H = {k: rp.host(k) for k in rp.f}
        for e, (src, dst, T, slot) in enumerate(desc):
            s, d = slice(src, src + T), slice(dst, dst + T)
            for name, x in (("obs", obs), ("pi", pi), ("r", r), ("v", v), ("Rn", Rn)):
                assert np.array_equal(_u32(H[name][d]), _u32(x[s])), (case, T, name)
            assert np.array_equal(H["a"][d], a[s]) and np.array_equal(_u64(H["w"][d]), _u64(w[s])), (case, T)
            assert np.array_equal(H["done"][d], (done[s] != 0).astype(np.uint8)), (case, T)
            assert np.array_equal(_u64(H["cw"][d]), _u64(np.cumsum(w[s]))), (case, T)
            assert (H["t_start"][slot], H["t_len"][slot], H["t_serial"][slot]) == (dst, T, serial[e]), (case, T)
            assert H["t_w"][slot] == ep_w[e], (case, T)


# ---- 3. reanalyse ----
@functools.lru_cache(maxsize=None)
def _new_values(case):
    """The searched values of a reanalysis, by episode in the store's stream order (float32)."""
    rng = np.random.default_rng(70 + len(CASES[case]))
    return rng.uniform(-30, 60, sum(CASES[case])).astype(F32)


@functools.lru_cache(maxsize=None)
def _reanalyse_reference(case, n, alpha):
    """Per episode (Rn, done, w, cw) of the loop reference on the STORED float32 rewards and the new values."""
    r32, v = _rv(case)[0].astype(F32), _new_values(case)
    return [loop.episode(r32[s].tolist(), v[s].tolist(), n, GAMMA, alpha)[:4] for s in _spans(CASES[case])]


def _selection(E):
    """Which episodes a reanalysis takes, in its stream order: a subset, not in arena, slot or store order."""
    order = list(range(E))[::-1]
    if E > 2:
        order = order[1:2] + order[3:] + order[:1]  # (the third from the end is left out)
    return order


@pytest.mark.parametrize("od,A", SHAPES)
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("n", N_STEPS)
def test_reanalyse_equals_the_loop_reference_on_stored_rewards(n, alpha, od, A):
    worst = 0.0
    for case, lengths in CASES.items():
        (r, v), (obs, a, pi) = _rv(case), _rest(case, od, A)
        spans, v_new, want_all = _spans(lengths), _new_values(case), _reanalyse_reference(case, n, alpha)
        rng = np.random.default_rng(80 + od)
        pi_new_all = rng.dirichlet(np.ones(A), sum(lengths)).astype(F32)
        for mode in MODES:
            rp = Replay(_max_steps(lengths), CAPACITY, od, A)
            stored = layout(lengths, rp.max_steps, CAPACITY, seed=n + mode)
            assert rp.store(stored, np.arange(len(lengths)), obs, a, pi, r, v, raw=True, n=3, gamma=0.9, alpha=0.5,
                            weight_mode=3 - mode) == _lib.MZS_OK
            sel = _selection(len(lengths))
            rows = sum(lengths[e] for e in sel)
            pad = 7
            desc, pi_s, v_s, at = [], np.full((rows + pad, A), np.nan, F32), np.full(rows + pad, np.nan, F32), 0
            for e in sel:
                T = lengths[e]
                desc.append([at, stored[e][1], T, stored[e][3]])
                pi_s[at:at + T], v_s[at:at + T] = pi_new_all[spans[e]], v_new[spans[e]]
                at += T
            desc = np.array(desc, np.int32)
            # (what must stay -- obs, a, r, the table's other columns, every row of no selected episode -- is the
            # harness's check: reanalyse() may write pi, v, Rn, done, w, cw of the selected rows and t_w of their slots)
            assert rp.reanalyse(desc, pi_s, v_s, n, GAMMA, alpha, mode, stream_rows=rows,
                                rows_padded=rows + pad) == _lib.MZS_OK
            H = {k: rp.host(k) for k in rp.f}
            for src, dst, T, slot in desc:
                assert np.array_equal(_u32(H["pi"][dst:dst + T]), _u32(pi_s[src:src + T])), (case, T)
                assert np.array_equal(_u32(H["v"][dst:dst + T]), _u32(v_s[src:src + T])), (case, T)
            _assert_nstep_fields(rp, H, desc, [want_all[e] for e in sel], mode, alpha, (case, MODES[mode]))
            worst = max(worst, rp.max_w_err)
    print(f"[w relative error max {worst:.2e}]", end=" ")


def test_reanalyse_refuses_weight_mode_zero_and_writes_nothing():
    case, lengths, od, A = "eight", CASES["eight"], 4, 2
    (r, v), (obs, a, pi) = _rv(case), _rest(case, od, A)
    rp = Replay(_max_steps(lengths), CAPACITY, od, A)
    desc = layout(lengths, rp.max_steps, CAPACITY)
    assert rp.store(desc, np.arange(8), obs, a, pi, r, v, raw=True, n=5, gamma=GAMMA, alpha=0.5, weight_mode=1) == _lib.MZS_OK
    before = rp.snapshot()
    # (a refused call may write nothing at all: the harness compares every buffer)
    assert rp.reanalyse(desc, pi, _new_values(case), 5, GAMMA, 0.5, weight_mode=0) == _lib.MZS_E_INVALID
    assert rp.reanalyse(desc, pi, _new_values(case), 0, GAMMA, 0.5, weight_mode=1) == _lib.MZS_E_INVALID
    after = rp.snapshot()
    assert all(torch.equal(after[k], before[k]) for k in before)


@pytest.mark.parametrize("alpha", [None, 0.5, 0.6])
@pytest.mark.parametrize("n", N_STEPS)
def test_reanalysing_with_the_stored_results_changes_nothing(n, alpha):
    """Metamorphic: with float32-representable rewards and values the raw store and the reanalysis read the same
    numbers, so reanalysing with the stored pi and v must leave every arena and the table bit-identical."""
    od, A = 4, 2
    for case, lengths in CASES.items():
        (r, v), (obs, a, pi) = _rv(case), _rest(case, od, A)
        r, v = r.astype(F32).astype(np.float64), v.astype(F32).astype(np.float64)
        for mode in MODES:
            rp = Replay(_max_steps(lengths), CAPACITY, od, A)
            desc = layout(lengths, rp.max_steps, CAPACITY, seed=mode)
            assert rp.store(desc, np.arange(len(lengths)), obs, a, pi, r, v, raw=True, n=n, gamma=GAMMA, alpha=alpha,
                            weight_mode=mode) == _lib.MZS_OK
            before = rp.snapshot()
            assert rp.reanalyse(desc, pi, v.astype(F32), n, GAMMA, alpha, mode) == _lib.MZS_OK
            after = rp.snapshot()
            for k in before:
                assert torch.equal(after[k], before[k]), (case, mode, k)


# ---- 4. gather ----
GATHER_EPISODES = {1: (5,), 3: (5, 64, 2), 6: (3, 65, 1, 130, 7, 64)}
PAD_ROWS = {1: (0, 1, 1024, 1025, 64512, 64513, 70000),  # floats: no pad wave; 1; 1; 2; 63; the cap of 64; 64, striding
            129: (0, 1, 7, 8, 500, 501, 543)}            # 0; 129; 903; 1 032; 64 500; 64 629; 70 047 floats


@pytest.mark.parametrize("episodes", sorted(GATHER_EPISODES))
@pytest.mark.parametrize("od", sorted(PAD_ROWS))
def test_gather_copies_the_rows_and_zeroes_the_padding(od, episodes):
    lengths = GATHER_EPISODES[episodes]
    rp = Replay(_max_steps(lengths), CAPACITY, od, 1)
    stored = layout(lengths, rp.max_steps, CAPACITY, seed=episodes)
    rng = np.random.default_rng(90 + od)
    obs = rng.uniform(-1, 1, (rp.max_steps, od)).astype(F32)
    for _, dst, T, _ in stored:  # (the rows of no episode stay the NaN pattern)
        rp.f["obs"].t[dst:dst + T] = torch.from_numpy(obs[dst:dst + T]).cuda()
    order = list(range(episodes))[::-1]  # stream order: the reverse of the store's
    desc, at = [], 0
    for e in order:
        desc.append([at, stored[e][1], lengths[e], stored[e][3]])
        at += lengths[e]
    desc, rows = np.array(desc, np.int32), at
    for pad in PAD_ROWS[od]:
        rc, out = rp.gather(desc, rows, rows + pad)  # (the guards behind rows_padded: the harness's check)
        assert rc == _lib.MZS_OK and out.shape == (rows + pad, od)
        for src, dst, T, _ in desc:
            assert np.array_equal(out[src:src + T], _u32(obs[dst:dst + T])), (pad, T)
        assert not out[rows:].any(), (pad, int(np.flatnonzero(out[rows:].reshape(-1))[0]))  # every bit: +0.0


# ---- 5. refresh ----
@pytest.mark.parametrize("head", [0, 100])
@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
def test_refresh_builds_the_compact_table(count, head):
    cap, k = 130, 5
    rng = np.random.default_rng(110)
    t_len = rng.integers(k + 1, 80, cap)
    t_len[::3] = rng.integers(1, k + 1, len(t_len[::3]))  # a third carries no probability ...
    t_len[[0, 3, 99, 129]] = k                            # ... some of them exactly k long
    t_len[[1, 100, 128]] = k + 1
    t_w = rng.uniform(0.0, 7.0, cap)                      # general: the partial sums round
    t_start, t_serial = rng.integers(0, 2 ** 31 - 1, cap), rng.integers(0, 2 ** 62, cap)
    rp = Replay(8, cap, 1, 1)
    live = (head + np.arange(count)) % cap
    for name, x in (("t_len", t_len), ("t_w", t_w), ("t_start", t_start), ("t_serial", t_serial)):
        rp.f[name].t[torch.from_numpy(live).cuda()] = torch.from_numpy(x[live]).to(rp.f[name].dtype).cuda()
    assert rp.refresh(head, count, k) == _lib.MZS_OK  # (entries >= count untouched: the harness's check)
    CW = np.cumsum(np.where(t_len[live] > k, t_w[live], 0.0))
    assert np.array_equal(_u64(rp.host("c_CW")[:count]), _u64(CW))
    assert np.array_equal(rp.host("c_start")[:count], t_start[live])
    assert np.array_equal(rp.host("c_len")[:count], t_len[live])
    assert np.array_equal(rp.host("c_serial")[:count], t_serial[live])


# ---- 6. sample ----
SAMPLE_CAP, SAMPLE_HEAD = 130, 100


@functools.lru_cache(maxsize=None)
def _sample_case(k, od, A):
    """130 episodes stored by the copy branch into shuffled rows and slots; `eps`: the episodes oldest first (slot
    head, head + 1, ... wrapping), with dyadic weights.  A third are no longer than k; position 7 is k + 1 long and
    position 11 has all-zero transition weights, both with a large buffer weight so that rows land on them."""
    rng = np.random.default_rng(120 + k)
    slots = rng.permutation(SAMPLE_CAP)                # slot of every episode, in the order they are stored
    age = (slots - SAMPLE_HEAD) % SAMPLE_CAP           # 0: the oldest
    lengths, store_eps = [], []
    for i in age:
        T = int(rng.integers(1, k + 1)) if i % 3 == 0 else k + 1 if i % 6 == 1 else int(rng.integers(k + 2, k + 70))
        T = k if i in (3, 9) else k + 1 if i == 7 else k + 40 if i == 11 else T
        lengths.append(T)
        if i in (7, 11):
            store_eps.append(ref.make_episode(rng, T, A, od, w=None if i == 7 else np.zeros(T), weight=8192.0))
        else:
            store_eps.append(ref.make_episode(rng, T, A, od))
    rp = Replay(_max_steps(lengths, gap=1), SAMPLE_CAP, od, A)
    desc = layout(lengths, rp.max_steps, SAMPLE_CAP, seed=k, gap=1)
    desc[:, 3] = slots
    order = np.argsort(age)  # store index by age
    cat = {n: np.concatenate([ep[n] for ep in store_eps]) for n in ("obs", "a", "r", "Rn", "v", "done", "pi", "w")}
    serial = 5000 + np.arange(SAMPLE_CAP)
    assert rp.store(desc, serial, cat["obs"], cat["a"], cat["pi"], cat["r"], cat["v"], raw=False,
                    ep_w=[ep["weight"] for ep in store_eps], Rn=cat["Rn"], done=cat["done"].astype(np.uint8),
                    w=cat["w"]) == _lib.MZS_OK
    assert rp.refresh(SAMPLE_HEAD, SAMPLE_CAP, k) == _lib.MZS_OK
    return rp, [store_eps[e] for e in order], serial[order]


def _assert_rows(got, eps, e, s, k):
    want = ref.batch_fields(eps, e, s, k)
    B = len(e)
    assert np.array_equal(_u32(got["obs"]), _u32(want["obs"].reshape(B, -1)))
    for n in ("r", "Rn", "v", "pi", "w"):
        assert got[n].shape == want[n].shape and np.array_equal(_u32(got[n]), _u32(want[n])), n
    assert np.array_equal(got["a"], want["a"]) and np.array_equal(got["done"], want["done"].astype(np.uint8))


@pytest.mark.parametrize("od,A", [(1, 1), (129, 65)])
@pytest.mark.parametrize("k", [1, 5, 64, 65])
def test_sample_draws_and_windows_equal_the_reference(k, od, A):
    rp, eps, serial = _sample_case(k, od, A)
    lengths = np.array([len(ep["w"]) for ep in eps])
    hit_one = hit_zero = 0
    for B, spt in ((1, 3), (3, 2), (4, 3), (5, 3), (257, 3)):
        key = [900 + B, k]
        rc, got = rp.sample(SAMPLE_CAP, B, k, spt, key)
        assert rc == _lib.MZS_OK
        e, s = ref.sample_indices(key, eps, B, k, spt)
        assert np.array_equal(got["serial"], serial[e]) and np.array_equal(got["start"], s), B
        _assert_rows(got, eps, e, s, k)
        assert (lengths[e] > k).all()
        assert (got["start"][lengths[e] == k + 1] == 0).all()
        _, u1 = ref.draws(key, B, spt)
        on_zero = e == 11
        assert np.array_equal(got["start"][on_zero], np.floor(u1[on_zero] * 40).astype(np.int32))
        hit_one, hit_zero = hit_one + int((e == 7).sum()), hit_zero + int(on_zero.sum())
    assert hit_one and hit_zero  # (both edge episodes were drawn)


@pytest.mark.parametrize("k", [1, 5, 65])
@pytest.mark.parametrize("newest", ["longer", "exactly k", "one step"])
def test_sample_with_every_table_weight_zero_lands_on_the_newest_episode(newest, k):
    """with every buffer weight zero the draw lands on the newest episode; when that one is no longer than
    k_steps the row is zero-filled with serial -1 and start -1."""
    od, A, B = 4, 2, 257
    lengths = [k + 4, k + 2, {"longer": k + 3, "exactly k": k, "one step": 1}[newest]]
    rng = np.random.default_rng(130 + k)
    eps = [ref.make_episode(rng, T, A, od, weight=0.0) for T in lengths]
    rp = Replay(_max_steps(lengths), 3, od, A)
    desc = layout(lengths, rp.max_steps, 3, seed=k)
    head = 1
    desc[:, 3] = (head + np.arange(3)) % 3  # slots by age from the head: episode 2 is the newest
    cat = {n: np.concatenate([ep[n] for ep in eps]) for n in ("obs", "a", "r", "Rn", "v", "done", "pi", "w")}
    assert rp.store(desc, [10, 11, 12], cat["obs"], cat["a"], cat["pi"], cat["r"], cat["v"], raw=False, ep_w=[0.0] * 3,
                    Rn=cat["Rn"], done=cat["done"].astype(np.uint8), w=cat["w"]) == _lib.MZS_OK
    assert rp.refresh(head, 3, k) == _lib.MZS_OK
    assert not rp.host("c_CW").any()
    key = [77, k]
    rc, got = rp.sample(3, B, k, 3, key)
    assert rc == _lib.MZS_OK
    if newest == "longer":
        _, u1 = ref.draws(key, B, 3)
        s = np.array([ref.pick_start(u, eps[2]["w"], k) for u in u1])
        assert (got["serial"] == 12).all() and np.array_equal(got["start"], s) and len(np.unique(s)) == 3
        _assert_rows(got, eps, np.full(B, 2), s, k)
    else:
        assert (got["serial"] == -1).all() and (got["start"] == -1).all()
        for n in ("obs", "a", "r", "Rn", "v", "done", "pi", "w"):
            assert not got[n].view(np.uint8).any(), n  # every byte zero (+0.0, not the pattern)


@pytest.mark.parametrize("newest_long", [False, True])
def test_public_route_to_all_zero_weights(newest_long):
    """The same state through DeviceReplayBuffer: add_raw with alpha on zero rewards and zero values gives w = 0 and
    table weights 0; sample() then draws the newest episode, or zero rows when that one is no longer than k_steps."""
    k, od, A, B = 5, 4, 2, 64
    lengths = [k, k + 3] if newest_long else [k + 3, k]
    M = sum(lengths)
    rng = np.random.default_rng(140)
    obs, a, pi = rng.uniform(-1, 1, (M, od)).astype(F32), rng.integers(0, A, M), rng.dirichlet(np.ones(A), M).astype(F32)
    buf = mx.DeviceReplayBuffer(4, 64)
    buf.add_raw(obs, a, np.zeros(M), np.zeros(M), pi, lengths, 10, GAMMA, alpha=0.5, weight="mean")
    assert not buf._t["w"].any() and not buf._t["t_w"].any()
    key = [3, 4]
    batch, (serial, start) = buf.sample(B, k_steps=k, key=key, with_indices=True)
    serial, start = serial.cpu().numpy(), start.cpu().numpy()
    if newest_long:
        _, u1 = ref.draws(key, B)
        assert (serial == 1).all() and np.array_equal(start, np.floor(u1 * 3).astype(np.int32))
        assert np.array_equal(batch.obs.cpu().numpy()[:, 0], obs[k + start])
        assert np.array_equal(batch.pi.cpu().numpy(), np.stack([pi[k + s:k + s + k] for s in start]))
        assert np.array_equal(batch.done.cpu().numpy(), np.ones((B, k), bool)) and not batch.w.any()  # (n = 10 > T)
    else:
        assert (serial == -1).all() and (start == -1).all()
        for n in ("obs", "a", "r", "Rn", "v", "done", "pi", "w"):
            assert not getattr(batch, n).any(), n
