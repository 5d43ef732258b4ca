"""GPU tests of the priority write-back (replay_prio_mark_kernel / replay_prio_apply_kernel in
muax_amd/csrc/mz_replay.cuh): through the C ABI alone with the guarded buffers of tests/replay_abi.py against the
plain-loop reference tests/priority_reference.py, then through DeviceReplayBuffer.update_priorities and fit_vector.

ABI shapes: one arena with episodes of 1, 63, 64, 65 and 130 steps (below, at and above the 64-lane pass; two passes and
a tail), in an arena order that is not the ring's, the 130-step one ending exactly at max_steps; the ring wrapped
(capacity 7, head 5: slots 5, 6, 0, 1, 2 live, 3 and 4 holding the canary pattern); serials 10, 11, 12, 20, 21 (a gap);
kp 1 and 3; batches of 1, 5 and 9 rows (none a multiple of the four wavefronts of a workgroup).  Bars: with alpha == 1
nothing but a widening, an fabs and one addition happens, so w, cw and t_w equal the reference bit for bit; otherwise
w goes through one pow and is held to 1e-12 relative (the bar of test_gpu_replay_kernels.py for two libms) and to
exactly 0 where the reference is 0, and cw / t_w are bit for bit the sequential sum of the device's own w."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import muax_amd as mx
import priority_reference as pref
from helpers import train_model
from muax_amd import _lib
from replay_abi import Guarded, Replay

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
LENGTHS = (1, 63, 64, 65, 130)
SERIALS = (10, 11, 12, 20, 21)
CAPACITY, HEAD, GAP = 7, 5, 3
SLOTS = tuple((HEAD + i) % CAPACITY for i in range(5))
ARENA_ORDER = (1, 0, 3, 2, 4)  # the episodes as they lie in the arena; rows 0..4 and GAP rows before each are canaries
MAX_STEPS = 5 + sum(LENGTHS) + GAP * len(LENGTHS)
MODES = {1: "mean", 2: "sum"}
BIG = 2 ** 31 - 1

# (serial, start, priorities [3]); with kp == 1 the first priority alone
ROWS = {
    "nine": [
        (12, 10, (1.5, -2.25, 0.0)),    # negative and zero priorities
        (12, 10, (NAN, 3.0, INF)),      # exact duplicate, higher row: 3.0 wins; its NaN / inf leave row 0's 1.5 / 0.0
        (12, 11, (0.75, -INF, 4.0)),    # overlapping window: 0.75 over 3.0; -inf leaves transition 12 to row 0
        (3, 0, (9.0, 9.0, 9.0)),        # a serial below the oldest
        (15, 0, (9.0, 9.0, 9.0)),       # inside the gap
        (30, 0, (9.0, 9.0, 9.0)),       # above the newest
        (-1, -1, (9.0, 9.0, 9.0)),      # a zero-filled sample row
        (21, 128, (5.0, 6.0, 7.0)),     # runs past T = 130, which is the end of the arena: 128 and 129 only
        (11, -1, (8.0, 8.0, 8.0)),      # a live serial with start = -1
    ],
    "five": [
        (20, 64, (2.0, 2.5, 3.5)),      # the last transition of the 65-step episode (second pass); the rest past T
        (20, 65, (1.0, 1.0, 1.0)),      # start == T: nothing
        (10, 0, (-0.5, 1.0, 1.0)),      # the 1-step episode
        (20, 64, (INF, 1.0, 1.0)),      # duplicate of row 0 in a higher row, invalid: 2.0 stays
        (11, 62, (0.0, 1.0, 1.0)),      # the last transition of the 63-step episode, priority zero
    ],
    "one": [(21, 63, (1.25, NAN, 2.5))],  # across the 64-lane pass boundary of the 130-step episode, a NaN between
    "void": [(3, 0, (9.0, 9.0, 9.0)), (15, 5, (9.0, 9.0, 9.0)), (30, 0, (9.0, 9.0, 9.0)), (-1, -1, (9.0, 9.0, 9.0)),
             (12, BIG, (9.0, 9.0, 9.0))],  # no valid element at all (start + i beyond int32 included): nothing written
}
WRITTEN = {("nine", 1): {12, 21}, ("nine", 3): {12, 21}, ("five", 1): {20, 10, 11}, ("five", 3): {20, 10, 11},
           ("one", 1): {21}, ("one", 3): {21}, ("void", 1): set(), ("void", 3): set()}  # serials, by hand


def _u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _desc():
    dst, at = {}, 5
    for e in ARENA_ORDER:
        at += GAP
        dst[e] = at
        at += LENGTHS[e]
    assert at == MAX_STEPS and ARENA_ORDER[-1] == 4
    src = np.concatenate([[0], np.cumsum(LENGTHS)[:-1]])
    return np.array([[src[e], dst[e], LENGTHS[e], SLOTS[e]] for e in range(5)], np.int32)


DESC = _desc()
LIVE = [(int(d[3]), int(d[1]), int(d[2]), s) for d, s in zip(DESC, SERIALS)]


@functools.lru_cache(maxsize=None)
def _stream():
    rng = np.random.default_rng(23)
    M = sum(LENGTHS)
    return dict(obs=rng.uniform(-1, 1, (M, 2)), a=rng.integers(0, 2, M), pi=rng.dirichlet(np.ones(2), M),
                r=rng.uniform(-2, 3, M), v=rng.uniform(-30, 60, M), Rn=rng.uniform(-30, 60, M),
                done=rng.integers(0, 2, M), w=rng.uniform(0.1, 2.0, M), ep_w=rng.uniform(0.5, 1.5, 5))


def _fresh():
    """The arena after one store with given weights: t_w holds the ep_w of the add (neither mean nor sum of w)."""
    rp, st = Replay(MAX_STEPS, CAPACITY, 2, 2), _stream()
    assert rp.store(DESC, SERIALS, st["obs"], st["a"], st["pi"], st["r"], st["v"], raw=False, weight_mode=0,
                    ep_w=st["ep_w"], Rn=st["Rn"], done=st["done"], w=st["w"]) == _lib.MZS_OK
    return rp


def _update(rp, rows, kp, alpha=1.0, eps=0.0, mode=1, written=(), arena=None, **override):
    """mzs_replay_update_priorities on `rows`; only w / cw / t_w of the episodes with the serials `written` may change,
    and the inputs -- the scratch included, so it is back to -1 / 0 -- and every guard must be as they were."""
    serial = Guarded.of(np.array([r[0] for r in rows], np.int64))
    start = Guarded.of(np.array([r[1] for r in rows], np.int32))
    prio = Guarded.of(np.array([r[2][:kp] for r in rows], np.float32).reshape(len(rows), kp))
    owner = Guarded.of(np.full(rp.max_steps, -1, np.int32))
    touched = Guarded.of(np.zeros(rp.capacity, np.int32))
    u = _lib.MzsReplayUpdateArgs()
    u.struct_size = C.sizeof(_lib.MzsReplayUpdateArgs)
    u.head, u.count, u.batch, u.k_prio, u.weight_mode, u.alpha, u.eps = HEAD, 5, len(rows), kp, mode, alpha, eps
    u.serial, u.start, u.prio, u.owner, u.touched = serial.ptr, start.ptr, prio.ptr, owner.ptr, touched.ptr
    for k, x in override.items():
        setattr(u, k, x)
    rows_mask, slots_mask = np.zeros(rp.max_steps, bool), np.zeros(rp.capacity, bool)
    for slot, first, T, s in LIVE:
        if s in written:
            rows_mask[first:first + T] = True
            slots_mask[slot] = True
    may = {"w": rows_mask, "cw": rows_mask, "t_w": slots_mask} if written else {}
    return rp._call(rp.L.mzs_replay_update_priorities, (C.byref(arena if arena is not None else rp.arena), C.byref(u)),
                    may, [serial, start, prio, owner, touched])


def _reference(rp, rows, kp, alpha, eps, mode):
    prio = np.array([r[2][:kp] for r in rows], np.float32).reshape(len(rows), kp)
    return pref.update(rp.host("w"), rp.host("cw"), rp.host("t_w"), LIVE, [r[0] for r in rows], [r[1] for r in rows],
                       prio, alpha, eps, MODES[mode])


def _assert_matches(rp, want, alpha, mode, where):
    """The episodes the reference wrote (everything else is checked against `before` by the call itself)."""
    w, cw, t_w, slots = want
    H = {k: rp.host(k) for k in ("w", "cw", "t_w")}
    worst = 0.0
    for slot, first, T, s in LIVE:
        if slot not in slots:
            continue
        d = slice(first, first + T)
        if alpha == 1.0:
            assert np.array_equal(_u64(H["w"][d]), _u64(w[d])), (where, s, "w")
            assert np.array_equal(_u64(H["cw"][d]), _u64(cw[d])), (where, s, "cw")
            assert _u64(H["t_w"][slot]) == _u64(t_w[slot]), (where, s, "t_w")
            continue
        got, ref = H["w"][d], w[d]
        zero = ref == 0
        assert np.array_equal(_u64(got[zero]), _u64(ref[zero])), (where, s, "w where the reference is 0")
        err = np.abs(got[~zero] - ref[~zero]) / ref[~zero]
        worst = max(worst, float(err.max()) if err.size else 0.0)
        assert (err <= 1e-12).all(), (where, s, "w", err.max())
        seq = np.cumsum(got)  # the sequential float64 sum of the device's own w
        assert np.array_equal(_u64(H["cw"][d]), _u64(seq)), (where, s, "cw")
        assert _u64(H["t_w"][slot]) == _u64(seq[-1] / T if mode == 1 else seq[-1]), (where, s, "t_w")
    return worst


# ---- 1. the C ABI against the loop reference ----
@pytest.mark.parametrize("kp", [1, 3])
@pytest.mark.parametrize("case", list(ROWS))
def test_update_equals_the_loop_reference(case, kp):
    rows, worst = ROWS[case], 0.0
    assert len(rows) in (1, 5, 9)
    for alpha, eps in ((1.0, 0.0), (1.0, 0.375), (0.5, 0.0), (0.6, 1e-3)):
        for mode in MODES:
            rp = _fresh()
            want = _reference(rp, rows, kp, alpha, eps, mode)
            assert want[3] == {slot for slot, _, _, s in LIVE if s in WRITTEN[case, kp]}
            assert _update(rp, rows, kp, alpha, eps, mode, written=WRITTEN[case, kp]) == _lib.MZS_OK
            worst = max(worst, _assert_matches(rp, want, alpha, mode, (case, kp, alpha, eps, MODES[mode])))
    print(f"[w relative error max {worst:.2e}]", end=" ")


def test_the_highest_valid_row_wins_whatever_the_values():
    """The duplicate rule spelled out on the device's own output: transition 10 of serial 12 keeps row 0's 1.5 (row 1
    is a NaN there), 11 takes row 2's 0.75 over rows 0 and 1, 12 row 0's 0.0 (rows 1 and 2 are inf / -inf), 13 row 2's 4."""
    rp = _fresh()
    old = rp.host("w")
    assert _update(rp, ROWS["nine"], 3, 1.0, 0.0, 2, written={12, 21}) == _lib.MZS_OK
    first12, first21 = int(DESC[2][1]), int(DESC[4][1])
    w = rp.host("w")
    assert w[first12 + 10:first12 + 14].tolist() == [1.5, 0.75, 0.0, 4.0]
    assert w[first21 + 128:first21 + 130].tolist() == [5.0, 6.0] and first21 + 130 == MAX_STEPS
    keep = np.ones(64, bool)
    keep[10:14] = False
    assert np.array_equal(_u64(w[first12:first12 + 64][keep]), _u64(old[first12:first12 + 64][keep]))
    st = _stream()
    for e in (0, 1, 3):  # the episodes no valid element addresses keep the weight they were added with
        assert rp.host("t_w")[SLOTS[e]] == st["ep_w"][e]


def test_two_runs_give_identical_bits():
    out = []
    for _ in range(2):
        rp = _fresh()
        assert _update(rp, ROWS["nine"], 3, 0.6, 1e-3, 1, written={12, 21}) == _lib.MZS_OK
        out.append({k: rp.f[k].bits.clone() for k in ("w", "cw", "t_w")})
    for k in out[0]:
        assert torch.equal(out[0][k], out[1][k]), k


def test_a_second_call_reuses_the_scratch_it_was_left():
    """Two calls on the SAME scratch buffers (what DeviceReplayBuffer does): the second finds them clean."""
    rp = _fresh()
    rows = ROWS["five"]
    want = _reference(rp, rows, 3, 1.0, 0.0, 1)
    assert _update(rp, rows, 3, written=WRITTEN["five", 3]) == _lib.MZS_OK
    _assert_matches(rp, want, 1.0, 1, "first")
    want = _reference(rp, ROWS["nine"], 1, 1.0, 0.25, 2)
    assert _update(rp, ROWS["nine"], 1, 1.0, 0.25, 2, written=WRITTEN["nine", 1]) == _lib.MZS_OK
    _assert_matches(rp, want, 1.0, 2, "second")


REJECTED = [("struct_size", {"struct_size": C.sizeof(_lib.MzsReplayUpdateArgs) - 4}, "size mismatch"),
            ("head", {"head": -1}, "head"), ("head", {"head": CAPACITY}, "head"),
            ("count", {"count": -1}, "count"), ("count", {"count": CAPACITY + 1}, "count"),
            ("batch", {"batch": -1}, "batch"), ("k_prio", {"k_prio": 0}, "k_prio"), ("k_prio", {"k_prio": -3}, "k_prio"),
            ("weight_mode", {"weight_mode": 0}, "weight_mode"), ("weight_mode", {"weight_mode": 3}, "weight_mode"),
            ("alpha", {"alpha": -0.5}, "alpha"), ("alpha", {"alpha": 1.5}, "alpha"), ("alpha", {"alpha": NAN}, "alpha"),
            ("eps", {"eps": -1.0}, "eps"), ("eps", {"eps": INF}, "eps"), ("eps", {"eps": NAN}, "eps"),
            ("serial", {"serial": None}, "serial"), ("start", {"start": None}, "start"), ("prio", {"prio": None}, "prio"),
            ("owner", {"owner": None}, "owner"), ("touched", {"touched": None}, "touched")]


def test_rejected_arguments_write_nothing():
    rp = _fresh()  # (_call asserts that a refused call changed no byte of any buffer)
    for name, override, text in REJECTED:
        assert _update(rp, ROWS["five"], 3, **override) == _lib.MZS_E_INVALID, (name, override)
        message = rp.L.mzs_last_error(None).decode()
        assert "mzs_replay_update_priorities" in message and text in message, (name, override, message)
    bad = _lib.MzsReplayArena.from_buffer_copy(rp.arena)
    bad.struct_size -= 8
    assert _update(rp, ROWS["five"], 3, arena=bad) == _lib.MZS_E_INVALID
    # nothing to do is not an error, and needs no pointers
    nothing = dict(serial=None, start=None, prio=None, owner=None, touched=None)
    assert _update(rp, ROWS["five"], 3, batch=0, **nothing) == _lib.MZS_OK
    assert _update(rp, ROWS["five"], 3, count=0) == _lib.MZS_OK


# ---- 2. DeviceReplayBuffer.update_priorities ----
N, GAMMA, K = 3, 0.997, 4
EPISODES = (12, 20, 9)


def _filled(capacity=3, max_steps=64, seed=0):
    rng = np.random.default_rng(31)
    M = sum(EPISODES)
    st = dict(obs=rng.uniform(-1, 1, (M, 4)).astype(np.float32), a=rng.integers(0, 2, M), r=rng.uniform(-2, 3, M),
              v=rng.uniform(-30, 60, M), pi=rng.dirichlet(np.ones(2), M).astype(np.float32))
    buf = mx.DeviceReplayBuffer(capacity, max_steps, random_seed=seed)
    buf.add_raw(st["obs"], st["a"], st["r"], st["v"], st["pi"], list(EPISODES), N, GAMMA, 0.5, weight="mean")
    return buf, st


def _all_transitions(buf):
    serial = np.concatenate([np.full(e.length, e.serial, np.int64) for e in buf._eps])
    start = np.concatenate([np.arange(e.length, dtype=np.int32) for e in buf._eps])
    return serial, start


def _weights(buf):
    return {n: buf._t[n].clone() for n in ("w", "cw", "t_w")}


def test_the_sample_follows_the_one_nonzero_priority():
    """Every transition of every episode -- so every window start, and the tails that count towards an episode's
    weight -- gets priority 0 except one start of the 20-step episode: with alpha 1, eps 0 and the sum as the episode
    weight that start is the only draw left.  Then the priority moves, and the sample follows."""
    buf, _ = _filled()
    serial, start = _all_transitions(buf)
    prio = np.zeros(len(serial), np.float32)
    chosen = 7
    prio[(serial == 1) & (start == chosen)] = 2.5
    assert buf.update_priorities((serial, start), prio, alpha=1.0, eps=0.0, weight="sum") is None
    for key in (0, 1):
        batch, (s, i) = buf.sample(64, k_steps=K, key=key, with_indices=True)
        assert (s == 1).all() and (i == chosen).all()
        assert (batch.w[:, 0] == 2.5).all() and (batch.w[:, 1:] == 0).all()
    ep = buf.episode(1)
    assert float(ep.w.sum()) == 2.5 and buf._t["t_w"].cpu().tolist() == [0.0, 2.5, 0.0]
    moved = 15  # the last start of the 20-step episode with k_steps = 4
    dev = buf._device
    indices = (torch.tensor([1, 1], dtype=torch.int64, device=dev), torch.tensor([chosen, moved], dtype=torch.int32, device=dev))
    buf.update_priorities(indices, torch.tensor([0.0, -4.0], device=dev), alpha=1.0, weight="sum")
    _, (s, i) = buf.sample(64, k_steps=K, key=2, with_indices=True)
    assert (s == 1).all() and (i == moved).all() and float(buf.episode(1).w[moved]) == 4.0


def test_rows_of_an_evicted_episode_change_nothing():
    buf, st = _filled()
    _, (serial, start) = buf.sample(16, k_steps=K, key=5, with_indices=True)
    assert buf.serials == [0, 1, 2]
    buf.add_raw(st["obs"][:10], st["a"][:10], st["r"][:10], st["v"][:10], st["pi"][:10], [10], N, GAMMA, 0.5)
    assert buf.serials == [1, 2, 3]  # episode 0 went; its rows 0..11 still hold what it left
    before = {n: t.clone() for n, t in buf._t.items()}
    gone = torch.zeros_like(serial)  # every row names the evicted serial 0
    assert buf.update_priorities((gone, start), torch.full((16, 2), 3.0, device=buf._device), alpha=0.5) is None
    torch.cuda.synchronize()
    for n, was in before.items():
        assert torch.equal(buf._t[n], was), n
    # the sampled rows, live and evicted mixed: only live episodes change, and the call raises nothing
    buf.update_priorities((serial, start), torch.full((16,), 3.0, device=buf._device))
    torch.cuda.synchronize()
    new = buf._eps[-1]
    for n in ("w", "cw"):
        assert torch.equal(buf._t[n][new.start:new.start + 10], before[n][new.start:new.start + 10]), n
        assert torch.equal(buf._t[n][:12], before[n][:12]), n
    assert buf._t["t_w"][buf._eps[-1].slot] == before["t_w"][buf._eps[-1].slot]
    for n in ("obs", "a", "r", "Rn", "v", "done", "pi", "t_start", "t_len", "t_serial"):
        assert torch.equal(buf._t[n], before[n]), n
    live = serial != 0
    if bool(live.any()):
        assert not torch.equal(buf._t["w"], before["w"])


def test_update_marks_the_table_stale_and_leaves_the_staleness_order():
    buf, _ = _filled()
    buf.sample(4, k_steps=K, key=0)
    assert not buf._dirty
    touched, clock = dict(buf._touched), buf._clock
    buf.update_priorities((np.array([2]), np.array([0])), np.array([1.0]))
    assert buf._dirty and buf._touched == touched and buf._clock == clock
    scratch = buf._prio_scratch
    buf.update_priorities((np.array([2]), np.array([0])), np.array([[1.0, 2.0]]))
    assert buf._prio_scratch is scratch  # allocated once
    torch.cuda.synchronize()
    assert bool((scratch[0] == -1).all()) and bool((scratch[1] == 0).all())


def test_reanalyse_after_an_update_overwrites_the_weights_as_before():
    model = train_model(2, 8, 4, seed=3, support=10)
    out = []
    for update in (True, False):
        buf, _ = _filled()
        if update:
            serial, start = _all_transitions(buf)
            buf.update_priorities((serial, start), np.linspace(0.0, 9.0, len(serial)), alpha=0.6, eps=0.01, weight="sum")
        assert buf.reanalyse(model, 77, N, GAMMA, 0.5, weight="mean", chunk_rows=64, num_simulations=8) == sum(EPISODES)
        out.append(_weights(buf))
    for n in out[0]:
        assert torch.equal(out[0][n], out[1][n]), n


# ---- 3. fit_vector ----
class _Recording(mx.DeviceReplayBuffer):
    """The device buffer, keeping a copy of what every update_priorities call was given."""
    calls = None

    def update_priorities(self, indices, priorities, **kw):
        self.calls = (self.calls or []) + [(indices[0].clone(), indices[1].clone(), priorities.clone(), kw)]
        return super().update_priorities(indices, priorities, **kw)


def _fit_vector_once(seed, **kw):
    """The arguments of test_gpu_replay.py's _fit_vector_once, plus `kw`."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    from cartpole_env import VectorCartPole
    g = torch.Generator().manual_seed(0)
    net = mx.nn.MZNetwork(mx.nn.Representation(8, generator=g), mx.nn.Prediction(2, 21, generator=g),
                          mx.nn.Dynamic(8, 2, 21, generator=g))
    model = mx.MuZero(net, optimizer=mx.optimizers.create_optimizer("adam", 5e-3))
    buf, rows = _Recording(64, 4096, random_seed=seed), []
    mx.fit_vector(model, VectorCartPole(16, seed=0), VectorCartPole(2, max_episode_steps=20, seed=1), n_step=3, buffer=buf,
                  iterations=3, steps_per_iteration=8, num_simulations=8, k_steps=3, num_trajectory=8,
                  sample_per_trajectory=2, num_update_per_iteration=2, test_interval=10, random_seed=3, metrics=rows, **kw)
    return model, buf, rows


def test_fit_vector_writes_priorities_back():
    _, buf, rows = _fit_vector_once(13, priority_update=True)
    losses = [r["loss"] for r in rows if "loss" in r]
    assert len(rows) == 3 and losses and np.isfinite(losses).all() and len(buf) > 0
    # one write-back per update, with the loop's alpha (0.5) and trajectory weight
    assert len(buf.calls) == rows[-1]["training_step"] > 0
    assert all(kw == {"alpha": 0.5, "weight": "mean"} for *_, kw in buf.calls)
    # the last one (no add follows it) is in the arena: per transition the last row's |p| ** 0.5, one pow (1e-12)
    serial, start, prio, _ = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in buf.calls[-1])
    assert serial.shape == start.shape == prio.shape == (16,) and prio.dtype == np.float32 and (prio > 0).any()
    want = {(int(s), int(i)): float(np.float64(abs(p)) ** 0.5) for s, i, p in zip(serial, start, prio)}
    assert want and set(s for s, _ in want) <= set(buf.serials)
    for (s, i), w in want.items():
        got = float(buf.episode(s).w[i])
        assert abs(got - w) <= 1e-12 * w, (s, i, got, w)
    for e in buf._eps:  # whatever was written, every episode's prefix sums and weight follow from its w
        w = buf._t["w"][e.start:e.start + e.length].cpu().numpy()
        assert np.isfinite(w).all() and (w >= 0).all()
        seq = np.cumsum(w)
        assert np.array_equal(buf._t["cw"][e.start:e.start + e.length].cpu().numpy(), seq)
        # (exact where update_priorities wrote it; an episode it never touched keeps the NumPy mean of its add)
        assert abs(float(buf._t["t_w"][e.slot]) - seq[-1] / e.length) <= 1e-12 * seq[-1] / e.length
    _, buf2, rows2 = _fit_vector_once(13, priority_update=True)
    assert [r.get("loss") for r in rows2] == [r.get("loss") for r in rows] and buf2.serials == buf.serials
    assert all(torch.equal(buf.episode(s).w, buf2.episode(s).w) for s in buf.serials)
    _, buf0, _ = _fit_vector_once(13)
    assert buf0.calls is None  # the default is off
