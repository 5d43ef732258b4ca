"""The two collection entry points of the C ABI (mzs_replay_stage, mzs_replay_store_steps; muax_amd/csrc/mz_replay.cuh)
called directly, with tests/replay_abi.py's guarded buffers: every byte a call may not write must be unchanged.

The store from the ring is compared (a) bit for bit, in every arena field, `cw` and the table rows, with
mzs_replay_store's raw route fed the same episodes as a dense stream (both run the same arithmetic, so there is no
tolerance), and (b) with the plain loops of tests/collect_reference.py: the integer and fp32 fields and Rn bit for bit;
w, cw and t_w bit for bit with alpha none or 1, else within the relative 1e-12 tests/test_gpu_priority.py uses for the
device pow."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import collect_reference as cref
from muax_amd import _lib
from replay_abi import ARENA, GUARD, Guarded, Replay

pytestmark = pytest.mark.gpu
N_ENVS, GAMMA = 3, 0.997
SHAPES = [(3, 2), (5, 18)]
RING_FIELDS = {"obs": torch.float32, "a": torch.int32, "r": torch.float64, "v": torch.float32, "pi": torch.float32}
TABLE_WRITTEN = ("t_start", "t_len", "t_w", "t_serial")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Ring:
    """A guarded collection ring of `steps` x N rows, filled from host arrays or left as the pattern."""

    def __init__(self, steps, N, obs_dim, A, rng=None):
        self.steps, self.N, self.obs_dim, self.A = steps, N, obs_dim, A
        rows = steps * N
        self.host = None
        if rng is not None:
            self.host = dict(obs=rng.uniform(-1, 1, (steps, N, obs_dim)).astype(np.float32),
                             a=rng.integers(0, A, (steps, N)).astype(np.int32), r=rng.uniform(-2, 3, (steps, N)),
                             v=rng.uniform(-30, 60, (steps, N)).astype(np.float32),
                             pi=rng.dirichlet(np.ones(A), (steps, N)).astype(np.float32))
            self.f = {k: Guarded.of(x.reshape(rows, -1) if x.ndim == 3 else x.reshape(rows)) for k, x in self.host.items()}
        else:
            widths = {"obs": obs_dim, "pi": A}
            self.f = {k: Guarded(rows, widths.get(k, 1), dt, flat=k not in widths) for k, dt in RING_FIELDS.items()}
        g = _lib.MzsReplayRing()
        g.struct_size = C.sizeof(_lib.MzsReplayRing)
        g.device = torch.cuda.current_device()
        g.ring_steps, g.num_envs, g.obs_dim, g.num_actions = steps, N, obs_dim, A
        for k, x in self.f.items():
            setattr(g, k, x.ptr)
        self.c = g

    def stage(self, row, obs, a, v, pi, edit=None):
        """One mzs_replay_stage; afterwards only ring row `row` of obs, a, v, pi may differ, no guard may, and the
        inputs are unchanged.  `edit(ring struct, args)` spoils an argument first.  Returns the status."""
        ins = dict(obs=Guarded.of(obs), a=Guarded.of(a), v=Guarded.of(v), pi=Guarded.of(pi))
        s = _lib.MzsReplayStageArgs()
        s.struct_size = C.sizeof(_lib.MzsReplayStageArgs)
        s.row = row
        for k, x in ins.items():
            setattr(s, k, x.ptr)
        ring = _lib.MzsReplayRing.from_buffer_copy(self.c)
        if edit:
            edit(ring, s)
        torch.cuda.synchronize()
        before = {k: x.bits.clone() for k, x in self.f.items()}
        kept = {k: x.bits.clone() for k, x in ins.items()}
        rc = _lib.load().mzs_replay_stage(C.byref(ring), C.byref(s), _stream())
        torch.cuda.synchronize()
        mine = np.zeros(self.steps * self.N, bool)
        if rc == _lib.MZS_OK:
            mine[row * self.N:(row + 1) * self.N] = True
        for k, x in self.f.items():
            assert x.guards_intact(), k
            same = x.bits == before[k]
            if k != "r":
                same |= x.row_mask(mine)
            assert bool(same.all()), f"stage: {k} changed outside row {row}"
        for k, x in ins.items():
            assert torch.equal(x.bits, kept[k]), k
        return rc


def _store_steps(rep, ring, desc, serial, n, alpha, weight_mode, edit=None):
    """One mzs_replay_store_steps through Replay._call: only the rows and slots the descriptors cover may change."""
    desc = np.ascontiguousarray(desc, np.int32)
    g = dict(desc=Guarded.of(desc.reshape(-1)), serial=Guarded.of(np.asarray(serial, np.int64)),
             gpow=Guarded.of(np.array([GAMMA ** i for i in range(max(int(n), 0) + 1)], np.float64)))
    a = _lib.MzsReplayStoreStepsArgs()
    a.struct_size = C.sizeof(_lib.MzsReplayStoreStepsArgs)
    a.episodes, a.n_step, a.weight_mode = len(desc), int(n), int(weight_mode)
    a.has_alpha, a.alpha = int(alpha is not None), float(alpha if alpha is not None else 0.0)
    a.desc_host = desc.ctypes.data
    for k, x in g.items():
        setattr(a, k, x.ptr)
    c_ring = _lib.MzsReplayRing.from_buffer_copy(ring.c)
    if edit:
        edit(c_ring, a)
    rows, slots = np.zeros(rep.max_steps, bool), np.zeros(rep.capacity, bool)
    for _, _, T, dst, slot in desc:
        if T > 0 and 0 <= dst and dst + T <= rep.max_steps and 0 <= slot < rep.capacity:
            rows[dst:dst + T] = True
            slots[slot] = True
    may = {k: rows for k in ARENA}
    may.update({k: slots for k in TABLE_WRITTEN})
    return rep._call(rep.L.mzs_replay_store_steps, (C.byref(rep.arena), C.byref(c_ring), C.byref(a)), may,
                     list(g.values()) + list(ring.f.values()))


def _place(episodes, capacity, gap=3):
    """[(env, first ring row, length)] -> (descriptors [E, 5], max_steps): arena rows from the end downwards in a
    shuffled order with `gap` uncovered rows before each -- the first one placed ends exactly at max_steps -- and
    shuffled table slots."""
    rng = np.random.default_rng(len(episodes))
    max_steps = sum(T for _, _, T in episodes) + gap * len(episodes)
    at, dst = max_steps, {}
    for e in rng.permutation(len(episodes)):
        at -= episodes[e][2]
        dst[e] = at
        at -= gap
    slots = rng.permutation(capacity)[:len(episodes)]
    desc = [[env, first, T, dst[e], slots[e]] for e, (env, first, T) in enumerate(episodes)]
    assert max(d[3] + d[2] for d in desc) == max_steps
    return np.array(desc, np.int32), max_steps


# the ring of 70 rows: an episode of 65 steps whose rows wrap past the ring's end (rows 40..69, 0..34), one of 64 that
# ends exactly on the last ring row, one of 63, and single steps (the first and the last ring row among them);
# the ring of 140 rows: 130 steps, wrapping, and a single step
CASES = {70: [(0, 40, 65), (1, 6, 64), (2, 3, 63), (1, 0, 1), (2, 69, 1), (0, 37, 1)],
         140: [(1, 100, 130), (0, 139, 1)]}
CAPACITY = 8


@functools.lru_cache(maxsize=None)
def _ring(steps, obs_dim, A):
    return Ring(steps, N_ENVS, obs_dim, A, np.random.default_rng(1000 * steps + 10 * obs_dim + A))


def _dense(ring, desc):
    """The same episodes as a dense stream for mzs_replay_store (raw): (descriptors [E, 4], stream fields)."""
    eps = [cref.ring_episode(ring.host, ring.steps, int(d[0]), int(d[1]), int(d[2])) for d in desc]
    src = np.concatenate([[0], np.cumsum(desc[:, 2])[:-1]])
    d4 = np.stack([src, desc[:, 3], desc[:, 2], desc[:, 4]], 1).astype(np.int32)
    return d4, {k: np.concatenate([e[k] for e in eps]) for k in ("obs", "a", "r", "v", "pi")}


@functools.lru_cache(maxsize=None)
def _stored(steps, obs_dim, A, n, weight_mode, alpha):
    """The episodes of CASES[steps] stored from the ring (guards checked by Replay._call); shared by the two tests."""
    ring = _ring(steps, obs_dim, A)
    desc, max_steps = _place(CASES[steps], CAPACITY)
    serial = 100 + np.arange(len(desc))
    rep = Replay(max_steps, CAPACITY, obs_dim, A)
    assert _store_steps(rep, ring, desc, serial, n, alpha, weight_mode) == _lib.MZS_OK
    return ring, desc, max_steps, serial, rep


_CASES = [pytest.mark.parametrize("alpha", [None, 1.0, 0.5]), pytest.mark.parametrize("weight_mode", [1, 2]),
          pytest.mark.parametrize("n", [1, 5]), pytest.mark.parametrize("obs_dim,A", SHAPES),
          pytest.mark.parametrize("steps", [70, 140])]


def _cases(fn):
    for mark in _CASES:
        fn = mark(fn)
    return fn


@_cases
def test_store_from_the_ring_equals_the_dense_raw_store(steps, obs_dim, A, n, weight_mode, alpha):
    """mzs_replay_store (raw) fed the same episodes as a dense stream: every bit of every arena field, cw and table."""
    ring, desc, max_steps, serial, rep = _stored(steps, obs_dim, A, n, weight_mode, alpha)
    dense = Replay(max_steps, CAPACITY, obs_dim, A)
    d4, st = _dense(ring, desc)
    assert dense.store(d4, serial, st["obs"], st["a"], st["pi"], st["r"], st["v"].astype(np.float64), raw=True, n=n,
                       gamma=GAMMA, alpha=alpha, weight_mode=weight_mode) == _lib.MZS_OK
    for k in rep.f:
        assert torch.equal(rep.f[k].bits, dense.f[k].bits), k


@_cases
def test_store_from_the_ring_against_the_loop_reference(steps, obs_dim, A, n, weight_mode, alpha):
    """The plain loops of tests/collect_reference.py: integer and fp32 fields and Rn bit for bit; w, cw, t_w bit for bit
    with alpha none or 1 (the kernels execute no pow for alpha == 1.0: the device pow(x, 1.0) was measured 2.1e-16
    relative off x), else within 1e-12 relative."""
    ring, desc, max_steps, serial, rep = _stored(steps, obs_dim, A, n, weight_mode, alpha)
    want = cref.expected_store(ring.host, steps, desc, n, GAMMA, alpha, "mean" if weight_mode == 1 else "sum")
    got = {k: rep.host(k) for k in list(ARENA) + list(TABLE_WRITTEN)}
    worst, checks = 0.0, []
    for x, s in zip(want, serial):
        rows = slice(x["dst"], x["dst"] + x["length"])
        for k in ("obs", "a", "r", "v", "pi", "Rn"):
            assert got[k][rows].dtype == x[k].dtype and np.array_equal(got[k][rows], x[k]), (k, x["length"])
        assert np.array_equal(got["done"][rows].astype(bool), x["done"])
        assert got["t_start"][x["slot"]] == x["dst"] and got["t_len"][x["slot"]] == x["length"]
        assert got["t_serial"][x["slot"]] == s
        for mine, ref in ((got["w"][rows], x["w"]), (got["cw"][rows], x["cw"]),
                          (got["t_w"][x["slot"]:x["slot"] + 1], np.array([x["t_w"]]))):
            worst = max(worst, float((np.abs(mine - ref) / np.abs(ref)).max()))
            checks.append((mine, ref, x["length"]))
    print(f"[w, cw, t_w: worst relative error {worst:.1e}]", end=" ")
    for mine, ref, T in checks:
        if alpha is None or alpha == 1.0:
            assert np.array_equal(mine, ref), (T, worst)
        else:
            assert (np.abs(mine - ref) <= 1e-12 * np.abs(ref)).all(), (T, worst)


@pytest.mark.parametrize("obs_dim,A", SHAPES)
@pytest.mark.parametrize("row", [0, 69, 33])
def test_stage_writes_its_row_and_nothing_else(row, obs_dim, A):
    rng = np.random.default_rng(row)
    ring = Ring(70, N_ENVS, obs_dim, A)
    obs = rng.uniform(-1, 1, (N_ENVS, obs_dim)).astype(np.float32)
    a = rng.integers(0, A, N_ENVS).astype(np.int32)
    v = rng.uniform(-3, 3, N_ENVS).astype(np.float32)
    pi = rng.dirichlet(np.ones(A), N_ENVS).astype(np.float32)
    assert ring.stage(row, obs, a, v, pi) == _lib.MZS_OK
    rows = slice(row * N_ENVS, (row + 1) * N_ENVS)
    assert np.array_equal(ring.f["obs"].host()[rows], obs) and np.array_equal(ring.f["pi"].host()[rows], pi)
    assert np.array_equal(ring.f["a"].host()[rows], a) and np.array_equal(ring.f["v"].host()[rows], v)


def _set(name, value, on_ring=False):
    def edit(ring, args):
        setattr(ring if on_ring else args, name, value)
    return edit


STAGE_REFUSALS = {
    "row below the ring": _set("row", -1), "row past the ring": _set("row", 70),
    "null obs": _set("obs", None), "null a": _set("a", None), "null v": _set("v", None), "null pi": _set("pi", None),
    "null ring field": _set("pi", None, on_ring=True), "args struct_size": _set("struct_size", 8),
    "ring struct_size": _set("struct_size", C.sizeof(_lib.MzsReplayRing) - 8, on_ring=True),
    "no environments": _set("num_envs", 0, on_ring=True),
}


@pytest.mark.parametrize("what", list(STAGE_REFUSALS))
def test_stage_refuses_before_any_launch(what):
    ring = Ring(70, N_ENVS, 3, 2)
    z = np.zeros
    rc = ring.stage(5, z((N_ENVS, 3), np.float32), z(N_ENVS, np.int32), z(N_ENVS, np.float32), z((N_ENVS, 2), np.float32),
                    edit=STAGE_REFUSALS[what])
    assert rc == _lib.MZS_E_INVALID


def _desc_edit(row, col, value):
    def change(desc):
        desc[row, col] = value
    return change


STORE_REFUSALS = {  # (change of the descriptors, or None; change of the structs, or None)
    "environment past the ring": (_desc_edit(1, 0, N_ENVS), None),
    "negative environment": (_desc_edit(1, 0, -1), None),
    "length zero": (_desc_edit(0, 2, 0), None),
    "length above ring_steps": (_desc_edit(0, 2, 71), None),
    "first row past the ring": (_desc_edit(2, 1, 70), None),
    "negative first row": (_desc_edit(2, 1, -1), None),
    "arena range past max_steps": (_desc_edit(0, 3, 10 ** 6), None),
    "negative arena row": (_desc_edit(0, 3, -1), None),
    "slot past the table": (_desc_edit(1, 4, CAPACITY), None),
    "negative slot": (_desc_edit(1, 4, -1), None),
    "n_step zero": (None, _set("n_step", 0)),
    "weight_mode 0": (None, _set("weight_mode", 0)),
    "weight_mode 3": (None, _set("weight_mode", 3)),
    "args struct_size": (None, _set("struct_size", 8)),
    "ring struct_size": (None, _set("struct_size", 8, on_ring=True)),
    "null gpow": (None, _set("gpow", None)),
    "null device descriptors": (None, _set("desc", None)),
    "ring of another obs_dim": (None, _set("obs_dim", 4, on_ring=True)),
    "no episodes": (None, _set("episodes", 0)),
}


@pytest.mark.parametrize("what", list(STORE_REFUSALS))
def test_store_steps_refuses_before_any_launch(what):
    ring = _ring(70, 3, 2)
    desc, max_steps = _place(CASES[70], CAPACITY)
    change, edit = STORE_REFUSALS[what]
    if change:
        desc = desc.copy()
        change(desc)
    rep = Replay(max_steps, CAPACITY, 3, 2)
    rc = _store_steps(rep, ring, desc, np.arange(len(desc)), 5, 0.5, 1, edit=edit)
    assert rc == _lib.MZS_E_INVALID  # (Replay._call has checked that not one byte changed)
    assert GUARD > 0
