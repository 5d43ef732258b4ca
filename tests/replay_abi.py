"""The five replay entry points of the C ABI (mzs_replay_store / _refresh / _sample / _gather_obs / _reanalyse) called
directly through muax_amd._lib: no DeviceReplayBuffer, no act().  For test_gpu_replay_kernels.py.

Every buffer a kernel sees -- arena, table, input stream, descriptor, output -- is a view into a larger tensor with
GUARD elements on each side, and the whole tensor, the view included, starts as a recognisable pattern: the NaN with
payload 0x5A5A... for floats, 0x5A bytes for integers.  So arena rows that no descriptor covers are canaries too.  Every
call is given the rows it MAY write; after it everything else -- guards, uncovered rows, table entries of other slots,
every input -- must be bit-identical to what it was, and the guards must still be the pattern.  The descriptors are the
caller's: stream order, arena order and slots are free, an episode may end exactly at max_steps."""
import ctypes as C

import numpy as np
import torch

from muax_amd import _lib

GUARD = 64  # elements on each side of every view
ARENA = {"obs": torch.float32, "a": torch.int32, "r": torch.float32, "Rn": torch.float32, "v": torch.float32,
         "done": torch.uint8, "pi": torch.float32, "w": torch.float64, "cw": torch.float64}
TABLE = {"t_start": torch.int32, "t_len": torch.int32, "t_w": torch.float64, "t_serial": torch.int64,
         "c_start": torch.int32, "c_len": torch.int32, "c_CW": torch.float64, "c_serial": torch.int64}
_INT_OF = {torch.float32: torch.int32, torch.float64: torch.int64, torch.int32: torch.int32, torch.int64: torch.int64,
           torch.uint8: torch.uint8}
_PATTERN = {torch.float32: 0x7FC5A5A5, torch.float64: 0x7FF85A5A5A5A5A5A, torch.int32: 0x5A5A5A5A,
            torch.int64: 0x5A5A5A5A5A5A5A5A, torch.uint8: 0x5A}


class Guarded:
    """`rows` x `width` elements of `dtype` between two guards; `.t` is the typed view [rows, width] (or [rows]),
    `.bits` the whole backing tensor as integers of the same size."""

    def __init__(self, rows, width, dtype, flat=True, device="cuda"):
        self.rows, self.width, self.dtype = int(rows), int(width), dtype
        n = self.rows * self.width
        self.bits = torch.full((n + 2 * GUARD,), _PATTERN[dtype], dtype=_INT_OF[dtype], device=device)
        inner = self.bits[GUARD:GUARD + n].view(dtype)
        self.t = inner if flat and self.width == 1 else inner.view(self.rows, self.width)

    @classmethod
    def of(cls, array, dtype=None):
        """A guarded device copy of a host array ([rows] or [rows, width])."""
        x = torch.as_tensor(np.ascontiguousarray(array))
        x = x if dtype is None else x.to(dtype)
        g = cls(x.shape[0], x.shape[1] if x.ndim == 2 else 1, x.dtype, flat=x.ndim == 1)
        g.t.copy_(x)
        return g

    @property
    def ptr(self):
        return self.t.data_ptr()

    def host(self):
        return self.t.cpu().numpy()

    def guards_intact(self):
        n = self.rows * self.width
        both = torch.cat([self.bits[:GUARD], self.bits[GUARD + n:]])
        return bool((both == _PATTERN[self.dtype]).all())

    def row_mask(self, rows):
        """Element mask over `.bits`: True where row index (into the view) is in the boolean vector `rows`."""
        m = torch.zeros(self.bits.shape, dtype=torch.bool, device=self.bits.device)
        m[GUARD:GUARD + self.rows * self.width] = torch.as_tensor(rows, device=m.device).repeat_interleave(self.width)
        return m


def layout(lengths, max_steps, capacity, seed=0, gap=3):
    """Descriptors [E, 4] (stream row, arena row, length, slot) for episodes that lie back to back in the stream in
    the order given, in the arena in a shuffled order with `gap` uncovered rows before each, the last one ending
    exactly at max_steps, and in shuffled table slots."""
    rng = np.random.default_rng(seed)
    E = len(lengths)
    assert sum(lengths) + gap * E <= max_steps and E <= capacity
    order = rng.permutation(E)
    dst, at = np.zeros(E, np.int64), max_steps
    for e in order:  # from the end of the arena downwards
        at -= lengths[e]
        dst[e] = at
        at -= gap
    slots = rng.permutation(capacity)[:E]
    src = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    return np.stack([src, dst, np.asarray(lengths), slots], 1).astype(np.int32)


class Replay:
    """Guarded arenas and tables of one replay store, and the five calls."""

    def __init__(self, max_steps, capacity, obs_dim, A):
        self.max_steps, self.capacity, self.obs_dim, self.A = int(max_steps), int(capacity), int(obs_dim), int(A)
        self.L = _lib.load()
        widths = {"obs": self.obs_dim, "pi": self.A}
        self.f = {n: Guarded(self.max_steps, widths.get(n, 1), dt, flat=n not in widths) for n, dt in ARENA.items()}
        self.f.update({n: Guarded(self.capacity, 1, dt) for n, dt in TABLE.items()})
        ar = _lib.MzsReplayArena()
        ar.struct_size = C.sizeof(_lib.MzsReplayArena)
        ar.device = torch.cuda.current_device()
        ar.max_steps, ar.capacity, ar.obs_dim, ar.num_actions = self.max_steps, self.capacity, self.obs_dim, self.A
        for n, g in self.f.items():
            setattr(ar, n, g.ptr)
        self.arena = ar
        self.max_w_err = 0.0  # (a test may record here what it measured)

    # ---- bookkeeping of what a call may write
    def snapshot(self):
        torch.cuda.synchronize()
        return {n: g.bits.clone() for n, g in self.f.items()}

    def host(self, name):
        return self.f[name].host()

    def _call(self, fn, args, may_write, others=()):
        """Run one entry point; afterwards only `may_write` ({field: boolean row vector}) may differ, and no guard of
        the store's buffers or of `others` (inputs: wholly unchanged; outputs: listed as (Guarded, True)) may."""
        before = self.snapshot()
        kept = [(g, g.bits.clone()) for g in others if not isinstance(g, tuple)]
        outs = [g for g in others if isinstance(g, tuple)]
        rc = fn(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        if rc != _lib.MZS_OK:
            may_write = {}
        for n, g in self.f.items():
            assert g.guards_intact(), f"{fn.__name__}: a guard of {n} was overwritten"
            same = g.bits == before[n]
            if n in may_write:
                same |= g.row_mask(may_write[n])
            assert bool(same.all()), f"{fn.__name__}: {n} changed outside the rows it may write " \
                                     f"(first at element {int((~same).nonzero()[0]) - GUARD} of the view)"
        for g, was in kept:
            assert torch.equal(g.bits, was), f"{fn.__name__}: an input was written"
        for g, _ in outs:
            assert g.guards_intact(), f"{fn.__name__}: a guard of an output was overwritten"
        return rc

    def _covered(self, desc):
        rows = np.zeros(self.max_steps, bool)
        slots = np.zeros(self.capacity, bool)
        for _, dst, T, slot in np.asarray(desc):
            rows[dst:dst + T] = True
            slots[slot] = True
        return rows, slots

    # ---- the five calls
    def store(self, desc, serial, obs, a, pi, r, v, raw, n=0, gamma=1.0, alpha=None, weight_mode=0, ep_w=None,
              Rn=None, done=None, w=None):
        """`raw`: r, v float64 streams; else r, v, Rn float32, done uint8, w float64 and ep_w.  Returns the status."""
        desc = np.ascontiguousarray(desc, np.int32)
        g = dict(desc=Guarded.of(desc.reshape(-1)), serial=Guarded.of(np.asarray(serial, np.int64)),
                 obs=Guarded.of(obs, torch.float32), a=Guarded.of(a, torch.int32), pi=Guarded.of(pi, torch.float32),
                 r=Guarded.of(r, torch.float64 if raw else torch.float32),
                 v=Guarded.of(v, torch.float64 if raw else torch.float32))
        if ep_w is not None:
            g["ep_w"] = Guarded.of(np.asarray(ep_w, np.float64))
        if raw:
            g["gpow"] = Guarded.of(np.array([float(gamma) ** i for i in range(int(n) + 1)], np.float64))
        else:
            g.update(Rn=Guarded.of(Rn, torch.float32), done=Guarded.of(done, torch.uint8), w=Guarded.of(w, torch.float64))
        s = _lib.MzsReplayStoreArgs()
        s.struct_size = C.sizeof(_lib.MzsReplayStoreArgs)
        s.episodes, s.stream_steps = len(desc), len(g["a"].t)
        s.raw, s.n_step, s.weight_mode = int(raw), int(n), int(weight_mode)
        s.has_alpha, s.alpha = int(alpha is not None), float(alpha if alpha is not None else 0.0)
        s.desc_host = desc.ctypes.data
        for k, x in g.items():
            setattr(s, k, x.ptr)
        rows, slots = self._covered(desc)
        may = {k: rows for k in ARENA}
        may.update({k: slots for k in ("t_start", "t_len", "t_w", "t_serial")})
        return self._call(self.L.mzs_replay_store, (C.byref(self.arena), C.byref(s)), may, list(g.values()))

    def refresh(self, head, count, k):
        may = {k_: np.arange(self.capacity) < count for k_ in ("c_start", "c_len", "c_CW", "c_serial")}
        return self._call(self.L.mzs_replay_refresh, (C.byref(self.arena), int(head), int(count), int(k)), may)

    def sample(self, count, B, k, spt, key):
        """Returns (status, {field: host array}); the outputs start as the pattern."""
        shapes = dict(obs=(B, self.obs_dim, torch.float32), a=(B, k, torch.int32), r=(B, k, torch.float32),
                      Rn=(B, k, torch.float32), v=(B, k, torch.float32), done=(B, k, torch.uint8),
                      pi=(B, k * self.A, torch.float32), w=(B, k, torch.float32), serial=(B, 1, torch.int64),
                      start=(B, 1, torch.int32))
        out = {n: Guarded(rows, width, dt, flat=False) for n, (rows, width, dt) in shapes.items()}
        s = _lib.MzsReplaySampleArgs()
        s.struct_size = C.sizeof(_lib.MzsReplaySampleArgs)
        s.count, s.batch, s.k_steps, s.sample_per_trajectory = int(count), int(B), int(k), int(spt)
        s.key[0], s.key[1] = int(key[0]), int(key[1])
        for n, g in out.items():
            setattr(s, n, g.ptr)
        rc = self._call(self.L.mzs_replay_sample, (C.byref(self.arena), C.byref(s)), {}, [(g, True) for g in out.values()])
        got = {n: g.host() for n, g in out.items()}
        got["pi"] = got["pi"].reshape(B, k, self.A)
        got["serial"], got["start"] = got["serial"][:, 0], got["start"][:, 0]
        return rc, got

    def gather(self, desc, stream_rows, rows_padded):
        """Returns (status, the stream [rows_padded, obs_dim] as float32 bit patterns (uint32))."""
        desc = np.ascontiguousarray(desc, np.int32)
        d = Guarded.of(desc.reshape(-1))
        out = Guarded(rows_padded, self.obs_dim, torch.float32, flat=False)
        a = _lib.MzsReplayGatherArgs()
        a.struct_size = C.sizeof(_lib.MzsReplayGatherArgs)
        a.episodes, a.stream_rows, a.rows_padded = len(desc), int(stream_rows), int(rows_padded)
        a.desc, a.desc_host, a.obs = d.ptr, desc.ctypes.data, out.ptr
        rc = self._call(self.L.mzs_replay_gather_obs, (C.byref(self.arena), C.byref(a)), {}, [d, (out, True)])
        return rc, out.host().view(np.uint32)

    def reanalyse(self, desc, pi, v, n, gamma, alpha=None, weight_mode=1, stream_rows=None, rows_padded=None):
        """pi [rows, A], v [rows] float32 streams (rows >= rows_padded).  Returns the status."""
        desc = np.ascontiguousarray(desc, np.int32)
        g = dict(desc=Guarded.of(desc.reshape(-1)), pi=Guarded.of(pi, torch.float32), v=Guarded.of(v, torch.float32),
                 gpow=Guarded.of(np.array([float(gamma) ** i for i in range(int(n) + 1)], np.float64)))
        a = _lib.MzsReplayReanalyseArgs()
        a.struct_size = C.sizeof(_lib.MzsReplayReanalyseArgs)
        rows = len(g["v"].t)
        a.episodes = len(desc)
        a.stream_rows = rows if stream_rows is None else int(stream_rows)
        a.rows_padded = rows if rows_padded is None else int(rows_padded)
        a.desc, a.desc_host = g["desc"].ptr, desc.ctypes.data
        a.n_step, a.weight_mode = int(n), int(weight_mode)
        a.has_alpha, a.alpha = int(alpha is not None), float(alpha if alpha is not None else 0.0)
        a.gpow, a.pi, a.v = g["gpow"].ptr, g["pi"].ptr, g["v"].ptr
        covered, slots = self._covered(desc)
        may = {k: covered for k in ("pi", "v", "Rn", "done", "w", "cw")}
        may["t_w"] = slots
        return self._call(self.L.mzs_replay_reanalyse, (C.byref(self.arena), C.byref(a)), may, list(g.values()))
