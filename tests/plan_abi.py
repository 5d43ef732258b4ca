"""mzs_replay_plan_steps called directly through muax_amd._lib, for test_gpu_plan_kernels.py: no collector, no buffer.

Every buffer the call sees -- the ring's five fields, the flags, open_len, open_ret, ep, ret, counts, scratch -- is a
`Guarded` view of tests/replay_abi.py: a pattern-filled tensor with 64 guard elements on each side.  After each call
every guard must be the pattern, the ring and the flags must be bit-identical, and so must every row of `ep` / `ret`
at or beyond min(counts[0], max_out); open_len, open_ret and counts are the call's to write, the inside of scratch is
its own.  A call that is refused must have changed nothing at all."""
import ctypes as C

import numpy as np
import torch

from muax_amd import _lib
from replay_abi import GUARD, Guarded

RING = {"obs": torch.float32, "a": torch.int32, "r": torch.float64, "v": torch.float32, "pi": torch.float32}


class Plan:
    """A guarded ring of `S` rows x `N` environments (obs_dim = num_actions = 1), its flags, and the plan's buffers
    with `out_rows` rows of ep / ret."""

    def __init__(self, S, N, out_rows):
        self.S, self.N, self.out_rows = int(S), int(N), int(out_rows)
        self.L = _lib.load()
        self.f = {n: Guarded(self.S * self.N, 1, dt) for n, dt in RING.items()}
        self.f["done"] = Guarded(self.S * self.N, 1, torch.uint8)
        self.f["open_len"] = Guarded(self.N, 1, torch.int32)
        self.f["open_ret"] = Guarded(self.N, 1, torch.float64)
        self.f["ep"] = Guarded(self.out_rows, 4, torch.int32, flat=False)
        self.f["ret"] = Guarded(self.out_rows, 1, torch.float64)
        self.f["counts"] = Guarded(4, 1, torch.int32)
        self.f["scratch"] = Guarded(_lib.replay_plan_scratch(self.N), 1, torch.int32)
        ring = _lib.MzsReplayRing()
        ring.struct_size = C.sizeof(_lib.MzsReplayRing)
        ring.device = torch.cuda.current_device()
        ring.ring_steps, ring.num_envs, ring.obs_dim, ring.num_actions = self.S, self.N, 1, 1
        for n in RING:
            setattr(ring, n, self.f[n].ptr)
        self.ring = ring

    def put(self, name, array):
        g = self.f[name]
        g.t.copy_(torch.as_tensor(np.ascontiguousarray(array)).to(g.dtype).reshape(g.t.shape))

    def host(self, name):
        return self.f[name].host()

    def args(self, row0, steps, min_length, max_out=None):
        a = _lib.MzsReplayPlanArgs()
        a.struct_size = C.sizeof(_lib.MzsReplayPlanArgs)
        a.row0, a.steps, a.min_length = int(row0), int(steps), int(min_length)
        a.max_out = self.out_rows if max_out is None else int(max_out)
        for n in ("done", "open_len", "open_ret", "ep", "ret", "counts", "scratch"):
            setattr(a, n, self.f[n].ptr)
        return a

    def call(self, a, ring=None):
        """Run the entry point with arguments `a` (None: a null pointer) and `ring` (default the rig's; False: a null
        pointer); returns the status after the checks of the module docstring."""
        torch.cuda.synchronize()
        before = {n: g.bits.clone() for n, g in self.f.items()}
        rc = self.L.mzs_replay_plan_steps(None if ring is False else C.byref(self.ring if ring is None else ring),
                                          None if a is None else C.byref(a),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        free = {"open_len", "open_ret", "counts", "scratch"} if rc == _lib.MZS_OK else set()
        written = min(int(self.host("counts")[0]), int(a.max_out)) if rc == _lib.MZS_OK else 0
        for n, g in self.f.items():
            assert g.guards_intact(), f"a guard of {n} was overwritten"
            if n in free:
                continue
            same = g.bits == before[n]
            if n in ("ep", "ret"):
                same |= g.row_mask(np.arange(g.rows) < written)
            assert bool(same.all()), f"{n} changed outside the rows the call may write " \
                                     f"(first at element {int((~same).nonzero()[0]) - GUARD} of the view)"
        return rc
