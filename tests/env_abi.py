"""The device-environment entry points of the C ABI (mzs_env_cartpole_* and mzs_env_classic_*; muax_amd/csrc/mz_env.cuh)
called directly through muax_amd._lib: no DeviceCartPole / DeviceAcrobot / DeviceMountainCar.  For test_gpu_env.py and
test_gpu_env_classic.py.

Every tensor a kernel sees lies between guards (tests/replay_abi.Guarded).  `r_out` and `done_out` are the MIDDLE row of
a [3, N] array, so a wrong row stride shows.  After each call everything outside state, t, draws, obs_out, r_out[0:N]
and done_out[0:N] must be bit-identical to what it was; a call that is refused must have changed nothing at all."""
import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch

from muax_amd import _lib, prng
from replay_abi import Guarded

MIDDLE = np.array([False, True, False])


class EnvAbi(NamedTuple):
    """What tells one environment's entries from another's: the descriptor class, the two entry names, the widths of
    state and observation, and the descriptor's `kind` (None: it has none)."""
    descriptor: type
    reset: str
    step: str
    state_dim: int
    obs_dim: int
    kind: Optional[int] = None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


class Env:
    """Guarded buffers of one environment descriptor (`abi`: an EnvAbi) and the two calls."""

    def __init__(self, abi, N, max_steps, seed, state=None, t=None, draws=None):
        self.abi, self.N, self.max_steps, self.key = abi, int(N), int(max_steps), prng.PRNGKey(seed)
        z, S = np.zeros, abi.state_dim
        self.g = dict(state=Guarded.of(z((N, S)) if state is None else np.asarray(state, np.float64).reshape(N, S)),
                      t=Guarded.of(np.asarray(z(N) if t is None else t, np.int32)),
                      draws=Guarded.of(np.asarray(z(N) if draws is None else draws, np.int32)),
                      obs=Guarded(N, abi.obs_dim, torch.float32, flat=False), a=Guarded(N, 1, torch.int32),
                      r=Guarded(3, N, torch.float64, flat=False), done=Guarded(3, N, torch.uint8, flat=False))
        self.L = _lib.load()
        self.env = self.descriptor()

    def descriptor(self, **over):
        d = self.abi.descriptor()
        d.struct_size = C.sizeof(self.abi.descriptor)
        d.device, d.num_envs, d.max_episode_steps = torch.cuda.current_device(), self.N, self.max_steps
        if self.abi.kind is not None:
            d.kind = self.abi.kind
        d.key[0], d.key[1] = int(self.key[0]), int(self.key[1])
        d.state, d.t, d.draws = self.g["state"].ptr, self.g["t"].ptr, self.g["draws"].ptr
        for k, v in over.items():
            setattr(d, k, v)
        return d

    def step_args(self, **over):
        s = _lib.MzsEnvStepArgs()
        s.struct_size = C.sizeof(_lib.MzsEnvStepArgs)
        s.a, s.obs_out = self.g["a"].ptr, self.g["obs"].ptr
        s.r_out, s.done_out = self.g["r"].t[1].data_ptr(), self.g["done"].t[1].data_ptr()
        for k, v in over.items():
            setattr(s, k, v)
        return s

    def _call(self, fn, args, writes):
        """`writes`: the buffers the call may write (r and done: their middle row only)."""
        torch.cuda.synchronize()
        before = {n: g.bits.clone() for n, g in self.g.items()}
        rc = fn(*args, _stream())
        torch.cuda.synchronize()
        for n, g in self.g.items():
            assert g.guards_intact(), f"{fn.__name__}: a guard of {n} was overwritten"
            same = g.bits == before[n]
            if rc == _lib.MZS_OK and n in writes:
                same |= g.row_mask(MIDDLE if n in ("r", "done") else np.ones(g.rows, bool))
            assert bool(same.all()), f"{fn.__name__}: {n} changed where it must not"
        return rc

    def reset(self, env=None, obs="own"):
        obs = self.g["obs"].ptr if obs == "own" else obs
        return self._call(getattr(self.L, self.abi.reset), (C.byref(env or self.env), C.c_void_p(obs)),
                          ("state", "t", "draws", "obs"))

    def step(self, a=None, env=None, args=None):
        if a is not None:
            self.g["a"].t.copy_(torch.as_tensor(np.asarray(a, np.int32)))
        return self._call(getattr(self.L, self.abi.step), (C.byref(env or self.env), C.byref(args or self.step_args())),
                          ("state", "t", "draws", "obs", "r", "done"))

    def host(self):
        """(state f64, t, draws, obs f32, r [N], done [N]) as the device holds them."""
        g = self.g
        return (g["state"].host(), g["t"].host(), g["draws"].host(), g["obs"].host(), g["r"].host()[1],
                g["done"].host()[1])
