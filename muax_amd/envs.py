"""Vector environments stepped on the device ("Device environments").

The device-environment protocol is duck-typed, as `add_steps` and `update_priorities` are.  An object implements it
when it has

    reset_device() -> obs                    float32 [N, obs_dim] device tensor
    step_device(a, r_out, done_out) -> obs   a: int32 [N] device tensor; r_out: float64 [N] and done_out: uint8 [N]
                                             device views the step writes; obs: the next observations, device tensor
    n, spec.max_episode_steps, device

(all three classes here, `DeviceCartPole`, `DeviceAcrobot` and `DeviceMountainCar`, also expose `obs_dim` and
`num_actions`) with the conventions of the host protocol (muax_amd/vector.py): `done` marks the LAST step of an episode
and the returned observation of a finished environment is already the first one of its next episode.  Neither call may
synchronise; both run on the current stream of `device`.  The returned tensor may be the environment's own and be
overwritten by its next call: `DeviceVectorCollector` stages it in its ring before it steps again.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np

from . import prng


class _DeviceEnv:
    """What the three environments share: the tensors of one descriptor of the C ABI and both protocols on its reset
    and step entries.  A subclass names its descriptor class `_DESC`, the two entries `_RESET` / `_STEP` and `_KIND`
    (all four by their names in `_lib`; `_KIND` None for a descriptor without one), `_ID`, `_STATE_DIM`, `obs_dim` and
    `num_actions`; `_HOST_HINT` is appended to the refusal of a device that is no GPU."""
    _DESC = _RESET = _STEP = _KIND = _ID = _STATE_DIM = obs_dim = num_actions = None
    _HOST_HINT = ""

    def __init__(self, n, max_episode_steps, seed=0, device=None):
        import torch

        from . import _lib
        name = type(self).__name__
        self.n = int(n)
        if self.n < 1 or int(max_episode_steps) < 1:
            raise ValueError(f"{name}: n and max_episode_steps must be at least 1")
        self.spec = SimpleNamespace(id=self._ID, max_episode_steps=int(max_episode_steps))
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"{name}: needs a GPU device{self._HOST_HINT}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._L = _lib.load()
        dev = self.device
        self._state = torch.zeros((self.n, self._STATE_DIM), dtype=torch.float64, device=dev)
        self._t = torch.zeros(self.n, dtype=torch.int32, device=dev)
        self._draws = torch.zeros(self.n, dtype=torch.int32, device=dev)
        self._obs = torch.zeros((self.n, self.obs_dim), dtype=torch.float32, device=dev)
        self._r = torch.zeros(self.n, dtype=torch.float64, device=dev)      # the host protocol's outputs
        self._done = torch.zeros(self.n, dtype=torch.uint8, device=dev)
        key = prng.PRNGKey(seed)
        kind = {} if self._KIND is None else {"kind": getattr(_lib, self._KIND)}
        self._env = _lib.args(getattr(_lib, self._DESC), device=dev.index, num_envs=self.n,
                              max_episode_steps=self.spec.max_episode_steps, key=(int(key[0]), int(key[1])),
                              state=self._state.data_ptr(), t=self._t.data_ptr(), draws=self._draws.data_ptr(), **kind)

    def _stream(self):
        import torch
        raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
        return C.c_void_p(raw(self.device.index) if raw is not None
                          else torch.cuda.current_stream(self.device).cuda_stream)

    def _view(self, x, dtype, name):
        if x.dtype != dtype or x.device != self.device or tuple(x.shape) != (self.n,) or not x.is_contiguous():
            raise ValueError(f"step_device: {name} must be a contiguous {dtype} [{self.n}] tensor on {self.device}")
        return x.data_ptr()

    # ---- the device protocol
    def reset_device(self):
        from . import _lib
        _lib.check(getattr(self._L, self._RESET)(C.byref(self._env), self._obs.data_ptr(), self._stream()))
        return self._obs

    def step_device(self, a, r_out, done_out):
        import torch

        from . import _lib
        s = _lib.args(_lib.MzsEnvStepArgs)  # (per step: fields by attribute, which is 1 us cheaper)
        s.a = self._view(a, torch.int32, "a")
        s.r_out, s.done_out = self._view(r_out, torch.float64, "r_out"), self._view(done_out, torch.uint8, "done_out")
        s.obs_out = self._obs.data_ptr()
        _lib.check(getattr(self._L, self._STEP)(C.byref(self._env), C.byref(s), self._stream()))
        return self._obs

    # ---- the host protocol
    def reset(self):
        return self.reset_device().cpu().numpy()

    def step(self, actions):
        import torch
        a = torch.from_numpy(np.ascontiguousarray(np.asarray(actions).reshape(-1), dtype=np.int32)).to(self.device)
        obs = self.step_device(a, self._r, self._done)
        return obs.cpu().numpy(), self._r.cpu().numpy(), self._done.cpu().numpy().astype(bool)


class DeviceCartPole(_DeviceEnv):
    """`examples/cartpole_env.VectorCartPole` on the device: N cart-poles, one launch per step
    (`mzs_env_cartpole_step`: the same fp64 arithmetic in the same order, the device's sin / cos), auto-reset inside
    that launch.  The start states are NOT NumPy's: environment e's d-th draw of component c is
    `-0.05 + 0.1 * u53(PRNGKey(seed), e, 4 d + c)`, the replay sampler's threefry uniform, so the state stream is a
    function of the seed and the actions alone.  Also offers the host protocol (`reset()` / `step(actions)` return NumPy
    copies, each a synchronisation), so it can be handed to `test_vector`; which of the two is called does not change
    the stream."""
    _DESC, _RESET, _STEP = "MzsEnvCartPole", "mzs_env_cartpole_reset", "mzs_env_cartpole_step"
    _ID, _STATE_DIM, obs_dim, num_actions = "CartPole-v1", 4, 4, 2
    _HOST_HINT = " (use examples/cartpole_env.VectorCartPole on the host)"

    def __init__(self, n, max_episode_steps=500, seed=0, device=None):
        super().__init__(n, max_episode_steps, seed, device)


class DeviceAcrobot(_DeviceEnv):
    """N Acrobots (Gym's Acrobot-v1: Sutton & Barto's "book" equations, one Runge-Kutta step of 0.2 s per action) on the
    device, one launch per step (`mzs_env_classic_step`), auto-reset inside that launch.  Three actions (torque -1, 0,
    +1), observations (cos th1, sin th1, cos th2, sin th2, dth1, dth2), reward -1 per step and 0 on the step that
    swings the tip above the bar.  Start states: environment e's d-th draw of component c is
    `-0.1 + 0.2 * u53(PRNGKey(seed), e, 4 d + c)`.  Both protocols, as `DeviceCartPole`."""
    _DESC, _RESET, _STEP = "MzsEnvClassic", "mzs_env_classic_reset", "mzs_env_classic_step"
    _KIND, _ID, _STATE_DIM, obs_dim, num_actions = "MZS_ENV_ACROBOT", "Acrobot-v1", 4, 6, 3

    def __init__(self, n, max_episode_steps=500, seed=0, device=None):
        super().__init__(n, max_episode_steps, seed, device)


class DeviceMountainCar(_DeviceEnv):
    """N mountain cars (Gym's MountainCar-v0 in fp64) on the device, one launch per step (`mzs_env_classic_step`),
    auto-reset inside that launch.  Three actions (push left, none, right), observations (x, v), reward -1 per step;
    an episode ends at x >= 0.5 with v >= 0.  Start states: environment e's d-th draw is
    x = `-0.6 + 0.2 * u53(PRNGKey(seed), e, d)`, v = 0.  Both protocols, as `DeviceCartPole`."""
    _DESC, _RESET, _STEP = "MzsEnvClassic", "mzs_env_classic_reset", "mzs_env_classic_step"
    _KIND, _ID, _STATE_DIM, obs_dim, num_actions = "MZS_ENV_MOUNTAINCAR", "MountainCar-v0", 2, 2, 3

    def __init__(self, n, max_episode_steps=200, seed=0, device=None):
        super().__init__(n, max_episode_steps, seed, device)
