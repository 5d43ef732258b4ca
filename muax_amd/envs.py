"""Vector environments stepped on the device ("Device environments").

The device-environment protocol is duck-typed, as `add_steps` and `update_priorities` are.  An object implements it
when it has

    reset_device() -> obs                    float32 [N, obs_dim] device tensor
    step_device(a, r_out, done_out) -> obs   a: int32 [N] device tensor; r_out: float64 [N] and done_out: uint8 [N]
                                             device views the step writes; obs: the next observations, device tensor
    n, spec.max_episode_steps, device

(all four classes here, `DeviceCartPole`, `DeviceAcrobot`, `DeviceMountainCar` and `Device2048`, also expose `obs_dim`
and `num_actions`) with the conventions of the host protocol (muax_amd/vector.py): `done` marks the LAST step of an episode
and the returned observation of a finished environment is already the first one of its next episode.  Neither call may
synchronise; both run on the current stream of `device`.  The returned tensor may be the environment's own and be
overwritten by its next call: `DeviceVectorCollector` stages it in its ring before it steps again.

Legal-move masks are an OPTIONAL extension of the protocol (`Device2048` has it, the three control tasks do not):

    invalid_actions_device() -> mask         uint8 [N, num_actions] device tensor, 1 where the action is illegal for the
                                             observation the last reset_device / step_device returned.  The environment's
                                             OWN tensor, the same object every call: its launches overwrite it in place,
                                             so act()'s argument cache keeps hitting
    invalid_actions_of(obs) -> mask          uint8 [B, num_actions] device tensor for observations [B, obs_dim] (a new
                                             tensor): what reanalysis of stored observations needs

`DeviceVectorCollector` and `test_vector_device` pass `invalid_actions=venv.invalid_actions_device()` to every act()
when the first exists, `fit_vector` hands `mask_fn=venv.invalid_actions_of` to `DeviceReplayBuffer.reanalyse` when the
second does.  An environment with neither is stepped exactly as before: the same launches, the same key stream.  The host
protocol's sibling is `invalid_actions()`, a NumPy copy, which `test_vector` uses when it is there.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib, prng
from ._call import device_index, raw_stream


class _DeviceEnv:
    """What the three environments share: the tensors of one descriptor of the C ABI and both protocols on its reset
    and step entries.  A subclass names its descriptor class `_DESC`, the two entries `_RESET` / `_STEP` and `_KIND`
    (all four by their names in `_lib`; `_KIND` None for a descriptor without one), `_ID`, `_STATE_DIM`, `obs_dim` and
    `num_actions`; `_HOST_HINT` is appended to the refusal of a device that is no GPU."""
    _DESC = _RESET = _STEP = _KIND = _ID = _STATE_DIM = obs_dim = num_actions = None
    _HOST_HINT = ""

    def __init__(self, n, max_episode_steps, seed=0, device=None):
        dev = self._open(n, max_episode_steps, device)
        self._state = torch.zeros((self.n, self._STATE_DIM), dtype=torch.float64, device=dev)
        key = prng.PRNGKey(seed)
        kind = {} if self._KIND is None else {"kind": getattr(_lib, self._KIND)}
        self._env = _lib.args(getattr(_lib, self._DESC), device=dev.index, num_envs=self.n,
                              max_episode_steps=self.spec.max_episode_steps, key=(int(key[0]), int(key[1])),
                              state=self._state.data_ptr(), t=self._t.data_ptr(), draws=self._draws.data_ptr(), **kind)

    def _open(self, n, max_episode_steps, device):
        """The checks and tensors of every descriptor: n, spec, device, the library, t, draws, obs and the host
        protocol's outputs.  Returns the device."""
        name = type(self).__name__
        self.n = int(n)
        if self.n < 1 or int(max_episode_steps) < 1:
            raise ValueError(f"{name}: n and max_episode_steps must be at least 1")
        self.spec = SimpleNamespace(id=self._ID, max_episode_steps=int(max_episode_steps))
        self.device = torch.device("cuda" if device is None else device)
        if self.device.type != "cuda":
            raise ValueError(f"{name}: needs a GPU device{self._HOST_HINT}")
        self.device = torch.device("cuda", device_index(self.device))
        self._L = _lib.load()
        dev = self.device
        self._t = torch.zeros(self.n, dtype=torch.int32, device=dev)
        self._draws = torch.zeros(self.n, dtype=torch.int32, device=dev)
        self._obs = torch.zeros((self.n, self.obs_dim), dtype=torch.float32, device=dev)
        self._r = torch.zeros(self.n, dtype=torch.float64, device=dev)      # the host protocol's outputs
        self._done = torch.zeros(self.n, dtype=torch.uint8, device=dev)
        return dev

    def _stream(self):
        return raw_stream(self.device.index)

    def _view(self, x, dtype, name):
        if x.dtype != dtype or x.device != self.device or tuple(x.shape) != (self.n,) or not x.is_contiguous():
            raise ValueError(f"step_device: {name} must be a contiguous {dtype} [{self.n}] tensor on {self.device}")
        return x.data_ptr()

    # ---- the device protocol
    def reset_device(self):
        _lib.check(getattr(self._L, self._RESET)(C.byref(self._env), self._obs.data_ptr(), self._stream()))
        return self._obs

    def step_device(self, a, r_out, done_out):
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


class Device2048(_DeviceEnv):
    """N games of 2048 on the device, one launch per step (`mzs_env_2048_step`: integer arithmetic on one uint64 board
    per game, include/mzsearch.h has the rules), auto-reset inside that launch, and the legal-move mask of every
    returned observation.  Four actions (0 up, 1 right, 2 down, 3 left), observations [N, 16] = exponent / 16, reward =
    the sum of the tiles a move's merges created times 2^-`reward_shift` (0..11; exact in fp64, partial sums included).
    A move that leaves the board unchanged is illegal and a no-op: reward 0, no spawn, no draw consumed, `t` advances.
    An episode ends when no move changes the board.  Spawn d of environment e takes `threefry2x32(PRNGKey(seed), (e, d))`:
    cell number `(x0 * n_empty) >> 32` of the empty ones, a 4 where `x1 < 0x1999999A`, else a 2; the stream is a
    function of the seed and the actions alone.  Both protocols, as `DeviceCartPole`, and the mask extension of both
    (module docstring): `invalid_actions_device()`, `invalid_actions_of(obs)`, `invalid_actions()`."""
    _DESC, _RESET, _STEP = "MzsEnv2048", "mzs_env_2048_reset", "mzs_env_2048_step"
    _ID, obs_dim, num_actions = "2048", 16, 4

    def __init__(self, n, max_episode_steps=2000, seed=0, reward_shift=0, device=None):
        self.reward_shift = int(reward_shift)
        if not 0 <= self.reward_shift <= 11:
            raise ValueError("Device2048: reward_shift must be in 0..11")
        dev = self._open(n, max_episode_steps, device)
        self._board = torch.zeros(self.n, dtype=torch.int64, device=dev)  # (the 64 bits of the ABI's uint64)
        self._invalid = torch.zeros((self.n, self.num_actions), dtype=torch.uint8, device=dev)
        key = prng.PRNGKey(seed)
        self._env = _lib.args(_lib.MzsEnv2048, device=dev.index, num_envs=self.n,
                              max_episode_steps=self.spec.max_episode_steps, key=(int(key[0]), int(key[1])),
                              reward_shift=self.reward_shift, board=self._board.data_ptr(), t=self._t.data_ptr(),
                              draws=self._draws.data_ptr(), invalid=self._invalid.data_ptr())

    # ---- the mask extension of the device protocol
    def invalid_actions_device(self):
        """uint8 [N, 4], 1 where the move is illegal for the observation the last reset / step returned: the
        environment's own tensor, the same object every call, overwritten in place by the reset and step launches."""
        return self._invalid

    def invalid_actions_of(self, obs):
        """The mask of observations [B, 16] (a float32 device tensor, e.g. stored ones) as a new uint8 [B, 4] device
        tensor: one launch of `mzs_env_2048_mask` on the current stream, no synchronisation.  An all-zero row (the
        padding of a reanalysis chunk) reports every move as legal."""
        if not isinstance(obs, torch.Tensor) or obs.device != self.device or obs.dtype != torch.float32 \
                or obs.ndim != 2 or obs.shape[1] != self.obs_dim or obs.shape[0] < 1:
            raise ValueError(f"invalid_actions_of: obs must be a float32 [B >= 1, {self.obs_dim}] tensor on {self.device}")
        obs = obs.contiguous()
        out = torch.empty((obs.shape[0], self.num_actions), dtype=torch.uint8, device=self.device)
        _lib.check(self._L.mzs_env_2048_mask(self.device.index, obs.data_ptr(), out.data_ptr(), int(obs.shape[0]),
                                             self._stream()))
        return out

    # ---- ... and of the host protocol
    def invalid_actions(self):
        """`invalid_actions_device()` as a NumPy copy (a synchronisation)."""
        return self._invalid.cpu().numpy()
