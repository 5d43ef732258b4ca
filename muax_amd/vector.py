"""Vectorised tracer + collector: the data plumbing that feeds the batched act().

The reference traces one environment with a Python deque per step (`muax/episode_tracer.py:118-249`,
driven from `muax/train.py:150-173`).  With thousands of roots searched per launch that bookkeeping is the
bottleneck, so here the n-step returns and priority weights of whole episodes are computed as array
operations, and a vector environment is stepped with ONE batched act() per step.  Values are those of
`NStep` / `PNStep` (tests/test_fit_cpu.py compares them transition by transition).  Host-side NumPy:
no arithmetic of the hot path lives here.

Vector-environment protocol (that of `rollout_batched`): `reset() -> obs [N, ...]`,
`step(actions [N]) -> (obs [N, ...], reward [N], done [N])`, where `done` marks the LAST step of an
episode (terminated or truncated) and the returned observation of a finished environment is already the
first observation of its next episode (auto-reset).
"""
from __future__ import annotations

import ctypes as C
import inspect
import time
from typing import Callable, NamedTuple, Optional

import numpy as np
import torch

from . import _lib, prng  # (_lib.load() is lazy: importing this module needs no built library)
from . import utils as mx_utils
from .replay_buffer import Trajectory, TrajectoryReplayBuffer
from .train import _temperature_fn, test


# ---- Capabilities.  What an environment or a buffer may offer beyond the protocol above, each asked in one place. ----
def _is_device_env(venv):
    """The device-environment protocol of muax_amd/envs.py: `reset_device` / `step_device` on device tensors."""
    return hasattr(venv, "step_device")


def _is_gym_env(env):
    """A gym-style single environment (`observation_space`, the five-tuple `step`): what `train.test` evaluates."""
    return hasattr(env, "observation_space")


def _device_mask_of(venv):
    """The mask extension of muax_amd/envs.py on the device: act()'s `invalid_actions` keyword with the environment's
    own uint8 [N, A] tensor (`invalid_actions_device()`, overwritten in place by its launches), or nothing."""
    return {"invalid_actions": venv.invalid_actions_device()} if hasattr(venv, "invalid_actions_device") else {}


def _has_host_mask(venv):
    """The same extension through the host protocol: `invalid_actions()` -> uint8 [N, A] as NumPy, asked every step."""
    return hasattr(venv, "invalid_actions")


def _mask_fn_of(venv):
    """The same extension for stored observations: reanalyse's `mask_fn` keyword (`invalid_actions_of`), or nothing."""
    return {"mask_fn": venv.invalid_actions_of} if hasattr(venv, "invalid_actions_of") else {}


def _has_device_store(buffer):
    """`add_steps` of muax_amd/replay_device.py: episodes cut out of a collection ring on the device."""
    return hasattr(buffer, "add_steps")


def _offers(buffer, method):
    """An optional method of muax_amd/replay_device.py that the host buffer lacks: `add_many` (a collection in one
    launch), `reanalyse` (with `stalest`), `update_priorities`."""
    return hasattr(buffer, method)


def _sample_takes(buffer):
    """The parameters of the buffer's `sample`: `is_beta` and `all_obs` are replay_device.py's, the host buffer has
    neither."""
    return inspect.signature(buffer.sample).parameters


def nstep_returns(r, v, n: int, gamma: float):
    """`NStep` over one COMPLETE episode at once (muax/episode_tracer.py:161-195).
    r, v: [T].  Returns (Rn [T] float64, done [T] bool): Rn[t] = sum_{i<n, t+i<T} gamma^i r[t+i]
    + gamma^n v[t+n] when step t+n exists; `done` marks the transitions that could not bootstrap."""
    r = np.asarray(r, np.float64).reshape(-1)
    v = np.asarray(v, np.float64).reshape(-1)
    T = r.shape[0]
    rp = np.concatenate([r, np.zeros(n)])
    Rn = np.zeros(T)
    for i in range(n):  # n is ~10: a loop over the horizon, vectorised over the episode
        Rn += (gamma ** i) * rp[i:i + T]
    boot = np.arange(T) + n < T
    vb = np.concatenate([v, np.zeros(n)])[n:n + T]
    Rn = Rn + np.where(boot, vb * (gamma ** n), 0.0)
    return Rn, ~boot


def episode_trajectory(obs, a, r, v, pi, n: int, gamma: float, alpha=None) -> Trajectory:
    """One finished episode (arrays [T, ...]) -> an array-backed Trajectory with the fields `NStep`
    (alpha None: w = 1) or `PNStep` (w = |v - Rn| ** alpha, muax/episode_tracer.py:198-249) would emit."""
    Rn, done = nstep_returns(r, v, n, gamma)
    v64 = np.asarray(v, np.float64).reshape(-1)
    w = np.ones_like(Rn) if alpha is None else np.abs(v64 - Rn) ** alpha
    pi = np.asarray(pi)
    if pi.ndim == 2:  # the reference keeps act()'s [1, A] row per step (muax/model.py:176, train.py:164)
        pi = pi[:, None, :]
    return Trajectory.from_arrays(np.asarray(obs), np.asarray(a).astype(np.int64), np.asarray(r, np.float64), done,
                                  Rn, v64, pi, w)


class VectorCollector:
    """Steps a vector environment with one batched act() per step and cuts the stream into episodes.
    Unfinished episodes are carried into the next `collect` call, so every trajectory handed out is a
    complete episode, exactly what the per-environment tracers of `fit` produce."""

    def __init__(self, venv, n: int, gamma: float, alpha=0.5):
        self.venv, self.n, self.gamma, self.alpha = venv, int(n), float(gamma), alpha
        self._obs = None
        self._pending = None  # per environment: (obs, a, r, v, pi) of the episode still open, or None

    def collect(self, model, key, steps: int, num_simulations: int = 50, temperature: float = 1.0, **act_kwargs):
        """`steps` lock-step environment steps.  Returns (finished trajectories, advanced key, env steps)."""
        if self._obs is None:
            self._obs = np.asarray(self.venv.reset())
            self._pending = [None] * self._obs.shape[0]
        N = self._obs.shape[0]
        obs_l, a_l, r_l, d_l, v_l, pi_l = [], [], [], [], [], []
        obs = self._obs
        for _ in range(steps):
            key, subkey = prng.split(key)
            a, pi, v = model.act(subkey, obs, with_pi=True, with_value=True, obs_from_batch=True,
                                 num_simulations=num_simulations, temperature=temperature, **act_kwargs)
            nxt, r, done = self.venv.step(a)
            obs_l.append(obs), a_l.append(np.asarray(a)), r_l.append(np.asarray(r, np.float64))
            d_l.append(np.asarray(done, bool)), v_l.append(np.asarray(v, np.float64)), pi_l.append(np.asarray(pi))
            obs = np.asarray(nxt)
        self._obs = obs
        fields = [np.stack(x) for x in (obs_l, a_l, r_l, v_l, pi_l)]  # [T, N, ...]
        (O, A, R, V, P), first, carried = self._flat_streams(fields, steps)
        ends, env_of_end, last_end, left = self._episode_ends(np.stack(d_l), first, carried, steps)
        Rn, nb, W = self._returns_and_priorities(R, V, left)
        if P.ndim == 2:
            P = P[:, None, :]
        streams = (O, A.astype(np.int64), R, nb, Rn, V, P, W)
        return self._cut_and_carry(streams, first, ends, env_of_end, last_end), key, steps * N

    def _flat_streams(self, fields, steps):
        """Env-major flat streams: for every environment its carried-over open episode, then the call's steps.
        Returns (the streams of `fields`, the stream offset of every environment [N + 1], the carried steps [N])."""
        N = len(self._pending)
        carried = np.array([0 if p is None else len(p[0]) for p in self._pending])
        flat = []
        for k, f in enumerate(fields):
            f = np.swapaxes(f, 0, 1)  # [N, T, ...]
            if carried.any():
                f = np.concatenate([x for e in range(N) for x in
                                    ((self._pending[e][k], f[e]) if carried[e] else (f[e],))])
            else:
                f = f.reshape((N * steps,) + f.shape[2:])
            flat.append(f)
        return flat, np.concatenate([[0], np.cumsum(carried + steps)]), carried

    @staticmethod
    def _episode_ends(D, first, carried, steps):
        """From the call's flags D [T, N]: the stream positions that end an episode, the environment of each, every
        environment's last one (-1: none; the stream up to it is closed, the rest is carried over), and `left`, the
        steps from every position to the end of its episode, that one included (garbage on open tails)."""
        N, M = len(carried), first[-1]
        done = np.zeros(M, bool)  # carried steps are never episode ends
        done[(first[:-1] + carried)[:, None] + np.arange(steps)[None, :]] = D.T
        ends = np.flatnonzero(done)
        last_end = np.full(N, -1)
        env_of_end = np.searchsorted(first, ends, side="right") - 1
        last_end[env_of_end] = ends  # ends ascend, so the last one per environment stays
        pos = np.arange(M)
        nxt = ends[np.minimum(np.searchsorted(ends, pos), max(len(ends) - 1, 0))] if len(ends) else pos
        return ends, env_of_end, last_end, nxt - pos + 1

    def _returns_and_priorities(self, R, V, left):
        """`nstep_returns` and the priority weights over the whole flat stream at once, `left` keeping every sum inside
        its episode.  (`nstep_returns` states the same arithmetic for ONE episode -- `episode_trajectory`, the tests and
        the reference comparison use it; calling it per episode here would be a Python loop over the thousands of
        episodes a wide collection finishes.)  Returns (Rn, the flags of the transitions that could not bootstrap, w)."""
        n, g, M = self.n, self.gamma, len(R)
        Rp, Vp = np.concatenate([R, np.zeros(n)]), np.concatenate([V, np.zeros(n)])
        Rn = np.zeros(M)
        for i in range(n):
            Rn += np.where(i < left, (g ** i) * Rp[i:i + M], 0.0)
        boot = left > n
        Rn = Rn + np.where(boot, Vp[n:n + M] * (g ** n), 0.0)
        W = np.ones(M) if self.alpha is None else np.abs(V - Rn) ** self.alpha
        return Rn, ~boot, W

    def _cut_and_carry(self, streams, first, ends, env_of_end, last_end):
        """Cut the closed part of the streams (obs, a, r, done, Rn, v, pi, w) into one Trajectory per episode and keep
        every environment's open tail for the next call."""
        O, A, R, nb, Rn, V, P, W = streams
        starts = np.concatenate([[0], ends[:-1] + 1]) if len(ends) else np.zeros(0, int)
        starts = np.maximum(starts, first[env_of_end]) if len(ends) else starts
        out = []
        for s0, e0 in zip(starts.tolist(), (ends + 1).tolist()):
            out.append(Trajectory.from_arrays(O[s0:e0], A[s0:e0], R[s0:e0], nb[s0:e0], Rn[s0:e0], V[s0:e0],
                                              P[s0:e0], W[s0:e0], _checked=True))
        for e in range(len(self._pending)):
            s0 = first[e] if last_end[e] < 0 else last_end[e] + 1
            e0 = first[e + 1]
            self._pending[e] = (O[s0:e0], A[s0:e0], R[s0:e0], V[s0:e0], P[s0:e0, 0]) if s0 < e0 else None
        return out


def ring_plan(done, open_start, step0, min_length=1):
    """The episodes a call of lock-step collection finishes, from its `done` flags alone (host arithmetic, no GPU).
    done [T, N]: the flags of the call's T steps; open_start [N]: the ABSOLUTE step at which every environment's open
    episode began; step0: the absolute index of the call's first step.  Returns (finished, dropped, new open_start):
    the finished episodes of at least `min_length` steps as (environment, first absolute step, length) in the order in
    which `VectorCollector.collect` hands out its trajectories (environment-major, then time), those shorter than
    `min_length` in the same form and order, and the start of every environment's episode still open afterwards."""
    D = np.asarray(done, bool)
    if D.ndim != 2:
        raise ValueError("ring_plan: done must be [T, N]")
    open_start = np.asarray(open_start, np.int64).reshape(-1)
    if open_start.shape[0] != D.shape[1]:
        raise ValueError("ring_plan: one open_start per environment")
    env, t = np.nonzero(D.T)  # environment-major, time ascending
    end = int(step0) + t.astype(np.int64)
    same = np.concatenate([[False], env[1:] == env[:-1]])
    first = np.where(same, np.concatenate([[0], end[:-1] + 1]), open_start[env])
    length = end - first + 1
    new_open = open_start.copy()
    new_open[env] = end + 1  # ends ascend inside an environment, so its last one stays
    rows = list(zip(env.tolist(), first.tolist(), length.tolist()))
    m = int(min_length)
    return [x for x in rows if x[2] >= m], [x for x in rows if x[2] < m], new_open


class DeviceVectorCollector:
    """`VectorCollector` for a `DeviceReplayBuffer`, with the search results kept on the device: every step's
    observations, actions, root values and search policies are staged in a step-major ring of `ring_steps` x N rows
    (one launch per step, `mzs_replay_stage`), only the ACTIONS come to the host (for `venv.step`), and at the end of
    `collect()` the rewards go up (at most two copies) and the finished episodes are cut out of the ring into the
    buffer's arenas in one launch (`DeviceReplayBuffer.add_steps`), which computes the n-step returns, `done`, the
    priority weights and the episode weight (`weight`: "mean" or "sum") as `add_raw` does, bit for bit.  Episodes
    shorter than `min_length` are dropped and get no serial.  The key stream is `VectorCollector.collect`'s, and so are
    the order of the episodes and therefore their serials.  `ring_steps` defaults to `venv.spec.max_episode_steps` plus
    the steps of the first `collect` call: an open episode must fit the ring together with the call's steps.
    How the strided reads of the store launch compare with `add_raw`'s dense ones has not been measured.
    A `venv` with `step_device` (the device-environment protocol of muax_amd/envs.py, e.g. `DeviceCartPole`) is stepped
    on the device: its observation tensor goes into act() and the staging launch as it is, `step_device` writes the
    step's rewards straight into the ring's `r` row and its `done` flags into the same row of a uint8
    [ring_steps, N] tensor, nothing inside the step loop copies to the host or synchronises, and per `collect()` the
    call's `r` and `done` rows come down once (at most two copies each) for `ring_plan` and the returns; there is no
    reward upload.  A host `venv` takes the path it always took.
    `device_plan=True` (a `venv` with `step_device`; any other is a ValueError) also cuts the episodes and sums their
    returns on the device (`mzs_replay_plan_steps`, two launches after the step loop): the [T, N] rewards and flags stay
    where they are, no per-environment state is kept on the host, and per `collect()` three small copies come down --
    the counts (the call's first synchronisation), then one (environment, first ring row, length, stored) row and one
    return per finished episode.  The episodes, their order, their serials and what the buffer stores are the default
    route's.  An episode's return on this route is the SEQUENTIAL fp64 sum of its rewards in time order, not
    `np.sum`'s pairwise sum; for rewards that are small integers (every environment of the project) the two are equal
    bit for bit, for other rewards they may differ in the last bits."""

    store_s = 0.0  # (fit_vector's `collect_s`: storing is part of this collection, nothing is taken out of its time)

    def __init__(self, venv, buffer, n: int, gamma: float, alpha=0.5, weight: str = "mean", min_length: int = 1,
                 ring_steps=None, device_plan: bool = False):
        if not _has_device_store(buffer):
            raise ValueError(f"DeviceVectorCollector needs a buffer with the device store (DeviceReplayBuffer); "
                             f"{type(buffer).__name__} has none")
        if weight not in ("mean", "sum"):
            raise ValueError("weight must be 'mean' or 'sum'")
        if int(n) < 1:
            raise ValueError("n must be at least 1")
        if ring_steps is not None and int(ring_steps) < 1:
            raise ValueError("ring_steps must be positive")
        if device_plan and not _is_device_env(venv):
            raise ValueError(f"DeviceVectorCollector: device_plan needs a device environment (one with step_device, "
                             f"e.g. DeviceCartPole): the plan kernel reads the rewards and flags the environment wrote "
                             f"on the device; {type(venv).__name__} has no step_device")
        if device_plan and int(min_length) < 1:
            raise ValueError("DeviceVectorCollector: device_plan needs min_length >= 1")
        self.venv, self.buffer, self.n, self.gamma, self.alpha = venv, buffer, int(n), float(gamma), alpha
        self.weight, self.min_length = weight, int(min_length)
        self.ring_steps = None if ring_steps is None else int(ring_steps)
        self._obs = self._ring = self._fields = self._done_rows = None
        self._step0 = 0          # absolute index of the next step
        self._open_start = None  # [N] absolute first step of every open episode
        self._open_r = None      # per environment: the host rewards of its open episode so far
        self.device_plan = bool(device_plan)
        self._plan = None        # device_plan: the plan kernel's device tensors, allocated once
        self._plan_held = 0      # device_plan: the longest open episode after the previous call (counts[2])

    def _alloc(self, N, obs_dim, A):
        buf = self.buffer
        buf._check_dims(obs_dim, A)  # (allocates the arenas on first use; a mismatch is the buffer's ValueError)
        dev, S = buf._device, self.ring_steps
        shapes = {"obs": ((S, N, obs_dim), torch.float32), "a": ((S, N), torch.int32), "r": ((S, N), torch.float64),
                  "v": ((S, N), torch.float32), "pi": ((S, N, A), torch.float32)}
        self._fields = {k: torch.zeros(shape, dtype=dt, device=dev) for k, (shape, dt) in shapes.items()}
        self._ring = _lib.args(_lib.MzsReplayRing, device=buf._arena.device, ring_steps=S, num_envs=N, obs_dim=obs_dim,
                               num_actions=A, **{k: x.data_ptr() for k, x in self._fields.items()})
        if _is_device_env(self.venv):  # the flags a device environment writes, beside the ring fields
            self._done_rows = torch.zeros((S, N), dtype=torch.uint8, device=dev)

    def _stage(self, i, obs_d, a, pi, v):
        """One `mzs_replay_stage`: step i of the call into its ring row.  Returns the actions as int32 on the device."""
        N = self._ring.num_envs
        flat = obs_d.reshape(N, -1).contiguous()
        a32 = a.to(torch.int32).contiguous()
        pi32, v32 = pi.to(torch.float32).reshape(N, -1).contiguous(), v.to(torch.float32).reshape(N).contiguous()
        s = _lib.args(_lib.MzsReplayStageArgs)  # (per step: fields by attribute, which is 1 us cheaper)
        s.row = (self._step0 + i) % self.ring_steps
        s.obs, s.a, s.v, s.pi = flat.data_ptr(), a32.data_ptr(), v32.data_ptr(), pi32.data_ptr()
        _lib.check(self.buffer._L.mzs_replay_stage(C.byref(self._ring), C.byref(s), self.buffer._stream()))
        return a32

    def _spans(self, steps):
        """The ring rows of the call's `steps` steps as [(lo, hi)]: one span, two where they wrap past the ring's end."""
        row0 = self._step0 % self.ring_steps
        k = min(steps, self.ring_steps - row0)
        return [(row0, row0 + k)] + ([(0, steps - k)] if k < steps else [])

    def _steps(self, model, key, steps, num_simulations, temperature, act_kwargs):
        """The step loop of every route: act() on device tensors, the staging launch, then the environment.  A host
        environment gets the actions (the one device-to-host copy of the step) and returns NumPy; its rewards go up
        into the ring's `r` rows after the loop.  A device environment (muax_amd/envs.py) keeps the observations on the
        device and writes every step's rewards into the ring's `r` row and its flags into the same row of
        `self._done_rows` (uint8 [ring_steps, N]); nothing in its loop copies to the host or synchronises, and all
        launches go on the one stream the staging launch uses, which orders the environment's overwrite of its
        observation tensor after the staging launch that read it.  Afterwards the call's rows of `r` and of the flags
        come down, in at most two copies each.  Returns (key, R [T, N] float64, D [T, N] bool); under `device_plan`
        nothing comes down and R, D are None.
        A device environment with `invalid_actions_device` (the mask extension of muax_amd/envs.py, e.g. `Device2048`;
        looked for once per call) has that tensor passed to every act() as `invalid_actions`: the environment's own
        uint8 [N, A] mask of the observation act() is given, the same object every step.  The same stream order holds
        for it: the environment's overwrite of the mask comes after the search that read it.  An environment without
        the method gets exactly the act() calls it always got."""
        venv, S = self.venv, self.ring_steps
        on_device = _is_device_env(venv)
        if on_device:
            act_kwargs = {**_device_mask_of(venv), **act_kwargs}  # (a caller's own wins)
        dev, first = self.buffer._device, self._obs is None
        if first:
            if on_device and dev is not None and dev.index is not None and torch.device(venv.device) != dev:
                raise ValueError(f"collect: the environment is on {venv.device}, the buffer on {dev}")
            self._obs = venv.reset_device() if on_device else np.asarray(venv.reset())
        obs = self._obs
        N = int(venv.n) if on_device else obs.shape[0]
        if first and not self.device_plan:
            self._open_start, self._open_r = np.zeros(N, np.int64), [[] for _ in range(N)]
        if dev is None and not on_device:
            dev = model.device
        r_l, d_l = [], []
        for i in range(steps):
            key, subkey = prng.split(key)
            obs_d = obs if on_device else torch.from_numpy(np.ascontiguousarray(obs, dtype=np.float32)).to(dev)
            a, pi, v = model.act(subkey, obs_d, with_pi=True, with_value=True, obs_from_batch=True, device_outputs=True,
                                 num_simulations=num_simulations, temperature=temperature, **act_kwargs)
            if self._ring is None:
                self._alloc(N, int(obs_d.numel() // N), int(pi.shape[-1]))
            a32 = self._stage(i, obs_d, a, pi, v)
            if on_device:
                row = (self._step0 + i) % S
                obs = venv.step_device(a32, self._fields["r"][row], self._done_rows[row])
            else:
                nxt, r, done = venv.step(a32.cpu().numpy())  # the one device-to-host copy of the step
                r_l.append(np.asarray(r, np.float64)), d_l.append(np.asarray(done, bool))
                obs = np.asarray(nxt)
        self._obs = obs
        if self.device_plan:
            return key, None, None
        spans = self._spans(steps)
        if on_device:
            R = np.concatenate([self._fields["r"][lo:hi].cpu().numpy() for lo, hi in spans])
            D = np.concatenate([self._done_rows[lo:hi].cpu().numpy() for lo, hi in spans]).astype(bool)
        else:
            R, D, at = np.stack(r_l), np.stack(d_l), 0  # [T, N]
            for lo, hi in spans:
                self._fields["r"][lo:hi].copy_(torch.from_numpy(R[at:at + hi - lo]))
                at += hi - lo
        return key, R, D

    def _plan_on_host(self, R, D, step0):
        """The call's episodes from its flags (`ring_plan`) and their returns from the host's rewards R [T, N]: the
        carried part of an episode, then the call's.  Returns ([(environment, first ring row, length, stored)], returns)
        and moves `_open_start` / `_open_r` on."""
        finished, dropped, new_open = ring_plan(D, self._open_start, step0, self.min_length)
        Rt = np.ascontiguousarray(R.T)
        stored = set(finished)
        every = sorted(finished + dropped, key=lambda x: (x[0], x[1])) if dropped else finished
        G = []
        for env, first, T in every:
            seg = Rt[env, max(first - step0, 0):first + T - step0]
            G.append(float(np.sum(np.concatenate(self._open_r[env] + [seg]) if first < step0 else seg)))
        for env in range(R.shape[1]):
            if new_open[env] <= step0:  # no episode of this environment ended: the open one grows
                self._open_r[env].append(Rt[env].copy())
            else:
                tail = Rt[env, new_open[env] - step0:]
                self._open_r[env] = [tail.copy()] if len(tail) else []
        self._open_start = new_open
        return [(env, first % self.ring_steps, T, (env, first, T) in stored) for env, first, T in every], G

    def _plan_on_device(self, steps):
        """`mzs_replay_plan_steps` on the call's rows, then the counts (the call's first synchronisation) and one
        episode row and one return per finished episode come down.  Returns what `_plan_on_host` returns and moves
        `_plan_held` on (the launch itself has advanced the device's open_len / open_ret)."""
        N, S = int(self._ring.num_envs), self.ring_steps
        dev = self._fields["r"].device
        if self._plan is None:
            self._plan = {"open_len": torch.zeros(N, dtype=torch.int32, device=dev),
                          "open_ret": torch.zeros(N, dtype=torch.float64, device=dev),
                          "counts": torch.zeros(4, dtype=torch.int32, device=dev),
                          "scratch": torch.zeros(_lib.replay_plan_scratch(N), dtype=torch.int32, device=dev)}
        pl = self._plan
        if "ep" not in pl or pl["ep"].shape[0] < N * steps:  # N * steps episodes at the most; grows with `steps`
            pl["ep"] = torch.zeros((N * steps, 4), dtype=torch.int32, device=dev)
            pl["ret"] = torch.zeros(N * steps, dtype=torch.float64, device=dev)
        max_out = int(pl["ep"].shape[0])
        a = _lib.args(_lib.MzsReplayPlanArgs, row0=self._step0 % S, steps=steps, min_length=self.min_length,
                      max_out=max_out, done=self._done_rows.data_ptr(), **{k: x.data_ptr() for k, x in pl.items()})
        _lib.check(self.buffer._L.mzs_replay_plan_steps(C.byref(self._ring), C.byref(a), self.buffer._stream()))
        counts = pl["counts"].cpu().numpy()
        episodes = int(counts[0])
        if episodes > max_out:
            raise RuntimeError(f"collect: the plan reports {episodes} episodes, more than its {max_out} output rows")
        rows = pl["ep"][:episodes].cpu().numpy().tolist() if episodes else []
        G = pl["ret"][:episodes].cpu().numpy().tolist() if episodes else []
        self._plan_held = int(counts[2])
        return rows, G

    def collect(self, model, key, steps: int, num_simulations: int = 50, temperature: float = 1.0, **act_kwargs):
        """`steps` lock-step environment steps.  Returns (finished, advanced key, env steps): `finished` lists, in
        `VectorCollector.collect`'s order, (length, undiscounted return, serial) of every episode that ended, the
        return summed from the host's rewards (with `device_plan`: summed on the device, sequentially in time order)
        and the serial None for one dropped as shorter than `min_length`.
        ValueError before the first step when an open episode could outgrow the ring (its steps so far plus `steps`
        exceed `ring_steps`): nothing is overwritten and a call with fewer steps still works."""
        steps = int(steps)
        if steps < 1:
            raise ValueError("collect: steps must be at least 1")
        if self.ring_steps is None:
            self.ring_steps = int(self.venv.spec.max_episode_steps) + steps
        S = self.ring_steps
        if self.device_plan:
            held = self._plan_held
        else:
            held = 0 if self._open_start is None else self._step0 - int(self._open_start.min())
        if held + steps > S:
            raise ValueError(f"collect: an open episode of {held} steps plus {steps} more does not fit the ring of "
                             f"{S} steps (ring_steps)")
        if self.device_plan and int(self.venv.n) * steps >= 2 ** 31:
            raise ValueError("collect: device_plan needs num_envs * steps below 2^31")
        step0 = self._step0
        key, R, D = self._steps(model, key, steps, num_simulations, temperature, act_kwargs)
        rows, G = self._plan_on_device(steps) if self.device_plan else self._plan_on_host(R, D, step0)
        # the collector's state moves on before add_steps on both routes: if add_steps raises -- an episode longer than
        # the buffer's max_steps -- the call's episodes are lost, not collected twice
        self._step0 = step0 + steps
        serials = iter(self.buffer.add_steps(self._ring, [(env, first, T) for env, first, T, kept in rows if kept],
                                             self.n, self.gamma, self.alpha, weight=self.weight))
        out = [(T, g, next(serials) if kept else None) for (_, _, T, kept), g in zip(rows, G)]
        return out, key, steps * int(self._ring.num_envs)


def test_vector(model, venv, key, num_simulations: int, max_steps=None):
    """Greedy evaluation (muax/test.py:5-48: temperature 0, mean undiscounted return) on a vector
    environment: the FIRST episode of each of its N environments, one batched act() per step.  An environment with
    `invalid_actions()` (uint8 [N, A] as NumPy, 1 where the action is illegal for the observation last returned) has it
    passed to every act() as `invalid_actions`; any other is evaluated as before."""
    obs = np.asarray(venv.reset())
    N = obs.shape[0]
    G, live = np.zeros(N), np.ones(N, bool)
    steps = max_steps if max_steps is not None else venv.spec.max_episode_steps
    masked = _has_host_mask(venv)
    for _ in range(steps):
        key, subkey = prng.split(key)
        mask = {"invalid_actions": venv.invalid_actions()} if masked else {}
        a = model.act(subkey, obs, obs_from_batch=True, num_simulations=num_simulations, temperature=0., **mask)
        obs, r, done = venv.step(a)
        obs = np.asarray(obs)
        G += np.where(live, np.asarray(r, np.float64), 0.0)
        live &= ~np.asarray(done, bool)
        if not live.any():
            break
    return float(G.mean())


def test_vector_device(model, venv, key, num_simulations: int, max_steps=None):
    """`test_vector` on a device environment (muax_amd/envs.py) without leaving the device: `reset_device` /
    `step_device`, act() on the environment's observation tensor with device outputs, the returns `G` [N] and the mask
    of the environments still in their first episode kept as device tensors.  Nothing inside the loop copies to the
    host or synchronises except the "all finished" check, made after every 16th step only (the steps in between add
    0.0 to every return: the value does not depend on when the loop stops).  At the end `G` comes down once and its mean
    is taken on the host: the key stream, the fp64 additions and the mean are `test_vector`'s, so the value is
    `test_vector(model, venv, key, ...)`'s exactly.
    An environment with `invalid_actions_device` (looked for once per call) has that tensor -- its own mask of the
    observation act() is given, overwritten in place by its launches -- passed to every act() as `invalid_actions`;
    the stream orders the environment's overwrite after the search that read it.  Any other is evaluated as before."""
    if not _is_device_env(venv):
        raise ValueError(f"test_vector_device needs a device environment (one with step_device); "
                         f"{type(venv).__name__} has none: use test_vector")
    mask = _device_mask_of(venv)
    obs = venv.reset_device()
    N, dev = int(venv.n), obs.device
    G = torch.zeros(N, dtype=torch.float64, device=dev)
    live = torch.ones(N, dtype=torch.bool, device=dev)
    r = torch.zeros(N, dtype=torch.float64, device=dev)
    done = torch.zeros(N, dtype=torch.uint8, device=dev)
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    steps = max_steps if max_steps is not None else venv.spec.max_episode_steps
    for i in range(steps):
        key, subkey = prng.split(key)
        a = model.act(subkey, obs, obs_from_batch=True, device_outputs=True, num_simulations=num_simulations,
                      temperature=0., **mask)
        obs = venv.step_device(a.to(torch.int32).contiguous(), r, done)
        G += torch.where(live, r, zero)
        live &= done == 0
        if i % 16 == 15 and not bool(live.any()):  # (the loop's one synchronisation, every 16th step)
            break
    return float(G.cpu().numpy().mean())


def value_priorities(model, batch):
    """New priorities of a sampled batch from the CURRENT network: |value(repr(obs[:, 0])) - Rn[:, 0]| as [B] float32
    on the model's device -- the value error of every window's first transition, the one whose weight decided the
    draw of the start.  The model's torch modules under no_grad, the scalar value decoded from the support logits as
    in root inference; no synchronisation."""
    dev = model.device
    with torch.no_grad():
        obs = torch.as_tensor(batch.obs, dtype=torch.float32, device=dev)
        Rn = torch.as_tensor(batch.Rn, dtype=torch.float32, device=dev)
        v_logits, _ = model.pred_func(model.repr_func(obs[:, 0]))
        v = mx_utils.support_to_scalar(torch.softmax(v_logits, dim=-1), model._support_size).flatten()
        return (v - Rn.reshape(Rn.shape[0], -1)[:, 0]).abs()


def unroll_value_priorities(model, batch, k_prio=None, backend: str = "auto"):
    """The [B, kp] sibling of `value_priorities`: |v_i - Rn[:, i]| for the first `kp` steps of every window (default: all
    of them), v_i the value of the state the CURRENT network unrolls to along the window's actions --
    `MuZero.unroll_values(batch, k_prio, backend)[1]`: one kernel launch for the default MLP trio on a GPU, else the
    model's torch modules.  float32 on the model's device, no synchronisation."""
    return model.unroll_values(batch, k_prio=k_prio, backend=backend)[1]


class _HostCollect:
    """`VectorCollector` behind `DeviceVectorCollector.collect`'s result, for fit_vector: the finished episodes of at
    least `k_steps` steps go into the buffer -- `add_many` where it has one (the device buffer: one upload and one
    launch for the collection), else `add` per trajectory -- with the "mean" or "sum" of their priority weights, and
    every finished episode, kept or not, comes back as a (length, undiscounted return, None) row in the collector's
    order.  `store_s`: the seconds the last call spent after the collection itself, which `collect_s` leaves out."""

    def __init__(self, collector, buffer, k_steps, weight):
        self.collector, self.buffer, self.k_steps, self.weight = collector, buffer, k_steps, weight
        self.add_many = _offers(buffer, "add_many")
        self.store_s = 0.0

    def collect(self, model, key, steps, num_simulations, temperature):
        trajs, key, env_steps = self.collector.collect(model, key, steps, num_simulations, temperature)
        t0 = time.perf_counter()
        keep = [tr for tr in trajs if len(tr) >= self.k_steps]
        weights = [tr.weights.mean() if self.weight == "mean" else tr.weights.sum() for tr in keep]
        if self.add_many:
            self.buffer.add_many(keep, weights)
        else:
            for tr, w in zip(keep, weights):
                self.buffer.add(tr, w)
        rows = [(len(tr), float(np.sum(tr.rewards)), None) for tr in trajs]
        self.store_s = time.perf_counter() - t0
        return rows, key, env_steps


def _tester(test_env, num_simulations, num_test_episodes):
    """(model, key) -> mean greedy return on `test_env`: the reference's `test` for a gym-style environment, else all
    the vector environment's first episodes in lock step, where it lives.  The value is the same either way."""
    if _is_gym_env(test_env):
        return lambda model, key: test(model, test_env, key, num_simulations=num_simulations,
                                       num_test_episodes=num_test_episodes)
    if _is_device_env(test_env):
        return lambda model, key: test_vector_device(model, test_env, key, num_simulations)
    return lambda model, key: test_vector(model, test_env, key, num_simulations)


def _unpack_sample(got, with_indices, with_isw):
    """What `sample` returned -- a batch alone, or (batch[, indices][, isw]) -- as (batch, indices or None, update()'s
    keywords: the weights as `sample_weight`, or none)."""
    if not (with_indices or with_isw):
        return got, None, {}
    return got[0], got[1] if with_indices else None, {"sample_weight": got[-1]} if with_isw else {}


class _FitPlan(NamedTuple):
    """What fit_vector's loop runs with, settled by `_fit_plan` before anything else happens."""
    buffer: object
    collector: object              # .collect(model, key, steps, num_simulations, temperature) -> (rows, key, env steps)
    sample_kw: dict                # the keywords every sample() gets (is_beta, where scheduled, is added per batch)
    prioritise: bool               # sample with indices and write priorities back after every update
    priorities: Callable           # (model, batch) -> the priorities to write back
    beta: Optional[Callable]       # training_step -> is_beta of the next batch, or None: no importance weights
    reanalyse_kw: Optional[dict]   # reanalyse()'s fixed keywords, or None: never reanalyse
    tester: Callable               # (model, key) -> test_G


def _fit_plan(model, venv, test_env, buffer, *, n_step, gamma, alpha, num_simulations, k_steps, num_trajectory,
              sample_per_trajectory, max_training_steps, num_test_episodes, trajectory_weight, reanalyse_every,
              priority_update, priority_steps, is_beta, device_collect, device_plan, all_obs) -> _FitPlan:
    """Every check of fit_vector's arguments against each other, the buffer, the environments and the model, and what
    follows from them.  Touches neither the model nor an environment; the first refusal that applies is raised:
      1. priority_steps below 1
      2. trajectory_weight neither "mean" nor "sum"
      3. device_plan without device_collect and a device environment
         (from here on `buffer` is the default host buffer where none was given)
      4. is_beta with a buffer whose sample() takes none
      5. is_beta neither a callable nor within 0..1
      6. all_obs=True with a buffer whose sample() takes none
      7. priority_steps written back (priority_update, a buffer with update_priorities) for a stochastic model that
         does not unroll its SMZNetwork
      8. a device environment without device_collect
      9. device_collect with a buffer without the device store
     10. what `DeviceVectorCollector` itself refuses (n_step below 1; k_steps below 1 under device_plan)."""
    on_device = _is_device_env(venv)
    if priority_steps is not None and int(priority_steps) < 1:
        raise ValueError("priority_steps must be None or >= 1")
    if trajectory_weight not in ("mean", "sum"):
        raise ValueError("trajectory_weight must be 'mean' or 'sum'")
    if device_plan and not (device_collect and on_device):
        raise ValueError(f"fit_vector: device_plan needs device_collect=True and a device environment (one with "
                         f"step_device); device_collect is {bool(device_collect)} and {type(venv).__name__} has "
                         f"{'a' if on_device else 'no'} step_device")
    buffer = buffer if buffer is not None else TrajectoryReplayBuffer(500)
    takes = _sample_takes(buffer)
    if is_beta is not None:
        if "is_beta" not in takes:
            raise ValueError(f"fit_vector: is_beta needs a buffer whose sample() takes is_beta (DeviceReplayBuffer); "
                             f"{type(buffer).__name__}.sample does not")
        if not callable(is_beta) and not 0.0 <= float(is_beta) <= 1.0:
            raise ValueError("fit_vector: is_beta must be None, a number in 0..1 or a callable")
    stochastic = bool(getattr(model, "trains_stochastic", False))  # (update()'s own predicate for stochastic_loss_fn)
    if all_obs and "all_obs" not in takes:
        raise ValueError(f"fit_vector: all_obs needs a buffer whose sample() takes all_obs (DeviceReplayBuffer); "
                         f"{type(buffer).__name__}.sample does not")
    all_obs = (stochastic and "all_obs" in takes) if all_obs is None else bool(all_obs)
    prioritise = bool(priority_update) and _offers(buffer, "update_priorities")
    if prioritise and priority_steps is not None and stochastic and not getattr(model, "unrolls_stochastic", False):
        raise ValueError("fit_vector: priority_update with priority_steps needs MuZero.unroll_values, which is not built "
                         "for an SMZNetwork (a stochastic model); use priority_steps=None (value_priorities)")
    if on_device and not device_collect:
        raise ValueError(f"fit_vector: {type(venv).__name__} is a device environment (it has step_device) and needs "
                         f"device_collect=True; device_collect is False")
    if device_collect and not _has_device_store(buffer):
        if on_device:
            needs = (f"{type(venv).__name__} is a device environment (it has step_device) and needs a buffer with "
                     f"the device store, add_steps (DeviceReplayBuffer)")
        else:
            needs = "device_collect needs a buffer with the device store (DeviceReplayBuffer)"
        raise ValueError(f"fit_vector: {needs}; {type(buffer).__name__} has none")
    if device_collect:  # the episodes are in the buffer when its collect() returns
        collector = DeviceVectorCollector(venv, buffer, n_step, gamma, alpha, weight=trajectory_weight,
                                          min_length=k_steps, device_plan=device_plan)
    else:
        collector = _HostCollect(VectorCollector(venv, n_step, gamma, alpha), buffer, k_steps, trajectory_weight)

    sample_kw = dict(num_trajectory=num_trajectory, k_steps=k_steps, sample_per_trajectory=sample_per_trajectory)
    if prioritise:
        sample_kw["with_indices"] = True
    if all_obs:
        sample_kw["all_obs"] = True
    # (both priority functions are looked up in this module when they are called)
    if priority_steps is None:
        def priorities(model, batch):
            return value_priorities(model, batch)
    else:
        def priorities(model, batch):
            return unroll_value_priorities(model, batch, min(int(priority_steps), k_steps))
    if is_beta is None:
        beta = None
    elif callable(is_beta):
        def beta(training_step):
            return float(is_beta(training_steps=training_step, max_training_steps=max_training_steps))
    else:
        def beta(training_step):
            return float(is_beta)
    reanalyse_kw = None
    if reanalyse_every > 0 and _offers(buffer, "reanalyse"):
        reanalyse_kw = dict(weight=trajectory_weight, num_simulations=num_simulations, **_mask_fn_of(venv))
    return _FitPlan(buffer, collector, sample_kw, prioritise, priorities, beta, reanalyse_kw,
                    _tester(test_env, num_simulations, num_test_episodes))


def fit_vector(model, venv, test_env, n_step: int = 10, gamma: float = 0.997, alpha=0.5, buffer=None,
               iterations: int = 100, steps_per_iteration: int = 64, num_simulations: int = 50, k_steps: int = 10,
               num_trajectory: int = 32, sample_per_trajectory: int = 1, num_update_per_iteration: int = 50,
               max_training_steps: int = 10000, test_interval: int = 10, num_test_episodes: int = 10,
               random_seed: int = 42, temperature_fn=None, metrics=None, trajectory_weight: str = "mean",
               reanalyse_every: int = 0, reanalyse_episodes=None, priority_update: bool = False,
               priority_steps=None, is_beta=None, device_collect: bool = False, device_plan: bool = False,
               all_obs=None):
    """The reference's fit() loop (muax/train.py:175-241: temperature schedule, buffer sampling, update, greedy
    test) with the acting half on a vector environment.  Per iteration: `steps_per_iteration` batched act() calls, the
    finished episodes of at least `k_steps` steps into the buffer, an optional reanalysis, `num_update_per_iteration`
    times sample -> update() -> optional priority write-back, every `test_interval`-th iteration a greedy test, one
    metrics row; it stops after `iterations` or once `max_training_steps` updates are done.  All arguments are checked
    against each other, the buffer, the environments and the model before `model.init` (`_fit_plan` lists the order);
    what is refused is a ValueError.  Every option below at its default leaves the key stream and every result as they
    are without it.  Returns the model.

    venv: the vector environment that is collected from.  One with `step_device` (a device environment,
        muax_amd/envs.py) is stepped on the device by `DeviceVectorCollector`; it needs `device_collect=True` and a
        buffer with the device store and is refused otherwise: stepping it through host copies would hide the cost it
        exists to avoid.  One with the mask extension of envs.py (e.g. `Device2048`) has its own mask passed to every
        act() of the collection by that collector, and see `reanalyse_every`.
    test_env: a gym-style environment (one with `observation_space`) is evaluated by the reference's `test` with
        `num_test_episodes` episodes; a vector environment with `step_device` by `test_vector_device` (no host hop per
        step), any other by `test_vector`; the value of the two is the same.
    n_step, gamma, alpha: the n-step return and the priority exponent of `NStep` / `PNStep` (alpha None: weights 1).
    buffer: default `TrajectoryReplayBuffer(500)`.  A buffer with `add_many` (the device buffer) gets a collection in
        one call, any other one `add` per episode.
    temperature_fn: called as `temperature_fn(max_training_steps=, training_steps=)` before every iteration; default
        the reference's schedule.
    metrics: a list that gets one dict per iteration: iteration, env_steps, episodes (all that finished), collect_s
        (the collection alone, without the host route's buffer adds), G (the mean undiscounted return of all finished
        episodes, NaN when none finished), loss (when the buffer held something), training_step, test_G (when tested).
    trajectory_weight: "mean" is the reference's buffer weight (mean priority of the episode, muax/train.py:171,203);
        "sum" weights an episode by its total priority, which undoes the bias of a fixed collection window towards
        short episodes (many short episodes finish while one long one runs).  Anything else is refused.
    reanalyse_every: > 0 with a buffer with `reanalyse` (the device buffer): before the updates of every
        `reanalyse_every`-th iteration the `reanalyse_episodes` episodes (default: all) whose targets are the oldest are
        searched again with the current network (`DeviceReplayBuffer.reanalyse`, `num_simulations` simulations, act()'s
        other defaults), its key one extra split of the running key.  A `venv` with `invalid_actions_of` hands it over
        as `mask_fn`, so that no reanalysed search policy puts weight on a move that is illegal in its stored
        observation.  Ignored for a buffer without the method and while the buffer is empty.
    priority_update: with a buffer with `update_priorities` (the device buffer) every batch is sampled with its
        indices and, after its `update()`, new priorities from the updated network are written back to the window
        starts with the loop's `alpha` (exponent 1 when `alpha` is None) and `weight=trajectory_weight`.  Ignored for a
        buffer without the method.
    priority_steps: which priorities are written back.  None: `value_priorities` (one transition per window); an
        integer kp >= 1: `unroll_value_priorities(model, batch, min(kp, k_steps))`, one priority for each of the first
        kp transitions of every window.  Below 1 is refused.  Ignored where nothing is written back; where something
        is, a stochastic model (`MuZero.trains_stochastic`) is refused unless it unrolls its `SMZNetwork`
        (`MuZero(..., stochastic_unroll_values=True)`, `MuZero.unrolls_stochastic`: the afterstate and chance dynamics
        with the encoder's codes, from the observations `all_obs` hands out).
    is_beta: importance-sampling correction of the prioritised draws: a float in 0..1, or a schedule called as
        `is_beta(training_steps=, max_training_steps=)` before every batch (as `temperature_fn` is).  Every batch is
        sampled with `sample(is_beta=)` and its `update()` takes the returned weights as `sample_weight`; composes with
        `priority_update` / `priority_steps`.  The weights are normalised by the largest one of the batch, so under
        data parallelism by each rank's own batch maximum, not a global one.  A buffer whose `sample` takes no
        `is_beta` (the host `TrajectoryReplayBuffer`) is refused: dropping a correction that was asked for would change
        what is learned.  A number outside 0..1 is refused.
    device_collect: True collects with `DeviceVectorCollector` (`min_length=k_steps`, `weight=trajectory_weight`): the
        search results stay on the device and the episodes are cut into the buffer in one launch; `episodes` and `G`
        come from the host's rewards.  The same key stream and the same episodes as the host collector.  Needs a buffer
        with the device store (`DeviceReplayBuffer`); any other is refused.
    device_plan: True hands the flag to that collector: the episodes are cut and their returns summed on the device,
        `G` is then the mean of sequential fp64 sums -- equal to the host's for integer rewards.  Needs
        `device_collect=True` and a device environment; refused otherwise.
    all_obs: whether every batch is sampled with `sample(all_obs=True)`, an observation for every step of a window
        (`DeviceReplayBuffer.sample`).  None asks for them exactly when `update()` trains with
        `loss.stochastic_loss_fn` (a model on an `SMZNetwork`, `MuZero.trains_stochastic`) and the buffer's `sample`
        takes `all_obs`; the host `TrajectoryReplayBuffer` returns every row anyway and is left alone; for any other
        model None changes nothing.  True / False force it; True with a buffer whose `sample` takes no `all_obs` is
        refused.  So a stochastic model trains through this loop on a `DeviceReplayBuffer` and a device environment,
        with `reanalyse_every`, `priority_update` and `is_beta` as for the deterministic model."""
    plan = _fit_plan(model, venv, test_env, buffer, n_step=n_step, gamma=gamma, alpha=alpha,
                     num_simulations=num_simulations, k_steps=k_steps, num_trajectory=num_trajectory,
                     sample_per_trajectory=sample_per_trajectory, max_training_steps=max_training_steps,
                     num_test_episodes=num_test_episodes, trajectory_weight=trajectory_weight,
                     reanalyse_every=reanalyse_every, priority_update=priority_update, priority_steps=priority_steps,
                     is_beta=is_beta, device_collect=device_collect, device_plan=device_plan, all_obs=all_obs)
    buffer, collector = plan.buffer, plan.collector
    temperature_fn = temperature_fn or _temperature_fn
    key = prng.PRNGKey(random_seed)
    key, test_key, subkey = prng.split(key, 3)
    model.init(subkey, np.asarray(venv.reset())[:1].astype(float))
    training_step = 0
    for it in range(iterations):
        temperature = temperature_fn(max_training_steps=max_training_steps, training_steps=training_step)
        t0 = time.perf_counter()
        finished, key, env_steps = collector.collect(model, key, steps_per_iteration, num_simulations, temperature)
        row = {"iteration": it, "env_steps": env_steps, "episodes": len(finished),
               "collect_s": time.perf_counter() - t0 - collector.store_s,
               "G": float(np.mean([g for _, g, _ in finished])) if finished else float("nan")}
        if plan.reanalyse_kw is not None and len(buffer) and (it + 1) % reanalyse_every == 0:
            key, subkey = prng.split(key)
            buffer.reanalyse(model, subkey, n_step, gamma, alpha,
                             serials=buffer.stalest(reanalyse_episodes or len(buffer)), **plan.reanalyse_kw)
        if len(buffer):
            loss = 0.0
            for _ in range(num_update_per_iteration):
                sample_kw = plan.sample_kw if plan.beta is None else dict(plan.sample_kw, is_beta=plan.beta(training_step))
                batch, indices, update_kw = _unpack_sample(buffer.sample(**sample_kw), plan.prioritise,
                                                           plan.beta is not None)
                loss += model.update(batch, **update_kw)["loss"]
                if plan.prioritise:
                    buffer.update_priorities(indices, plan.priorities(model, batch),
                                             alpha=1.0 if alpha is None else alpha, weight=trajectory_weight)
                training_step += 1
            row["loss"] = loss / num_update_per_iteration
        row["training_step"] = training_step
        if it % test_interval == 0:
            row["test_G"] = plan.tester(model, test_key)
        if metrics is not None:
            metrics.append(row)
        if training_step >= max_training_steps:
            break
    return model
