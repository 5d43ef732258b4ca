"""Device-resident trajectory replay: `TrajectoryReplayBuffer`'s interface (muax/replay_buffer.py:161-262) with the
storage on the GPU and `sample()` as ONE launch that leaves a `Transition` of device tensors in the layout
`MuZero.update(backend="hip")` reads in place (kernels: muax_amd/csrc/mz_replay.cuh; the arithmetic
spec, the arena and the eviction rule: DESIGN.md 4.7).

The Python here keeps the bookkeeping -- where an episode goes, which ones are evicted, the running key -- and never
reads the device: `sample()` makes no device-to-host copy and no synchronisation, so it can be captured in a graph.
There is no CPU fallback: without a GPU the first add raises."""
from __future__ import annotations

import ctypes as C
import math
import os
from collections import deque, namedtuple

import numpy as np
import torch

from . import _lib, prng
from ._call import device_index, raw_stream
from .episode_tracer import Transition
from .replay_buffer import BaseReplayBuffer

_Episode = namedtuple("_Episode", "slot start length serial")
_ARENA_FIELDS = (("obs", torch.float32), ("a", torch.int32), ("r", torch.float32), ("Rn", torch.float32),
                 ("v", torch.float32), ("done", torch.uint8), ("pi", torch.float32), ("w", torch.float64),
                 ("cw", torch.float64))
_TABLE_FIELDS = (("t_start", torch.int32), ("t_len", torch.int32), ("t_w", torch.float64), ("t_serial", torch.int64),
                 ("c_start", torch.int32), ("c_len", torch.int32), ("c_CW", torch.float64), ("c_serial", torch.int64))
_WEIGHT_MODES = {"mean": 1, "sum": 2}
ReanalysePlan = namedtuple("ReanalysePlan", "offsets stream_rows n_chunks rows_padded")


def reanalyse_plan(lengths, chunk_rows):
    """Where the episodes of a reanalysis lie in its dense stream: `offsets` (the first row of every episode, the
    episodes back to back in the order given), `stream_rows` = sum(lengths), `n_chunks` = ceil(stream_rows /
    chunk_rows) searches of exactly `chunk_rows` roots, and `rows_padded` = n_chunks * chunk_rows."""
    lengths = [int(x) for x in lengths]
    chunk_rows = int(chunk_rows)
    if not lengths or min(lengths) <= 0:
        raise ValueError("reanalyse_plan: episode lengths must be positive")
    if chunk_rows <= 0:
        raise ValueError("reanalyse_plan: chunk_rows must be positive")
    offsets, rows = [], 0
    for T in lengths:
        offsets.append(rows)
        rows += T
    n_chunks = -(-rows // chunk_rows)
    return ReanalysePlan(offsets, rows, n_chunks, n_chunks * chunk_rows)


def _columns(trajectory):
    """(obs [T, obs_dim] f32, a [T] i32, r, Rn, v [T] f32, done [T] u8, pi [T, A] f32, w [T] f64) of a Trajectory,
    array-backed or filled step by step."""
    if getattr(trajectory, "_rows", None) is not None:
        cols = trajectory._rows
    else:
        if trajectory.batched_transitions is None:
            trajectory.finalize()
        cols = [np.asarray(x)[0] for x in trajectory.batched_transitions]
    obs, a, r, done, Rn, v, pi, w = (np.asarray(x) for x in cols)
    T = len(trajectory)
    if T == 0:
        raise ValueError("an empty trajectory cannot be stored")

    def col(x, dt):
        x = x.reshape(T, -1)[:, 0] if x.ndim else np.full(T, x)
        return np.ascontiguousarray(x, dtype=dt)
    return (np.ascontiguousarray(obs.reshape(T, -1), dtype=np.float32), col(a, np.int32), col(r, np.float32),
            col(Rn, np.float32), col(v, np.float32), col(done, np.uint8),
            np.ascontiguousarray(pi.reshape(T, -1), dtype=np.float32), col(w, np.float64))


def _gpow(gamma, n):
    """The discount powers gamma ** 0 .. gamma ** n the n-step kernels read."""
    return np.array([float(gamma) ** i for i in range(int(n) + 1)], np.float64)


def _check_nstep(who, n, weight):
    if weight not in _WEIGHT_MODES:
        raise ValueError("weight must be 'mean' or 'sum'")
    if int(n) < 1:
        raise ValueError(f"{who}: n must be at least 1")


def _nstep_fields(n, weight_mode, alpha):
    """The n-step fields the store, store_steps and reanalyse argument structs share."""
    return dict(n_step=int(n), weight_mode=weight_mode, has_alpha=int(alpha is not None),
                alpha=float(alpha if alpha is not None else 0.0))


class DeviceReplayBuffer(BaseReplayBuffer):
    """Ring buffer of whole episodes on the GPU.

    `capacity` episodes at most, `max_steps` transitions at most: every field has an arena of `max_steps` rows in
    which an episode is one contiguous range (never split across the wrap).  A new episode evicts the oldest ones
    while the episode count would exceed `capacity` or the arena has no contiguous room for it; one longer than
    `max_steps` is a ValueError.  `obs_dim` / `num_actions` default to those of the first episode added.

    `sample()` differs from the host buffer in two documented ways: the batch size is FIXED (episodes no longer than
    `k_steps` carry no probability instead of shortening the batch), and the random stream is a threefry key
    (`random_seed`, split on every call, or `key=`) instead of Python's `random`.  `obs` comes out as [B, 1, obs_dim],
    the window's first observation -- all the deterministic losses read -- or, with `sample(all_obs=True)`, as
    [B, k_steps, obs_dim], every step's, which the stochastic loss needs."""

    def __init__(self, capacity, max_steps, obs_dim=None, num_actions=None, random_seed=None, device=None,
                 transition_class=Transition):
        self._capacity, self._max_steps = int(capacity), int(max_steps)
        if self._capacity <= 0 or not 0 < self._max_steps < 2 ** 31:
            raise ValueError("capacity and max_steps must be positive (max_steps below 2^31)")
        self.obs_dim = None if obs_dim is None else int(obs_dim)
        self.num_actions = None if num_actions is None else int(num_actions)
        self.transition_class = transition_class
        self._device = None if device is None else torch.device(device)
        seed = int.from_bytes(os.urandom(4), "little") if random_seed is None else random_seed
        self._key = prng.PRNGKey(seed)
        self._arena = self._t = self._prio_scratch = self._is_scratch = None
        self._serial = 0
        self.clear()

    # ------------------------------------------------------------------ bookkeeping (host)
    @property
    def capacity(self):
        return self._capacity

    @property
    def max_steps(self):
        return self._max_steps

    @property
    def steps(self):
        """Transitions held."""
        return self._steps

    @property
    def serials(self):
        """Serial numbers of the episodes held, oldest first."""
        return [e.serial for e in self._eps]

    def eligible_windows(self, k_steps):
        """Number of windows of `k_steps` transitions `sample()` can draw: the sum of length - k_steps over the held
        episodes longer than k_steps (the N of the importance-sampling weights).  Host bookkeeping."""
        k = int(k_steps)
        return sum(e.length - k for e in self._eps if e.length > k)

    def episode(self, serial):
        """The stored episode with that serial as a Transition of views [T, ...] into the arenas (w: float64)."""
        for e in self._eps:
            if e.serial == serial:
                rows = slice(e.start, e.start + e.length)
                return self.transition_class(**{n: self._t[n][rows] for n in ("obs", "a", "r", "done", "Rn", "v", "pi", "w")})
        raise KeyError(f"no episode with serial {serial} in the buffer")

    def clear(self):
        self._eps = deque()
        self._touched, self._clock = {}, 0  # serial -> count of the add / reanalysis that last wrote its targets
        self._head = self._tail = self._steps = 0
        self._dirty, self._table_k, self._eligible, self._windows = True, None, False, 0

    def __len__(self):
        return len(self._eps)

    def __bool__(self):
        return bool(self._eps)

    def _evict(self):
        e = self._eps.popleft()
        self._touched.pop(e.serial, None)
        self._steps -= e.length
        self._head = (self._head + 1) % self._capacity

    def _place_all(self, lengths):
        """[(first transition in the stream, _Episode)] for consecutive episodes of a stream."""
        for T in lengths:
            if T > self._max_steps:
                raise ValueError(f"an episode of {T} steps does not fit max_steps = {self._max_steps}")
        placed, src = [], 0
        for T in lengths:
            placed.append((src, self._place(T)))
            src += T
        return placed

    def _place(self, T):
        """Make room for an episode of T transitions and enter it."""
        while len(self._eps) >= self._capacity:
            self._evict()
        while True:
            if not self._eps:
                dst = 0
                break
            lo = self._eps[0].start
            if lo < self._tail:  # the episodes are one stretch [lo, tail): room after it, or before it from row 0
                if self._tail + T <= self._max_steps:
                    dst = self._tail
                    break
                if T <= lo:
                    dst = 0
                    break
            elif self._tail + T <= lo:  # wrapped: [lo, end) and [0, tail), room in between
                dst = self._tail
                break
            self._evict()
        slot = (self._head + len(self._eps)) % self._capacity
        self._eps.append(_Episode(slot, dst, T, self._serial))
        self._clock += 1
        self._touched[self._serial] = self._clock
        self._serial += 1
        self._tail = dst + T
        self._steps += T
        self._dirty = True
        return self._eps[-1]

    # ------------------------------------------------------------------ device side
    def _alloc(self, obs_dim, num_actions):
        if not torch.cuda.is_available():
            raise RuntimeError("muax_amd needs a ROCm GPU (gfx950); there is no CPU fallback")
        if self._device is None:
            self._device = torch.device("cuda", torch.cuda.current_device())
        self.obs_dim = int(obs_dim) if self.obs_dim is None else self.obs_dim
        self.num_actions = int(num_actions) if self.num_actions is None else self.num_actions
        self._L = _lib.load()
        dev, S = self._device, self._max_steps
        shapes = {"obs": (S, self.obs_dim), "pi": (S, self.num_actions)}
        self._t = {n: torch.zeros(shapes.get(n, (S,)), dtype=dt, device=dev) for n, dt in _ARENA_FIELDS}
        self._t.update({n: torch.zeros(self._capacity, dtype=dt, device=dev) for n, dt in _TABLE_FIELDS})
        self._arena = _lib.args(_lib.MzsReplayArena, max_steps=S, capacity=self._capacity, obs_dim=self.obs_dim,
                                num_actions=self.num_actions, **{n: x.data_ptr() for n, x in self._t.items()},
                                device=device_index(dev))

    def _stream(self):
        return raw_stream(self._arena.device)

    def _check_dims(self, obs_dim, num_actions):
        if self._arena is None:
            self._alloc(obs_dim, num_actions)
        if obs_dim != self.obs_dim or num_actions != self.num_actions:
            raise ValueError(f"episode has obs_dim {obs_dim}, {num_actions} actions; the buffer holds "
                             f"obs_dim {self.obs_dim}, {self.num_actions} actions")

    def _upload(self, **host):
        """Small host arrays in ONE staging tensor and one copy: the widest element type first, every block starting
        on a multiple of 16 bytes.  Returns (the device tensor, {name: device pointer})."""
        names = sorted(host, key=lambda k: -host[k].dtype.itemsize)
        offs, total = {}, 0
        for k in names:
            offs[k] = total
            total += -(-host[k].nbytes // 16) * 16
        stage = np.empty(total, np.uint8)
        for k in names:
            stage[offs[k]:offs[k] + host[k].nbytes] = host[k].reshape(-1).view(np.uint8)
        dstage = torch.from_numpy(stage).to(self._device)
        return dstage, {k: dstage.data_ptr() + offs[k] for k in names}

    def _store(self, placed, host, device, raw=False, n=0, alpha=None, weight_mode=0, stream_steps=0):
        """One upload (the arrays of `host`, by name, in one staging buffer) and one launch.  `placed`:
        [(first transition in the stream, _Episode)] of the episodes that are still held; `device`: fields that
        already are device tensors."""
        live = {e.serial for e in self._eps}
        placed = [(src, e) for src, e in placed if e.serial in live]
        if not placed:
            return
        desc = np.array([[src, e.start, e.length, e.slot] for src, e in placed], np.int32)
        dstage, ptrs = self._upload(**host, serial=np.array([e.serial for _, e in placed], np.int64), desc=desc)
        a = _lib.args(_lib.MzsReplayStoreArgs, episodes=len(placed), stream_steps=stream_steps, raw=int(raw),
                      desc_host=desc.ctypes.data, **_nstep_fields(n, weight_mode, alpha), **ptrs,
                      **{k: x.data_ptr() for k, x in device.items()})
        _lib.check(self._L.mzs_replay_store(C.byref(self._arena), C.byref(a), self._stream()))
        self._keep = (dstage, device)

    def add(self, trajectory, w=1.):
        """Store one finished episode (a `Trajectory`, array-backed or filled step by step) with the buffer weight `w`."""
        self.add_many([trajectory], [w])

    def add_many(self, trajectories, weights):
        """`add` for a whole collection with one upload and one launch."""
        cols = [_columns(t) for t in trajectories]
        weights = [float(np.asarray(w).reshape(-1)[0]) for w in weights]
        if len(cols) != len(weights):
            raise ValueError("add_many: one weight per trajectory")
        if not cols:
            return
        for c in cols:
            self._check_dims(c[0].shape[1], c[6].shape[1])
        placed = self._place_all([len(c[0]) for c in cols])
        live = {e.serial for e in self._eps}
        keep = [i for i, (_, e) in enumerate(placed) if e.serial in live]
        # the stream holds the surviving episodes only (a collection larger than the buffer evicts its own head)
        src, kept = 0, []
        for i in keep:
            kept.append((src, placed[i][1]))
            src += placed[i][1].length
        host = {k: np.concatenate([cols[i][j] for i in keep])
                for j, k in enumerate(("obs", "a", "r", "Rn", "v", "done", "pi", "w"))}
        host["ep_w"] = np.array([weights[i] for i in keep], np.float64)
        self._store(kept, host, {}, stream_steps=src)

    def add_raw(self, obs, a, r, v, pi, lengths, n, gamma, alpha=None, weight="mean"):
        """Complete episodes as one flat stream (NumPy arrays or device tensors, [M, ...] with M = sum(lengths)):
        the n-step returns, `done` and the priority weights of `vector.nstep_returns` / `episode_trajectory`
        (w = |v - Rn| ** alpha, 1 when alpha is None) are computed on the device in fp64, in NumPy's operation
        order; the buffer weight of an episode is the `weight` ("mean" or "sum") of its transition weights."""
        _check_nstep("add_raw", n, weight)
        lengths = [int(x) for x in np.asarray(lengths).reshape(-1)]
        M = sum(lengths)
        if not lengths or min(lengths) <= 0:
            raise ValueError("add_raw: episode lengths must be positive")
        host, device = {}, {}
        for k, x, np_dt, t_dt in (("obs", obs, np.float32, torch.float32), ("a", a, np.int32, torch.int32),
                                  ("r", r, np.float64, torch.float64), ("v", v, np.float64, torch.float64),
                                  ("pi", pi, np.float32, torch.float32)):
            if len(x) != M:
                raise ValueError(f"add_raw: {k} has {len(x)} rows, the lengths sum to {M}")
            if isinstance(x, torch.Tensor):
                if self._device is None:
                    self._device = x.device
                device[k] = x.to(device=self._device, dtype=t_dt).reshape(M, -1).contiguous()
            else:
                host[k] = np.ascontiguousarray(np.asarray(x).reshape(M, -1), dtype=np_dt)
        dims = {**host, **device}
        if dims["a"].shape[1] != 1 or dims["r"].shape[1] != 1 or dims["v"].shape[1] != 1:
            raise ValueError("add_raw: a, r and v are one scalar per transition")
        self._check_dims(dims["obs"].shape[1], dims["pi"].shape[1])
        placed = self._place_all(lengths)
        host["gpow"] = _gpow(gamma, n)
        self._store(placed, host, device, raw=True, n=n, alpha=alpha, weight_mode=_WEIGHT_MODES[weight], stream_steps=M)

    def add_steps(self, ring, episodes, n, gamma, alpha=None, weight="mean"):
        """Complete episodes straight from a step-major collection ring on the device (`DeviceVectorCollector`'s;
        `ring` is its `_lib.MzsReplayRing`): `episodes` is [(environment, first ring row, length)], transition t of an
        episode being ring row (first + t) % ring_steps of that environment.  What `add_raw` does for a dense stream
        -- the same placement, evictions and serials, and on the device the same copies and the same fp64 arithmetic
        for Rn, done, w, cw and the episode weight, bit for bit -- with one small upload (descriptors, serials, discount
        powers) and one launch; no observation, policy or value crosses the host.  The strided reads of that launch
        have not been timed against `add_raw`'s dense ones.  An episode longer than `max_steps` is add_raw's
        ValueError, before anything is placed.  Returns the serial given to every episode, in order (an episode the
        collection itself evicts again has one, but is not stored)."""
        _check_nstep("add_steps", n, weight)
        episodes = [(int(env), int(first), int(T)) for env, first, T in episodes]
        if not episodes:
            return []
        if min(T for _, _, T in episodes) <= 0:
            raise ValueError("add_steps: episode lengths must be positive")
        self._check_dims(int(ring.obs_dim), int(ring.num_actions))
        placed = self._place_all([T for _, _, T in episodes])
        serials = [e.serial for _, e in placed]
        live = {e.serial for e in self._eps}
        kept = [(env, first, e) for (env, first, _), (_, e) in zip(episodes, placed) if e.serial in live]
        desc = np.array([[env, first, e.length, e.start, e.slot] for env, first, e in kept], np.int32)
        dstage, ptrs = self._upload(serial=np.array([e.serial for _, _, e in kept], np.int64), gpow=_gpow(gamma, n),
                                    desc=desc)
        a = _lib.args(_lib.MzsReplayStoreStepsArgs, episodes=len(kept), desc_host=desc.ctypes.data,
                      **_nstep_fields(n, _WEIGHT_MODES[weight], alpha), **ptrs)
        _lib.check(self._L.mzs_replay_store_steps(C.byref(self._arena), C.byref(ring), C.byref(a), self._stream()))
        self._keep = (dstage,)
        return serials

    def stalest(self, count):
        """Serials of up to `count` held episodes whose targets are the oldest: ordered by when they were last stored
        or reanalysed, earliest first (the episodes of one reanalysis tie; ties go by serial)."""
        order = sorted((e.serial for e in self._eps), key=lambda s: (self._touched[s], s))
        return order[:max(int(count), 0)]

    def reanalyse(self, model, key, n, gamma, alpha=None, weight="mean", serials=None, chunk_rows=4096, mask_fn=None,
                  **act_kwargs):
        """MuZero Reanalyse on the device: search the stored observations of the episodes `serials` (default: all
        held, oldest first; otherwise in the order given) again with `model` and overwrite, in place, their `pi`
        (search policy) and `v` (root value) and what follows from them -- `Rn`, `done`, `w = |v - Rn| ** alpha`
        (1 with alpha None), the prefix sums and the episode's buffer weight (`weight`: "mean" or "sum" of w), with
        the arithmetic of `add_raw` on the STORED float32 rewards.  Observations, actions, rewards, serials and
        the placement stay as they are, so nothing is evicted.

        The observations are gathered into one dense stream, zero-padded to `n_chunks = ceil(rows / chunk_rows)`
        chunks, and chunk c is searched as `model.act(keys[c], chunk, with_pi=True, with_value=True,
        obs_from_batch=True, device_outputs=True, **act_kwargs)` with `keys = prng.split(key, n_chunks)` (always
        split, also for one chunk); every call has exactly `chunk_rows` roots, so one search handle serves them all.
        `act_kwargs` reach act() untouched: its own defaults hold unless given here -- `num_simulations=5`,
        `temperature=1`, and the Dirichlet root noise `dirichlet_fraction=0.25` of acting; pass
        `dirichlet_fraction=0.0` for noise-free targets.  The actions act() returns are discarded.
        `mask_fn` (e.g. `Device2048.invalid_actions_of`): every chunk is searched with
        `invalid_actions=mask_fn(chunk)`, a uint8 [chunk_rows, A] device tensor with 1 where the action is illegal in
        that row's stored observation -- without it the search would write policies with weight on illegal moves into
        the buffer.  It is called on the padded rows as well (all-zero observations) and must leave such a row at least
        one legal action.  None: nothing changes, padded rows included.

        One upload (descriptors and discount powers), two launches around the searches; no device-to-host copy and
        no synchronisation beyond what act() does on its route.  A serial that is not held is a KeyError, a
        repeated one a ValueError, both before anything is launched.  Returns the number of transitions refreshed."""
        _check_nstep("reanalyse", n, weight)
        held = {e.serial: e for e in self._eps}
        serials = list(held) if serials is None else [int(s) for s in serials]
        if len(set(serials)) != len(serials):
            raise ValueError("reanalyse: a serial is given more than once")
        for s in serials:
            if s not in held:
                raise KeyError(f"no episode with serial {s} in the buffer")
        if not serials:
            return 0
        eps = [held[s] for s in serials]
        R = int(chunk_rows)
        plan = reanalyse_plan([e.length for e in eps], R)
        desc = np.array([[src, e.start, e.length, e.slot] for src, e in zip(plan.offsets, eps)], np.int32)
        dstage, ptrs = self._upload(gpow=_gpow(gamma, n), desc=desc)
        dev, f32, stream = self._device, torch.float32, self._stream()
        obs = torch.empty((plan.rows_padded, self.obs_dim), dtype=f32, device=dev)
        pi = torch.empty((plan.rows_padded, self.num_actions), dtype=f32, device=dev)
        v = torch.empty(plan.rows_padded, dtype=f32, device=dev)
        stream_args = dict(episodes=len(eps), stream_rows=plan.stream_rows, rows_padded=plan.rows_padded,
                           desc=ptrs["desc"], desc_host=desc.ctypes.data)
        g = _lib.args(_lib.MzsReplayGatherArgs, obs=obs.data_ptr(), **stream_args)
        _lib.check(self._L.mzs_replay_gather_obs(C.byref(self._arena), C.byref(g), stream))
        keys = prng.split(prng.as_key(key), plan.n_chunks)
        for c in range(plan.n_chunks):
            rows = slice(c * R, (c + 1) * R)
            mask = {} if mask_fn is None else {"invalid_actions": mask_fn(obs[rows])}
            _, pi_c, v_c = model.act(keys[c], obs[rows], with_pi=True, with_value=True, obs_from_batch=True,
                                     device_outputs=True, **mask, **act_kwargs)
            pi[rows].copy_(pi_c)
            v[rows].copy_(v_c)
        a = _lib.args(_lib.MzsReplayReanalyseArgs, gpow=ptrs["gpow"], pi=pi.data_ptr(), v=v.data_ptr(), **stream_args,
                      **_nstep_fields(n, _WEIGHT_MODES[weight], alpha))
        _lib.check(self._L.mzs_replay_reanalyse(C.byref(self._arena), C.byref(a), self._stream()))
        self._keep = (dstage, obs, pi, v)
        self._clock += 1
        for s in serials:
            self._touched[s] = self._clock
        self._dirty = True
        return plan.stream_rows

    def update_priorities(self, indices, priorities, alpha=1.0, eps=0.0, weight="mean"):
        """Priorities from training written back on the device: `indices` is the (serial [B], start [B]) pair of
        `sample(with_indices=True)`, `priorities` a device tensor or an array, [B, kp] for the first kp transitions
        of every window or [B] for the first one alone (the one whose weight decided the draw of the start).  The
        addressed transitions get w = (|p| + eps) ** alpha in fp64 (alpha in 0..1; exactly |p| + eps with alpha 1),
        their episodes new prefix sums and the buffer weight `weight` ("mean" or "sum") of their w; an episode no
        row addresses keeps every byte, the weight given to `add` included.  Where rows address one transition the
        last row wins, as in NumPy's w[idx] = p.  Skipped silently: a row whose episode has been evicted since the
        sample (or a zero-filled row, serial -1), a negative start, a transition past the episode's end, a NaN or
        infinite priority.  The search targets are not rewritten, so `stalest()` is unaffected.

        Two launches on caller-invisible scratch; no device-to-host copy and no synchronisation.  ValueError before
        anything is launched: indices and priorities that disagree in shape, alpha / eps / weight out of range, an
        empty buffer.  Returns None."""
        if weight not in _WEIGHT_MODES:
            raise ValueError("weight must be 'mean' or 'sum'")
        alpha, eps = float(alpha), float(eps)
        if not 0.0 <= alpha <= 1.0:
            raise ValueError("update_priorities: alpha must be in 0..1")
        if not (eps >= 0.0 and math.isfinite(eps)):
            raise ValueError("update_priorities: eps must be finite and not negative")
        try:
            serial, start = indices
        except (TypeError, ValueError):
            raise ValueError("update_priorities: indices must be the (serial, start) pair of sample(with_indices=True)")
        serial, start, prio = (x if isinstance(x, torch.Tensor) else np.asarray(x) for x in (serial, start, priorities))
        B = serial.shape[0] if serial.ndim == 1 else -1
        if B < 0 or tuple(start.shape) != (B,):
            raise ValueError(f"update_priorities: serial and start must be [B], got {tuple(serial.shape)} and "
                             f"{tuple(start.shape)}")
        if prio.ndim not in (1, 2) or prio.shape[0] != B or (prio.ndim == 2 and prio.shape[1] < 1):
            raise ValueError(f"update_priorities: priorities must be [B] or [B, kp >= 1] with B = {B}, got "
                             f"{tuple(prio.shape)}")
        if not self._eps:
            raise ValueError("cannot update the priorities of an empty buffer")
        if B == 0:
            return
        dev = self._device
        serial, start, prio = (torch.as_tensor(x).to(device=dev, dtype=dt).contiguous() for x, dt in
                               ((serial, torch.int64), (start, torch.int32), (prio, torch.float32)))
        if self._prio_scratch is None:  # owner [max_steps] = -1, touched [capacity] = 0; the kernels leave them so
            self._prio_scratch = (torch.full((self._max_steps,), -1, dtype=torch.int32, device=dev),
                                  torch.zeros(self._capacity, dtype=torch.int32, device=dev))
        u = _lib.args(_lib.MzsReplayUpdateArgs)  # (per training step: fields by attribute, which is 1 us cheaper)
        u.head, u.count, u.batch, u.k_prio = self._head, len(self._eps), B, prio.shape[1] if prio.ndim == 2 else 1
        u.weight_mode, u.alpha, u.eps = _WEIGHT_MODES[weight], alpha, eps
        u.serial, u.start, u.prio = serial.data_ptr(), start.data_ptr(), prio.data_ptr()
        u.owner, u.touched = (x.data_ptr() for x in self._prio_scratch)
        _lib.check(self._L.mzs_replay_update_priorities(C.byref(self._arena), C.byref(u), self._stream()))
        self._keep = (serial, start, prio)
        self._dirty = True

    def sample(self, batch_size=32, num_trajectory: int = None, k_steps: int = 5, sample_per_trajectory: int = 1,
               key=None, with_indices: bool = False, is_beta=None, is_normalize: bool = True, all_obs: bool = False):
        """A batch of `num_trajectory * sample_per_trajectory` windows of `k_steps` transitions (the arguments of
        muax/replay_buffer.py:192-240; `batch_size` alone means that many trajectories, one window each) as a
        Transition of device tensors: obs [B, 1, obs_dim], a [B, k] int32, r / Rn / v / w [B, k] float32, done
        [B, k] bool, pi [B, k, A] float32.  Episodes are drawn with their buffer weights, the start inside an
        episode with the transition weights, the rows of one trajectory sharing their episode.  The batch size is
        fixed: an episode no longer than `k_steps` is never drawn (the reference returns a shorter batch).
        `key`: an int seed or two uint32 words fix the draws; default: the buffer's own key, split on every call.
        `with_indices=True` returns (batch, (episode serial [B] int64, start [B] int32)).

        `is_beta`, a float in 0..1, adds the importance-sampling weights of the rows as a trailing `isw` [B] float32
        device tensor -- (batch, isw), or (batch, (serial, start), isw) with the indices -- for
        `MuZero.update(batch, sample_weight=isw)`: isw = (N q) ** -is_beta in fp64, q the probability with which the
        row's window was drawn (episode times start), N the number of windows the buffer could have drawn (the sum
        of length - k_steps over the episodes longer than k_steps); `is_normalize` (default) divides by the largest
        weight of the batch, so that the weights only ever scale a step down.  A zero-filled row gets 0.  The draws
        and every field are those of the call without `is_beta`, bit for bit, and nothing is copied to the host or
        synchronised: one more small launch for the normalisation.  Outside 0..1 or not finite: ValueError before
        any launch.  None: no weights, today's return value.

        `all_obs=True`: obs is [B, k_steps, obs_dim], the observation of EVERY transition of the window -- what
        `loss.stochastic_loss_fn` and the fused stochastic training step read (the chance code of transition i is
        encoded from obs_i).  The same launch copies them: a window's observations are one contiguous run of the
        arena.  Every other field, the indices and `isw` are those of the call without it for the same key, bit for
        bit, and obs[:, 0] is that call's obs[:, 0].  `value_priorities`, `unroll_values` and `default_loss_fn` read
        obs[:, 0] alone and are therefore indifferent to the flag.  False: obs [B, 1, obs_dim], today's return value."""
        if is_beta is not None:
            is_beta = float(is_beta)
            if not 0.0 <= is_beta <= 1.0:  # (False for NaN)
                raise ValueError("sample: is_beta must be None or a number in 0..1")
        if batch_size is None and num_trajectory is None:
            raise ValueError("Either num_trajectory or batch_size need to be given.")
        elif batch_size is not None and num_trajectory is None:
            num_trajectory, sample_per_trajectory = batch_size, 1
        if not self._eps:
            raise ValueError("cannot sample from an empty buffer")
        k, spt = int(k_steps), int(sample_per_trajectory)
        B = int(num_trajectory) * spt
        stream = self._stream()
        if self._dirty or self._table_k != k:
            self._windows = self.eligible_windows(k)  # (isw's N)
            self._eligible = self._windows > 0
            _lib.check(self._L.mzs_replay_refresh(C.byref(self._arena), self._head, len(self._eps), k, stream))
            self._dirty, self._table_k = False, k
        if not self._eligible:
            raise ValueError(f"no episode in the buffer is longer than k_steps = {k}")
        if key is None:
            self._key, key = prng.split(self._key)
        else:
            key = prng.as_key(key)
        dev, f32 = self._device, torch.float32
        obs = torch.empty((B, k if all_obs else 1, self.obs_dim), dtype=f32, device=dev)
        a = torch.empty((B, k), dtype=torch.int32, device=dev)
        r, Rn, v, w = (torch.empty((B, k), dtype=f32, device=dev) for _ in range(4))
        done = torch.empty((B, k), dtype=torch.bool, device=dev)
        pi = torch.empty((B, k, self.num_actions), dtype=f32, device=dev)
        serial = torch.empty(B, dtype=torch.int64, device=dev)
        start = torch.empty(B, dtype=torch.int32, device=dev)
        s = _lib.args(_lib.MzsReplaySampleArgs)  # (per training step: fields by attribute, which is 1 us cheaper)
        s.count, s.batch, s.k_steps, s.sample_per_trajectory = len(self._eps), B, k, spt
        s.obs_steps = k if all_obs else 0
        s.key[0], s.key[1] = int(key[0]), int(key[1])
        s.obs, s.a, s.r, s.Rn, s.v, s.done = (x.data_ptr() for x in (obs, a, r, Rn, v, done))
        s.pi, s.w, s.serial, s.start = pi.data_ptr(), w.data_ptr(), serial.data_ptr(), start.data_ptr()
        batch = self.transition_class(obs=obs, a=a, r=r, done=done, Rn=Rn, v=v, pi=pi, w=w)
        if is_beta is None:
            _lib.check(self._L.mzs_replay_sample(C.byref(self._arena), C.byref(s), stream))
            return (batch, (serial, start)) if with_indices else batch
        isw = torch.empty(B, dtype=f32, device=dev)
        if is_normalize and (self._is_scratch is None or self._is_scratch.numel() < B):
            self._is_scratch = torch.empty(B, dtype=torch.float64, device=dev)  # raw weights; grows with the batch
        q = _lib.args(_lib.MzsReplayIsArgs)
        q.normalize, q.beta, q.num_windows = int(bool(is_normalize)), is_beta, float(self._windows)
        q.isw, q.scratch = isw.data_ptr(), self._is_scratch.data_ptr() if is_normalize else None
        _lib.check(self._L.mzs_replay_sample_is(C.byref(self._arena), C.byref(s), C.byref(q), stream))
        return (batch, (serial, start), isw) if with_indices else (batch, isw)
