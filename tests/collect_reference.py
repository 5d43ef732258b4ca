"""Plain-loop reference of collection on the device ("Collecting"), for test_collect_cpu.py,
test_gpu_collect_kernels.py and test_gpu_collect.py: which episodes a call finishes (`ring_plan`), and what the store
launch must leave in the arenas and the table for a ring and its descriptors.  One step and one transition at a time;
the n-step arithmetic is tests/nstep_reference.py's.  Also the scripted vector environment and the stub model the
tests share.  Nothing from muax_amd."""
import numpy as np

import nstep_reference as nref


def ring_plan(done, open_start, step0, min_length=1):
    """(finished, dropped, new open_start) with episodes as (environment, first absolute step, length), environment by
    environment and inside one in the order of time."""
    T, N = len(done), len(open_start)
    finished, dropped, new_open = [], [], []
    for env in range(N):
        first = int(open_start[env])
        for t in range(T):
            if done[t][env]:
                length = step0 + t - first + 1
                (finished if length >= min_length else dropped).append((env, first, length))
                first = step0 + t + 1
        new_open.append(first)
    return finished, dropped, new_open


def ring_episode(ring, ring_steps, env, first, length):
    """The transitions of one episode read out of the ring's host arrays ([ring_steps, N, ...]), one row at a time."""
    out = {k: [] for k in ("obs", "a", "r", "v", "pi")}
    for t in range(length):
        row = (first + t) % ring_steps
        for k in out:
            out[k].append(ring[k][row][env])
    return {k: np.stack(x) for k, x in out.items()}


def expected_store(ring, ring_steps, desc, n, gamma, alpha, weight):
    """Per descriptor {env, first ring row, length, first arena row, slot}: the arena rows and the table row the store
    launch must write -- obs, a, v, pi copied, r rounded to float32, Rn / done / w / cw and the episode weight by the
    loop reference on the fp64 rewards and the widened fp32 values."""
    out = []
    for env, first, length, dst, slot in desc:
        ep = ring_episode(ring, ring_steps, int(env), int(first), int(length))
        r = [float(x) for x in ep["r"]]
        v = [float(x) for x in ep["v"]]  # fp32 -> Python float: exact
        Rn, done, w, cw, ep_w = nref.episode(r, v, n, gamma, alpha, weight)
        out.append(dict(dst=int(dst), slot=int(slot), length=int(length), obs=ep["obs"].astype(np.float32),
                        a=ep["a"].astype(np.int32), r=np.array(r, np.float64).astype(np.float32),
                        v=ep["v"].astype(np.float32), pi=ep["pi"].astype(np.float32),
                        Rn=np.array(Rn, np.float64).astype(np.float32), done=np.array(done, bool),
                        w=np.array(w, np.float64), cw=np.array(cw, np.float64), t_w=float(ep_w)))
    return out


class Spec:
    def __init__(self, max_episode_steps):
        self.max_episode_steps = int(max_episode_steps)


class ScriptedVecEnv:
    """A vector environment whose `done` flags and rewards are a fixed table [S, N] (step s of the run, whatever the
    actions were; the table repeats after S steps) and whose observation encodes (environment, step): nothing depends
    on the actions.  Counts its `step` calls."""

    def __init__(self, done, rewards, obs_dim=4, max_episode_steps=1000, seed=0):
        self.done, self.rewards = np.asarray(done, bool), np.asarray(rewards, np.float64)
        self.S, self.N = self.done.shape
        self.obs_dim, self.spec = int(obs_dim), Spec(max_episode_steps)
        self.noise = np.random.default_rng(seed).uniform(-1, 1, (self.S + 1, self.N, self.obs_dim)).astype(np.float32)
        self.s = self.step_calls = 0

    def _obs(self):
        obs = self.noise[self.s % (self.S + 1)].copy()
        obs[:, 0] = np.arange(self.N)  # (environment, absolute step) in the first two columns
        if self.obs_dim > 1:
            obs[:, 1] = self.s
        return obs

    def reset(self):
        self.s = 0
        return self._obs()

    def step(self, actions):
        assert len(actions) == self.N
        self.step_calls += 1
        r, d = self.rewards[self.s % self.S].copy(), self.done[self.s % self.S].copy()
        self.s += 1
        return self._obs(), r, d


class StubModel:
    """act() that returns fixed arrays computed from the observation alone."""

    def __init__(self, A=2):
        self.A = A

    def act(self, key, obs, with_pi=False, with_value=False, obs_from_batch=False, **kw):
        obs = np.asarray(obs, np.float32)
        a = (np.abs(obs).sum(1).astype(np.int64) % self.A).astype(np.int32)
        pi = np.full((len(obs), self.A), 1.0 / self.A, np.float32)
        v = (obs.sum(1) * 0.125).astype(np.float32)
        return (a, pi, v) if (with_pi and with_value) else a
