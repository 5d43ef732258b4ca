"""`DeviceVectorCollector` with a device environment (muax_amd/envs.DeviceCartPole) end to end, independent of any
libm: route A collects with the environment stepped on the device; route B is the collector's host branch on a
test-local replay environment that hands back route A's recorded observations, rewards and flags whatever action it is
given, with an equal-weight copy of the model, the same key and a fresh buffer.  Both must leave the same bits in every
arena and table, the same serials, the same `finished` lists and the same keys, and the actions route B's environment
receives must be the ring's.

5 environments, max_episode_steps 7, a ring of 12 rows, calls of 4, 5 and 4 steps (the third wraps), 8 simulations,
min_length 3.  From a start state in +-0.05 no cart-pole can fall within 7 steps (on the reference the earliest
termination over the corner states under a constant push is step 8), so with this limit every episode is cut at 7
steps whatever the seed; episodes shorter than min_length come from environments that begin part-way through an
episode: the test's environment sets the step counters `t` to (0, 5, 6, 3, 0) after its first reset, a plain write to the
environment's own tensor.  That gives dropped episodes of 2 and 1 steps, a stored one of 4, carried ones of 7."""
import functools

import numpy as np
import pytest
import torch

import cartpole_reference as cp
import muax_amd as mx
from helpers import train_model

pytestmark = pytest.mark.gpu
N, MAX_STEPS, RING, CALLS, SIMS, MIN_LENGTH, N_STEP, GAMMA, ALPHA = 5, 7, 12, (4, 5, 4), 8, 3, 5, 0.997, 0.5
T0 = (0, 5, 6, 3, 0)
SEED = 17


class StaggeredCartPole(mx.DeviceCartPole):
    """DeviceCartPole whose environments are T0 steps into their first episode."""

    def reset_device(self):
        obs = super().reset_device()
        self._t.copy_(torch.tensor(T0, dtype=torch.int32))
        return obs


class ReplayEnv:
    """Host-protocol environment that replays recorded steps and keeps the actions it was given."""

    def __init__(self, obs, r, done):
        self.obs, self.r, self.done = obs, r, done  # [T, N, 4], [T, N], [T, N]
        self.n, self.spec = obs.shape[1], cp_spec(MAX_STEPS)
        self.s, self.actions = 0, []

    def reset(self):
        return self.obs[0].copy()

    def step(self, actions):
        self.actions.append(np.asarray(actions).copy())
        r, d = self.r[self.s].copy(), self.done[self.s].copy()
        self.s += 1
        nxt = self.obs[self.s].copy() if self.s < len(self.obs) else np.zeros_like(self.obs[0])  # (never acted on)
        return nxt, r, d


def cp_spec(max_episode_steps):
    from types import SimpleNamespace
    return SimpleNamespace(max_episode_steps=max_episode_steps)


def _model():
    return train_model(2, 8, 4, seed=3, support=10)


def test_the_schedule_stores_and_drops_on_the_reference():
    """The cap that keeps the comparison below from comparing nothing, checked on the loop reference with random
    actions before any device result is looked at: at least two episodes stored, at least one dropped."""
    rng, key = np.random.default_rng(0), mx.prng.PRNGKey(SEED)
    envs = [(cp.draw(key, e, 0), T0[e], 1) for e in range(N)]
    lengths, age = [], [0] * N
    for _ in range(sum(CALLS)):
        for e in range(N):
            s, t, d, _, done = cp.step(*envs[e], int(rng.integers(0, 2)), key, e, MAX_STEPS)
            envs[e], age[e] = (s, t, d), age[e] + 1
            if done:
                lengths.append(age[e])
                age[e] = 0
    assert sum(T >= MIN_LENGTH for T in lengths) >= 2 and sum(T < MIN_LENGTH for T in lengths) >= 1


@functools.lru_cache(maxsize=None)
def _routes():
    model_a, model_b = _model(), _model()
    for pa, pb in zip((p for m in model_a.network for p in m.parameters()),
                      (p for m in model_b.network for p in m.parameters())):
        assert torch.equal(pa, pb)
    buf_a, buf_b = (mx.DeviceReplayBuffer(16, 128, random_seed=0) for _ in range(2))
    env = StaggeredCartPole(N, max_episode_steps=MAX_STEPS, seed=SEED)
    dev = mx.DeviceVectorCollector(env, buf_a, N_STEP, GAMMA, ALPHA, min_length=MIN_LENGTH, ring_steps=RING)
    key = mx.prng.PRNGKey(7)
    rec = {k: [] for k in ("obs", "a", "r", "done")}
    fin_a, keys_a, step0 = [], [], 0
    for steps in CALLS:
        fin, key, count = dev.collect(model_a, key, steps, num_simulations=SIMS)
        assert count == steps * N
        rows = [(step0 + i) % RING for i in range(steps)]
        for k in ("obs", "a", "r"):
            rec[k].append(dev._fields[k][rows].cpu().numpy())
        rec["done"].append(dev._done_rows[rows].cpu().numpy().astype(bool))
        fin_a.append(fin), keys_a.append(np.array(key))
        step0 += steps
    rec = {k: np.concatenate(v) for k, v in rec.items()}
    replay = ReplayEnv(rec["obs"], rec["r"], rec["done"])
    host = mx.DeviceVectorCollector(replay, buf_b, N_STEP, GAMMA, ALPHA, min_length=MIN_LENGTH, ring_steps=RING)
    key = mx.prng.PRNGKey(7)
    fin_b, keys_b = [], []
    for steps in CALLS:
        fin, key, _ = host.collect(model_b, key, steps, num_simulations=SIMS)
        fin_b.append(fin), keys_b.append(np.array(key))
    torch.cuda.synchronize()
    return dict(buf_a=buf_a, buf_b=buf_b, rec=rec, replay=replay, fin_a=fin_a, fin_b=fin_b, keys_a=keys_a,
                keys_b=keys_b, dev=dev, host=host)


def _bits(x):
    return x.view({4: torch.int32, 8: torch.int64, 1: torch.uint8}[x.element_size()])


def test_device_environment_route_equals_the_host_branch_on_its_recorded_steps():
    R = _routes()
    a, b, rec = R["buf_a"], R["buf_b"], R["rec"]
    every = [x for fin in R["fin_a"] for x in fin]
    stored = [x for x in every if x[2] is not None]
    assert len(stored) >= 2 and len(every) - len(stored) >= 1  # the cap: something was stored, something dropped
    assert [T for T, _, _ in every if T < MIN_LENGTH] and all(s is None for T, _, s in every if T < MIN_LENGTH)
    assert R["fin_a"] == R["fin_b"]
    assert all(np.array_equal(x, y) for x, y in zip(R["keys_a"], R["keys_b"]))
    assert a.serials == b.serials == [s for _, _, s in stored] and len(a) == len(stored) and a.steps == b.steps
    assert (a._head, a._tail, a._steps, a._serial, a._clock) == (b._head, b._tail, b._steps, b._serial, b._clock)
    assert set(a._t) == set(b._t)
    for name in a._t:  # every arena and both tables
        assert torch.equal(_bits(a._t[name]), _bits(b._t[name])), name
    # the tables of the live episodes, written by the first sample
    ba, ia = a.sample(num_trajectory=6, sample_per_trajectory=2, k_steps=3, key=5, with_indices=True)
    bb, ib = b.sample(num_trajectory=6, sample_per_trajectory=2, k_steps=3, key=5, with_indices=True)
    assert torch.equal(ia[0], ib[0]) and torch.equal(ia[1], ib[1])
    for name in a._t:
        assert torch.equal(_bits(a._t[name]), _bits(b._t[name])), name
    for k in ("obs", "a", "r", "Rn", "v", "done", "pi", "w"):
        assert torch.equal(getattr(ba, k), getattr(bb, k)), k
    # route B's environment was given the ring's actions
    assert np.array_equal(np.stack(R["replay"].actions), rec["a"])
    # and the two rings agree row by row (the last call's 12 rows)
    for k in ("obs", "a", "r", "v", "pi"):
        assert torch.equal(_bits(R["dev"]._fields[k]), _bits(R["host"]._fields[k])), k


def test_recorded_steps_are_the_cartpoles():
    """What route A recorded is an environment's stream: rewards of 1, every flag where the reference's step counter
    says (truncation at 7 steps, the first episodes shortened by T0), observations of a finished environment the
    reference's start states bit for bit, and lengths and returns of `finished` to match."""
    R = _routes()
    rec, key = R["rec"], mx.prng.PRNGKey(SEED)
    assert (rec["r"] == 1.0).all() and rec["obs"].dtype == np.float32
    t, draws, want_len = list(T0), [1] * N, []
    age = [0] * N
    assert np.array_equal(rec["obs"][0], np.array([cp.draw(key, e, 0) for e in range(N)]).astype(np.float32))
    for s in range(sum(CALLS)):
        for e in range(N):
            t[e], age[e] = t[e] + 1, age[e] + 1
            done = t[e] >= MAX_STEPS
            assert bool(rec["done"][s, e]) == done, (s, e)
            if done:
                if s + 1 < sum(CALLS):
                    want = np.array(cp.draw(key, e, draws[e])).astype(np.float32)
                    assert np.array_equal(rec["obs"][s + 1, e], want), (s, e)
                t[e], draws[e] = 0, draws[e] + 1
                want_len.append((e, s, age[e]))
                age[e] = 0
    got = [T for fin in R["fin_a"] for T, _, _ in fin]
    assert sorted(got) == sorted(T for _, _, T in want_len)
    assert all(G == float(T) for fin in R["fin_a"] for T, G, _ in fin)
    assert np.array_equal(R["dev"].venv._draws.cpu().numpy(), np.array(draws))


def test_fit_vector_device_collect_with_a_device_environment():
    g = torch.Generator().manual_seed(0)
    net = mx.nn.MZNetwork(mx.nn.Representation(8, generator=g), mx.nn.Prediction(2, 21, generator=g),
                          mx.nn.Dynamic(8, 2, 21, generator=g))
    model = mx.MuZero(net, optimizer=mx.optimizers.create_optimizer("adam", 5e-3))
    buf, rows = mx.DeviceReplayBuffer(64, 4096, random_seed=13), []
    venv = mx.DeviceCartPole(8, max_episode_steps=6, seed=1)
    mx.fit_vector(model, venv, mx.DeviceCartPole(2, max_episode_steps=5, seed=2), n_step=3, alpha=None, buffer=buf,
                  iterations=2, steps_per_iteration=8, num_simulations=4, k_steps=3, num_trajectory=8,
                  sample_per_trajectory=2, num_update_per_iteration=3, test_interval=10, random_seed=3, metrics=rows,
                  device_collect=True)
    assert len(rows) == 2 and len(buf) == 16 and buf.steps == 16 * 6
    assert [r["episodes"] for r in rows] == [8, 8] and all(r["G"] == 6.0 for r in rows)
    assert np.isfinite(rows[-1]["loss"]) and rows[0]["test_G"] == 5.0
    with pytest.raises(ValueError, match="device_collect"):
        mx.fit_vector(model, venv, None, buffer=buf, device_collect=False)
