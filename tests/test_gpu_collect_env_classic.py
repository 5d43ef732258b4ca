"""Collection and greedy evaluation on the device environments that are not the cart-pole: `DeviceAcrobot`
(6 observations, 3 actions, rewards -1 and a terminating 0) and `DeviceMountainCar` (2 observations, 3 actions).

For both: 5 environments, max_episode_steps 7, 20 steps in calls of 8, 7 and 5, 5 simulations.  `DeviceVectorCollector`
with the plan on the host and on the device (`device_plan`) must hand out the same `finished` lists and serials and
leave the same bits in every arena and table; and both must equal `VectorCollector` on the same environment's HOST
protocol (same seed, so the same stream: the two protocols are one environment) with its trajectories flattened into
`add_raw` -- the same lengths and returns in the same order, the same serials and, episode by episode, the same stored
bits in every field.

The Acrobot environments begin near the top (a test-local subclass writes the start states of the first reset: th1
close to pi, where -cos th1 - cos(th1 + th2) > 1 after one step), so their first episodes terminate with reward 0 and a
return of 0.0 next to the truncated ones of -7.0.

`test_vector_device` against `test_vector`: exact equality of the value, on `DeviceCartPole` and `DeviceAcrobot`, also
with a `max_steps` below the episode length, where no environment finishes."""
import functools

import numpy as np
import pytest
import torch

import acrobot_reference as ac
import mountaincar_reference as mc
import muax_amd as mx
from helpers import train_model

pytestmark = pytest.mark.gpu
N, MAX_STEPS, CALLS, SIMS, N_STEP, GAMMA, ALPHA, MIN_LENGTH = 5, 7, (8, 7, 5), 5, 3, 0.997, 0.5, 1
SEED = 23
TOP = {0: [3.0, 0.1, 0.0, 0.0], 3: [-3.0, -0.1, 0.0, 0.0]}  # environments that begin one step from termination


class AcrobotFromTheTop(mx.DeviceAcrobot):
    """DeviceAcrobot whose environments 0 and 3 begin their FIRST episode near the top: a plain write to the
    environment's own tensors after its first reset (the observation is rewritten to match)."""

    def reset_device(self):
        obs = super().reset_device()
        for e, s in TOP.items():
            self._state[e] = torch.tensor(s, dtype=torch.float64)
            obs[e] = torch.tensor(ac.obs(s), dtype=torch.float64).to(torch.float32)
        return obs


ENVS = {"acrobot": (AcrobotFromTheTop, ac), "mountaincar": (mx.DeviceMountainCar, mc)}
BOTH = pytest.mark.parametrize("name", list(ENVS))


def _model(ref):
    return train_model(ref.NUM_ACTIONS, 8, ref.OBS_DIM, seed=3, support=10)


def _bits(x):
    return x.view({4: torch.int32, 8: torch.int64, 1: torch.uint8}[x.element_size()])


def _flat(trajs):
    """Host trajectories as add_raw's flat stream."""
    bt = [t.batched_transitions for t in trajs]
    lengths = [len(t) for t in trajs]
    cat = {k: np.concatenate([np.asarray(getattr(b, k))[0].reshape(T, -1) for b, T in zip(bt, lengths)])
           for k in ("obs", "a", "r", "v", "pi")}
    return cat["obs"], cat["a"][:, 0], cat["r"][:, 0], cat["v"][:, 0], cat["pi"], lengths


@functools.lru_cache(maxsize=None)
def _routes(name):
    cls, ref = ENVS[name]
    out = {}
    for route in ("host_plan", "device_plan"):
        model, buf = _model(ref), mx.DeviceReplayBuffer(32, 256, random_seed=0)
        col = mx.DeviceVectorCollector(cls(N, max_episode_steps=MAX_STEPS, seed=SEED), buf, N_STEP, GAMMA, ALPHA,
                                       min_length=MIN_LENGTH, device_plan=route == "device_plan")
        key, fins, keys = mx.prng.PRNGKey(7), [], []
        for steps in CALLS:
            fin, key, count = col.collect(model, key, steps, num_simulations=SIMS)
            assert count == steps * N
            fins.append(fin), keys.append(np.array(key))
        out[route] = dict(buf=buf, fins=fins, keys=keys, col=col)
    # VectorCollector on the host protocol of the same environment
    model, buf = _model(ref), mx.DeviceReplayBuffer(32, 256, random_seed=0)
    col = mx.VectorCollector(cls(N, max_episode_steps=MAX_STEPS, seed=SEED), N_STEP, GAMMA, ALPHA)
    key, trajs, keys = mx.prng.PRNGKey(7), [], []
    for steps in CALLS:
        tr, key, _ = col.collect(model, key, steps, num_simulations=SIMS)
        if tr:
            buf.add_raw(*_flat(tr), N_STEP, GAMMA, ALPHA, weight="mean")
        trajs.append(tr), keys.append(np.array(key))
    out["host"] = dict(buf=buf, trajs=trajs, keys=keys)
    torch.cuda.synchronize()
    return out


@BOTH
def test_device_plan_off_and_on_give_the_same_episodes_and_bits(name):
    R = _routes(name)
    a, b = R["host_plan"], R["device_plan"]
    every = [x for fin in a["fins"] for x in fin]
    assert len(every) >= 2 * N  # 20 steps of episodes of at most 7: every environment finished at least two
    assert a["fins"] == b["fins"]
    assert all(np.array_equal(x, y) for x, y in zip(a["keys"], b["keys"]))
    ba, bb = a["buf"], b["buf"]
    assert ba.serials == bb.serials == [s for _, _, s in every] and len(ba) == len(every) and ba.steps == bb.steps
    assert set(ba._t) == set(bb._t)
    for n in ba._t:
        assert torch.equal(_bits(ba._t[n]), _bits(bb._t[n])), n
    for k in ("obs", "a", "r", "v", "pi"):
        assert torch.equal(_bits(a["col"]._fields[k]), _bits(b["col"]._fields[k])), k
    assert torch.equal(a["col"].venv._state, b["col"].venv._state)


@BOTH
def test_both_equal_vector_collector_on_the_host_protocol(name):
    R = _routes(name)
    _, ref = ENVS[name]
    dev, host = R["host_plan"], R["host"]
    assert all(np.array_equal(x, y) for x, y in zip(dev["keys"], host["keys"]))
    for fin, trajs in zip(dev["fins"], host["trajs"]):  # the same episodes in the same order, call by call
        assert [(T, G) for T, G, _ in fin] == [(len(t), float(np.sum(t.rewards))) for t in trajs]
    every = [t for trajs in host["trajs"] for t in trajs]
    for route in ("host_plan", "device_plan"):
        bd, bh = R[route]["buf"], host["buf"]
        assert bd.serials == bh.serials and len(bd) == len(every) and bd.steps == bh.steps == sum(len(t) for t in every)
        for s in bd.serials:  # the stored bits, episode by episode: the ring route == add_raw of the host's episodes
            ed, eh = bd.episode(s), bh.episode(s)
            assert tuple(ed.obs.shape[1:]) == (ref.OBS_DIM,) and ed.pi.shape[-1] == ref.NUM_ACTIONS
            for k in ("obs", "a", "r", "Rn", "v", "done", "pi", "w"):
                gx, gy = getattr(ed, k), getattr(eh, k)
                assert gx.dtype == gy.dtype and gx.shape == gy.shape and torch.equal(gx, gy), (route, s, k)


def test_acrobot_returns_include_the_terminating_zero():
    R = _routes("acrobot")
    first = R["host_plan"]["fins"][0]
    got = {(T, G) for T, G, _ in first}
    assert (1, 0.0) in got  # one step, terminated: its only reward is the 0
    assert (MAX_STEPS, -float(MAX_STEPS)) in got  # truncated: -1 on every step
    # on the reference: the two environments from the top terminate at once, with reward 0
    for e, s in TOP.items():
        assert ac.margin(s, 1) >= 1e-6
        for a in (0, 1, 2):
            assert ac.step(s, 0, 1, a, mx.prng.PRNGKey(SEED), e, MAX_STEPS)[3:] == (0.0, True)
    assert sum(1 for T, G, _ in first if (T, G) == (1, 0.0)) == len(TOP)
    every = [x for fin in R["host_plan"]["fins"] for x in fin]
    assert all(G == -float(T) or (T, G) == (1, 0.0) for T, G, _ in every)  # small integers: sums are exact


def test_mountaincar_returns_are_minus_the_length():
    every = [x for fin in _routes("mountaincar")["host_plan"]["fins"] for x in fin]
    assert every and all(T == MAX_STEPS and G == -float(MAX_STEPS) for T, G, _ in every)


EVAL = {"cartpole": (lambda **kw: mx.DeviceCartPole(6, **kw), 2, 4),
        "acrobot": (lambda **kw: mx.DeviceAcrobot(6, **kw), 3, 6)}


@pytest.mark.parametrize("name", list(EVAL))
@pytest.mark.parametrize("max_episode_steps,max_steps", [(9, None), (20, None), (20, 5)])
def test_vector_device_equals_test_vector(name, max_episode_steps, max_steps):
    """(9, None): every environment finishes after 9 steps, before the first "all finished" check at step 16; (20,
    None): the check at step 16 finds them live, the loop runs out at 20; (20, 5): max_steps ends the loop with every
    environment still in its first episode."""
    make, A, obs_dim = EVAL[name]
    model = train_model(A, 8, obs_dim, seed=5, support=10)
    key = mx.prng.PRNGKey(11)
    want = mx.test_vector(model, make(max_episode_steps=max_episode_steps, seed=4), key, SIMS, max_steps=max_steps)
    got = mx.test_vector_device(model, make(max_episode_steps=max_episode_steps, seed=4), key, SIMS, max_steps=max_steps)
    assert got == want and np.isfinite(want)
    if name == "acrobot":
        assert want == -float(max_steps or max_episode_steps)


def test_vector_device_stops_at_the_sixteenth_step_when_all_finished():
    """max_episode_steps 3 and 40 allowed steps: every first episode is over after 3 steps, the check after step 16
    ends the loop -- 16 environment steps, not 40 -- and the value is test_vector's, which stopped after 3."""
    model = train_model(3, 8, 6, seed=5, support=10)
    key = mx.prng.PRNGKey(2)
    host_env, dev_env = (mx.DeviceAcrobot(4, max_episode_steps=3, seed=9) for _ in range(2))
    want = mx.test_vector(model, host_env, key, SIMS, max_steps=40)
    got = mx.test_vector_device(model, dev_env, key, SIMS, max_steps=40)
    assert got == want == -3.0
    assert int(host_env._draws[0]) == 2 and int(dev_env._draws[0]) == 1 + 16 // 3


def test_fit_vector_evaluates_a_device_test_env_on_the_device():
    g = torch.Generator().manual_seed(0)
    net = mx.nn.MZNetwork(mx.nn.Representation(8, generator=g), mx.nn.Prediction(3, 21, generator=g),
                          mx.nn.Dynamic(8, 3, 21, generator=g))
    model = mx.MuZero(net, optimizer=mx.optimizers.create_optimizer("adam", 5e-3))
    buf, rows = mx.DeviceReplayBuffer(64, 4096, random_seed=13), []

    class Counting(mx.DeviceAcrobot):
        host_steps = 0

        def step(self, actions):
            Counting.host_steps += 1
            return super().step(actions)

    mx.fit_vector(model, mx.DeviceAcrobot(8, max_episode_steps=6, seed=1), Counting(2, max_episode_steps=5, seed=2),
                  n_step=3, alpha=None, buffer=buf, iterations=1, steps_per_iteration=6, num_simulations=4, k_steps=3,
                  num_trajectory=8, sample_per_trajectory=2, num_update_per_iteration=2, test_interval=10,
                  random_seed=3, metrics=rows, device_collect=True, device_plan=True)
    assert len(rows) == 1 and rows[0]["episodes"] == 8 and rows[0]["G"] == -6.0 and rows[0]["test_G"] == -5.0
    assert Counting.host_steps == 0 and np.isfinite(rows[0]["loss"])
