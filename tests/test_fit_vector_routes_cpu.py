"""CPU tests of the routing of fit_vector and of the two collectors (muax_amd/vector.py): what is refused, with which
text and in which order; which calls the loop makes on the model, the buffer and the environments, in which order and
with which arguments and keys; and the metrics rows.  No GPU and no library: the model, the buffers and the environments
are scripted recorders, the "device" of the device route is the CPU and the two C calls of that route are recorded.
The GPU suites check what the routes compute; this file pins the routing itself."""
import inspect
import itertools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import collect_reference as cref
import muax_amd as mx
from muax_amd import prng, vector

N, STEPS, K = 3, 4, 2          # environments, steps per iteration, k_steps
N_STEP, GAMMA, ALPHA = 2, 0.9, 0.5
SAMPLE_BASE = dict(num_trajectory=4, k_steps=K, sample_per_trajectory=1)


def _k(key):
    return tuple(int(x) for x in np.asarray(key).ravel())


# ---------------------------------------------------------------------------------------------------------- the fakes
class Model:
    """Records every call.  act() is a function of the observation alone and keeps what it returned."""
    device = torch.device("cpu")

    def __init__(self, log, stochastic=False, unrolls=False):
        self.log, self.trains_stochastic, self.unrolls_stochastic = log, stochastic, unrolls
        self.acted, self.updates = [], 0

    def init(self, key, sample):
        self.log.append(("init", _k(key), np.asarray(sample).tolist()))

    def act(self, key, obs, **kw):
        self.log.append(("act", _k(key), kw))
        x = (obs.numpy() if isinstance(obs, torch.Tensor) else np.asarray(obs, np.float32)).reshape(len(obs), -1)
        a = np.abs(x).sum(1).astype(np.int64) % 2
        pi = (0.25 + 0.5 * (np.arange(2)[None] == a[:, None])).astype(np.float32)
        v = (x.sum(1) * 0.125).astype(np.float32)
        if not kw.get("with_pi"):
            return torch.from_numpy(a) if kw.get("device_outputs") else a
        self.acted.append((x.copy(), a, pi, v))
        return tuple(torch.from_numpy(y) for y in (a, pi, v)) if kw.get("device_outputs") else (a, pi, v)

    def update(self, batch, **kw):
        self.updates += 1
        self.log.append(("update", batch, kw))
        return {"loss": float(self.updates)}

    def unroll_values(self, batch, k_prio=None, backend="auto"):
        self.log.append(("unroll_values", batch, k_prio, backend))
        return None, ("unrolled", batch, k_prio)


def make_buffer(log, add_many=True, priorities=True, is_beta=True, all_obs=True, reanalyse=True, store=False):
    """A recording buffer that offers or lacks each capability fit_vector looks for.  `store`: the device store as
    far as DeviceVectorCollector touches it, on the CPU, with the library's two entry points recorded."""
    takes = tuple(SAMPLE_BASE) + ("batch_size",) + (("with_indices",) if priorities else ()) \
        + (("is_beta",) if is_beta else ()) + (("all_obs",) if all_obs else ())

    class Buffer:
        def __init__(self):
            self.held, self.samples = [], 0

        def __len__(self):
            return len(self.held)

        def add(self, trajectory, w=1.):
            self.held.append(trajectory)
            log.append(("add", trajectory, w))

        def sample(self, **kw):
            assert set(kw) <= set(takes), kw
            log.append(("sample", dict(kw)))
            self.samples += 1
            out = (("batch", self.samples),) + ((("indices", self.samples),) if kw.get("with_indices") else ()) \
                + ((("isw", self.samples),) if kw.get("is_beta") is not None else ())
            return out if len(out) > 1 else out[0]

    P = inspect.Parameter
    Buffer.sample.__signature__ = inspect.Signature([P(n, P.POSITIONAL_OR_KEYWORD, default=None)
                                                     for n in ("self",) + takes])

    def _add_many(self, trajectories, weights):
        self.held.extend(trajectories)
        log.append(("add_many", list(trajectories), list(weights)))

    def _update_priorities(self, indices, priorities, **kw):
        log.append(("update_priorities", indices, priorities, kw))

    def _stalest(self, count):
        log.append(("stalest", count))
        return list(range(100, 100 + min(count, len(self))))

    def _reanalyse(self, model, key, n, gamma, alpha, **kw):
        log.append(("reanalyse", model, _k(key), n, gamma, alpha, kw))

    def _add_steps(self, ring, episodes, n, gamma, alpha=None, weight="mean"):
        episodes = [tuple(int(x) for x in e) for e in episodes]
        log.append(("add_steps", ring, episodes, n, gamma, alpha, weight))
        first = len(self.held)
        self.held.extend(episodes)
        return list(range(first, len(self.held)))

    def _stage(ring, args, stream):
        ring, args = ring._obj, args._obj
        log.append(("stage", args.row, (ring.ring_steps, ring.num_envs, ring.obs_dim, ring.num_actions), stream))
        return 0

    if add_many:
        Buffer.add_many = _add_many
    if priorities:
        Buffer.update_priorities = _update_priorities
    if reanalyse:
        Buffer.stalest, Buffer.reanalyse = _stalest, _reanalyse
    if store:
        Buffer.add_steps = _add_steps
        Buffer._device, Buffer._arena = torch.device("cpu"), SimpleNamespace(device=0)
        Buffer._L = SimpleNamespace(mzs_replay_stage=_stage)
        Buffer._check_dims = lambda self, obs_dim, A: log.append(("check_dims", obs_dim, A))
        Buffer._stream = lambda self: "stream"
    return Buffer()


def _table(ends, steps=3 * STEPS):
    """[steps, N] done flags from per-environment lists of the steps that end an episode; small integer rewards."""
    done = np.zeros((steps, N), bool)
    for env, at in enumerate(ends):
        done[list(at), env] = True
    rewards = ((np.arange(steps)[:, None] * 3 + np.arange(N)[None]) % 5 - 1).astype(np.float64)
    return done, rewards


# Environment 0: lengths 2, 1 (shorter than k_steps), 5 (over two iterations); environment 1: one that ends on the last
# step of an iteration, one of one step on the first step of the next, one of 7 over two; environment 2: none.
FIT_ENDS = ([1, 2, 7], [3, 4, 11], [])


class Env(cref.ScriptedVecEnv):
    """The scripted vector environment (observation = noise with (environment, step) in front), counting resets."""

    def __init__(self, ends=FIT_ENDS, steps=3 * STEPS, log=None, name="env", **kw):
        super().__init__(*_table(ends, steps), **kw)
        self.log, self.name = log if log is not None else [], name

    def reset(self):
        self.log.append((self.name + ".reset",))
        return super().reset()

    def step(self, actions):
        self.log.append((self.name + ".step",))
        return super().step(actions)


class DeviceEnv:
    """The device-environment protocol of muax_amd/envs.py on CPU tensors, around the scripted environment."""

    def __init__(self, host, masks=False):
        self.host, self.n, self.device, self.spec = host, host.N, torch.device("cpu"), host.spec
        if masks:
            mask = torch.zeros((host.N, 2), dtype=torch.uint8)
            self.invalid_actions_device = lambda: mask
            self.invalid_actions_of = lambda obs: None

    def reset(self):
        return self.host.reset()

    def reset_device(self):
        self.host.log.append((self.host.name + ".reset_device",))
        self.obs = torch.from_numpy(cref.ScriptedVecEnv.reset(self.host))
        return self.obs

    def step_device(self, a, r_out, done_out):
        assert a.dtype == torch.int32
        obs, r, d = self.host.step(a.numpy())
        self.obs.copy_(torch.from_numpy(obs))
        r_out.copy_(torch.from_numpy(r))
        done_out.copy_(torch.from_numpy(d.astype(np.uint8)))
        return self.obs


class GymEnv:
    """A gym-style test environment: `observation_space`, reset() -> (obs, info), the five-tuple step."""
    observation_space, spec = object(), SimpleNamespace(max_episode_steps=2)

    def __init__(self, log):
        self.log = log

    def reset(self, **kw):
        self.log.append(("gym.reset", kw))
        return np.zeros(4, np.float32), {}

    def step(self, a):
        self.log.append(("gym.step",))
        return np.ones(4, np.float32), 1.5, False, False, {}


@pytest.fixture
def log(monkeypatch):
    events = []
    monkeypatch.setattr(vector, "value_priorities", lambda model, batch: events.append(("value_priorities", batch))
                        or ("vp", batch))
    return events


def _names(log, *names):
    return [e for e in log if e[0] in names]


def _acts(log):
    """The act() calls of collection (the testers ask for neither the policy nor the value)."""
    return [e for e in log if e[0] == "act" and e[2].get("with_pi")]


def _test_acts(log):
    return [e for e in log if e[0] == "act" and not e[2].get("with_pi")]


def _test_env(log):
    """The default test environment: every first episode ends on its first step, so test_G is the mean of the first
    rewards.  (Iteration 0 is always tested: 0 % test_interval == 0.)"""
    return Env(ends=([0], [0], [0]), steps=2, log=log, name="test", max_episode_steps=3)


TEST_G = float(np.mean(_table(([0], [0], [0]), 2)[1][0]))


def _fit(log, model=None, venv=None, test_env=None, buffer=None, **kw):
    rows = []
    model = model if model is not None else Model(log)
    args = dict(n_step=N_STEP, gamma=GAMMA, alpha=ALPHA, iterations=3, steps_per_iteration=STEPS, num_simulations=7,
                k_steps=K, num_trajectory=4, num_update_per_iteration=2, test_interval=100, random_seed=5, metrics=rows)
    args.update(kw)
    out = mx.fit_vector(model, venv if venv is not None else Env(log=log),
                        test_env if test_env is not None else _test_env(log),
                        buffer=buffer if buffer is not None else make_buffer(log), **args)
    assert out is model
    assert all(r.pop("collect_s") >= 0.0 for r in rows)
    return model, rows


def _keys(seed, iterations, steps=STEPS, reanalyse_at=()):
    """The key stream of the loop: (init key, test key, per iteration the act sub-keys, the reanalysis sub-keys)."""
    key, test_key, init_key = prng.split(prng.PRNGKey(seed), 3)
    acts, reanalysed = [], []
    for it in range(iterations):
        acts.append([])
        for _ in range(steps):
            key, sub = prng.split(key)
            acts[-1].append(_k(sub))
        if it in reanalyse_at:
            key, sub = prng.split(key)
            reanalysed.append(_k(sub))
    return _k(init_key), _k(test_key), acts, reanalysed


def _episodes(model, env, calls):
    """What every call of `calls` steps finishes, by a plain loop over what the model returned and the environment's
    table: per call the `episode_trajectory` of every finished episode, environment by environment and then in time."""
    out, step0, open_start = [], 0, [0] * N
    for steps in calls:
        finished, _, open_start = cref.ring_plan(env.done[step0:step0 + steps].tolist(), open_start, step0, 1)
        out.append([])
        for e, first, T in finished:
            rows = range(first, first + T)
            obs, a, pi, v = ([model.acted[s][j][e] for s in rows] for j in range(4))
            shaped = np.stack(obs).reshape((T,) + env.noise.shape[2:])
            out[-1].append(mx.episode_trajectory(shaped, np.stack(a), [env.rewards[s, e] for s in rows], np.stack(v),
                                                 np.stack(pi), N_STEP, GAMMA, ALPHA))
        step0 += steps
    return out


def _same_trajectory(got, want):
    g, w = got.batched_transitions, want.batched_transitions
    assert len(got) == len(want)
    for name, x, y in zip(("obs", "a", "r", "done", "Rn", "v", "pi", "w"), g, w):
        x, y = np.asarray(x), np.asarray(y)
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), name
    assert np.array_equal(got.weights, want.weights) and np.array_equal(got.rewards, want.rewards)


# ------------------------------------------------------------------------------------------------------- the refusals
def _is_beta_text(buffer="Buffer"):
    return (f"fit_vector: is_beta needs a buffer whose sample() takes is_beta (DeviceReplayBuffer); "
            f"{buffer}.sample does not")


def _all_obs_text(buffer="Buffer"):
    return (f"fit_vector: all_obs needs a buffer whose sample() takes all_obs (DeviceReplayBuffer); "
            f"{buffer}.sample does not")


def _device_plan_text(device_collect, on_device):
    return (f"fit_vector: device_plan needs device_collect=True and a device environment (one with step_device); "
            f"device_collect is {device_collect} and {'DeviceEnv' if on_device else 'Env'} has "
            f"{'a' if on_device else 'no'} step_device")


PRIORITY_STEPS = "priority_steps must be None or >= 1"
WEIGHT = "trajectory_weight must be 'mean' or 'sum'"
IS_BETA_RANGE = "fit_vector: is_beta must be None, a number in 0..1 or a callable"
STOCHASTIC_STEPS = ("fit_vector: priority_update with priority_steps needs MuZero.unroll_values, which is not built for "
                    "an SMZNetwork (a stochastic model); use priority_steps=None (value_priorities)")
NEEDS_DEVICE_COLLECT = ("fit_vector: DeviceEnv is a device environment (it has step_device) and needs "
                        "device_collect=True; device_collect is False")
NEEDS_STORE = "fit_vector: device_collect needs a buffer with the device store (DeviceReplayBuffer); Buffer has none"
DEVICE_ENV_NEEDS_STORE = ("fit_vector: DeviceEnv is a device environment (it has step_device) and needs a buffer with "
                          "the device store, add_steps (DeviceReplayBuffer); Buffer has none")
N_AT_LEAST_1 = "n must be at least 1"
PLAN_MIN_LENGTH = "DeviceVectorCollector: device_plan needs min_length >= 1"


class Case:
    """One call of fit_vector that is to be refused: the keyword arguments, the buffer's capabilities, the kind of
    environment and of model.  A refusal's trigger edits it; two triggers edit it one after the other."""

    def __init__(self):
        self.kw, self.caps, self.on_device, self.stochastic = {}, dict(store=True), False, False

    def raises(self, log):
        model = Model(log, stochastic=self.stochastic)
        venv = DeviceEnv(Env(log=log)) if self.on_device else Env(log=log)
        with pytest.raises(ValueError) as ei:
            mx.fit_vector(model, venv, _test_env(log), buffer=make_buffer(log, **self.caps), **self.kw)
        assert type(ei.value) is ValueError and log == []  # before model.init, reset() and every buffer call
        return str(ei.value)


def _t_priority_steps(c):
    c.kw["priority_steps"] = 0


def _t_weight(c):
    c.kw["trajectory_weight"] = "max"


def _t_device_plan(c):
    c.kw["device_plan"] = True


def _t_is_beta_range(c):
    c.kw["is_beta"] = 1.5


def _t_is_beta_needs(c):
    c.caps["is_beta"] = False
    c.kw.setdefault("is_beta", 0.5)


def _t_all_obs(c):
    c.caps["all_obs"] = False
    c.kw["all_obs"] = True


def _t_stochastic_steps(c):
    c.stochastic = True
    c.kw["priority_update"] = True
    c.kw.setdefault("priority_steps", 2)


def _t_needs_device_collect(c):
    c.on_device = True


def _t_needs_store(c):
    c.kw["device_collect"] = True
    c.caps["store"] = False


def _t_collector(c):
    c.kw["device_collect"] = True
    c.kw["n_step"] = 0


# The ladder, first refusal first.  (Triggers that set a value outright stand before those that only default it.)
LADDER = [("priority_steps", _t_priority_steps, lambda c: PRIORITY_STEPS),
          ("trajectory_weight", _t_weight, lambda c: WEIGHT),
          ("device_plan", _t_device_plan, lambda c: _device_plan_text(bool(c.kw.get("device_collect")), c.on_device)),
          ("is_beta_needs", _t_is_beta_needs, lambda c: _is_beta_text()),
          ("is_beta_range", _t_is_beta_range, lambda c: IS_BETA_RANGE),
          ("all_obs", _t_all_obs, lambda c: _all_obs_text()),
          ("stochastic_steps", _t_stochastic_steps, lambda c: STOCHASTIC_STEPS),
          ("needs_device_collect", _t_needs_device_collect, lambda c: NEEDS_DEVICE_COLLECT),
          ("needs_store", _t_needs_store, lambda c: NEEDS_STORE),
          ("collector", _t_collector, lambda c: N_AT_LEAST_1)]
RUNG = {name: i for i, (name, _, _) in enumerate(LADDER)}
SETS_OUTRIGHT = ("priority_steps", "is_beta_range")
# pairs that cannot apply to one call: a device environment without device_collect against anything that turns it on,
# and a buffer without the store against the collector that needs one
EXCLUSIVE = [{"needs_device_collect", "needs_store"}, {"needs_device_collect", "collector"}, {"needs_store", "collector"}]


@pytest.mark.parametrize("name", list(RUNG))
def test_every_refusal_alone(log, name):
    c = Case()
    _, trigger, text = LADDER[RUNG[name]]
    trigger(c)
    assert c.raises(log) == text(c)


@pytest.mark.parametrize("first,second", [(a, b) for a, b in itertools.combinations(RUNG, 2) if {a, b} not in EXCLUSIVE])
def test_of_two_refusals_the_earlier_rung_wins(log, first, second):
    c = Case()
    for name in sorted((first, second), key=lambda n: (n not in SETS_OUTRIGHT, RUNG[n])):
        LADDER[RUNG[name]][1](c)
    assert c.raises(log) == LADDER[RUNG[first]][2](c)


def test_the_refusals_other_texts(log):
    # device_plan: every way of lacking one of its two needs
    for device_collect, on_device in ((False, False), (True, False), (False, True)):
        c = Case()
        c.kw.update(device_plan=True, device_collect=device_collect)
        c.on_device = on_device
        assert c.raises(log) == _device_plan_text(device_collect, on_device)
    # a device environment and a buffer without the store
    c = Case()
    c.kw["device_collect"], c.on_device, c.caps["store"] = True, True, False
    assert c.raises(log) == DEVICE_ENV_NEEDS_STORE
    # the default buffer is the host one
    for kw, text in ((dict(is_beta=0.5), _is_beta_text("TrajectoryReplayBuffer")),
                     (dict(all_obs=True), _all_obs_text("TrajectoryReplayBuffer")),
                     (dict(device_collect=True), NEEDS_STORE.replace("Buffer has", "TrajectoryReplayBuffer has"))):
        with pytest.raises(ValueError) as ei:
            mx.fit_vector(Model(log), Env(log=log), None, **kw)
        assert str(ei.value) == text and log == []
    # the collector's own refusal of the plan comes last of all
    c = Case()
    c.kw.update(device_collect=True, device_plan=True, k_steps=0)
    c.on_device = True
    assert c.raises(log) == PLAN_MIN_LENGTH
    # what is no refusal: the ends of is_beta's range, a callable, priority_steps where nothing is written back
    for kw in (dict(is_beta=0.0), dict(is_beta=1.0), dict(is_beta=lambda **k: 7.0),
               dict(priority_steps=2, model=Model(log, stochastic=True)),
               dict(priority_update=True, priority_steps=2, model=Model(log, stochastic=True),
                    buffer=make_buffer(log, priorities=False)),
               dict(priority_update=True, priority_steps=2, model=Model(log, stochastic=True, unrolls=True))):
        _fit(log, iterations=1, num_update_per_iteration=1, **kw)


# ----------------------------------------------------------------------------------- sample / update / write-back grid
def _expected_updates(caps, stochastic, priority_update, priority_steps, is_beta, all_obs, updates, alpha, weight):
    prioritise = priority_update and caps["priorities"]
    kw = dict(SAMPLE_BASE)
    if prioritise:
        kw["with_indices"] = True
    if (stochastic and caps["all_obs"]) if all_obs is None else all_obs:
        kw["all_obs"] = True
    out = []
    for n in range(1, updates + 1):
        if is_beta is not None:
            kw["is_beta"] = float(is_beta(training_steps=n - 1, max_training_steps=10000)) if callable(is_beta) else is_beta
        batch = ("batch", n)
        out += [("sample", dict(kw)), ("update", batch, {"sample_weight": ("isw", n)} if is_beta is not None else {})]
        if prioritise:
            if priority_steps is None:
                prio = ("vp", batch)
                out.append(("value_priorities", batch))
            else:
                prio = ("unrolled", batch, min(priority_steps, K))
                out.append(("unroll_values", batch, min(priority_steps, K), "auto"))
            out.append(("update_priorities", ("indices", n), prio, dict(alpha=1.0 if alpha is None else alpha,
                                                                          weight=weight)))
    return out


def _beta_schedule(training_steps, max_training_steps):
    assert max_training_steps == 10000
    return 0.25 + 0.125 * training_steps


BUFFERS = {"every": {}, "no_priorities": dict(priorities=False), "no_is_beta": dict(is_beta=False),
           "no_all_obs": dict(all_obs=False), "bare": dict(priorities=False, is_beta=False, all_obs=False,
                                                            add_many=False, reanalyse=False)}


@pytest.mark.parametrize("stochastic,unrolls", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("buffer", list(BUFFERS))
def test_sample_update_and_write_back_for_every_combination(log, buffer, stochastic, unrolls):
    caps = dict(priorities=True, is_beta=True, all_obs=True)
    caps.update(BUFFERS[buffer])
    ran = 0
    for priority_update, priority_steps, is_beta, all_obs, (alpha, weight) in itertools.product(
            (False, True), (None, 1, 5), (None, 0.5, _beta_schedule), (None, True, False), ((ALPHA, "mean"), (None, "sum"))):
        what = dict(priority_update=priority_update, priority_steps=priority_steps, is_beta=is_beta, all_obs=all_obs)
        refused = (_is_beta_text() if is_beta is not None and not caps["is_beta"] else
                   _all_obs_text() if all_obs and not caps["all_obs"] else
                   STOCHASTIC_STEPS if priority_update and caps["priorities"] and priority_steps is not None
                   and stochastic and not unrolls else None)
        del log[:]
        model = Model(log, stochastic=stochastic, unrolls=unrolls)
        kw = dict(model=model, buffer=make_buffer(log, **caps), iterations=1, num_update_per_iteration=3, alpha=alpha,
                  trajectory_weight=weight, **what)
        if refused:
            with pytest.raises(ValueError) as ei:
                _fit(log, **kw)
            assert str(ei.value) == refused and log == [], what
            continue
        _, rows = _fit(log, **kw)
        got = _names(log, "sample", "update", "value_priorities", "unroll_values", "update_priorities")
        assert got == _expected_updates(caps, stochastic, priority_update, priority_steps, is_beta, all_obs, 3, alpha,
                                        weight), what
        assert rows[0]["loss"] == (1 + 2 + 3) / 3 and rows[0]["training_step"] == 3
        ran += 1
    assert ran > 0


def test_the_priority_functions_are_looked_up_in_the_module_at_call_time(log, monkeypatch):
    monkeypatch.setattr(vector, "unroll_value_priorities", lambda model, batch, kp: ("mine", batch, kp))
    _fit(log, iterations=1, priority_update=True, priority_steps=7)
    assert [e[2] for e in _names(log, "update_priorities")] == [("mine", ("batch", 1), K), ("mine", ("batch", 2), K)]
    assert _names(log, "unroll_values", "value_priorities") == []


# ------------------------------------------------------------------------------- the loop: collect, store, keys, rows
def _expected_rows(env, per_iteration, updates=2, tested=None):
    tested = {0: TEST_G} if tested is None else tested
    rows, step0, open_start, trained = [], 0, [0] * N, 0
    for it in range(len(per_iteration)):
        finished, _, open_start = cref.ring_plan(env.done[step0:step0 + STEPS].tolist(), open_start, step0, 1)
        G = [float(np.sum(env.rewards[first:first + T, e])) for e, first, T in finished]
        row = {"iteration": it, "env_steps": STEPS * N, "episodes": len(finished),
               "G": float(np.mean(G)) if G else float("nan")}
        if per_iteration[it]:  # the buffer holds something: the updates run
            row["loss"] = sum(range(trained + 1, trained + updates + 1)) / updates
            trained += updates
        row["training_step"] = trained
        if it in tested:
            row["test_G"] = tested[it]
        rows.append(row)
        step0 += STEPS
    return rows


def _same_rows(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert list(g) == [k for k in ("iteration", "env_steps", "episodes", "G", "loss", "training_step", "test_G")
                           if k in w]
        assert all(g[k] == w[k] or (k == "G" and math.isnan(g[k]) and math.isnan(w[k])) for k in w), (g, w)


ACT_KW = dict(with_pi=True, with_value=True, obs_from_batch=True, num_simulations=7, temperature=1.0)


@pytest.mark.parametrize("weight", ["mean", "sum"])
@pytest.mark.parametrize("add_many", [True, False])
def test_the_host_route_over_three_iterations(log, add_many, weight):
    env = Env(log=log)
    model, rows = _fit(log, venv=env, buffer=make_buffer(log, add_many=add_many), trajectory_weight=weight)
    init_key, _, act_keys, _ = _keys(5, 3)
    # model.init first, on the first observation of the first environment; the collector resets again
    first = cref.ScriptedVecEnv.reset(Env())[:1].astype(float)
    assert log[:3] == [("env.reset",), ("init", init_key, first.tolist()), ("env.reset",)]
    assert [e[1:] for e in _acts(log)] == [(k, ACT_KW) for it in act_keys for k in it]
    # per iteration: the steps, then the finished episodes of at least k_steps into the buffer, then the updates
    want = _episodes(model, env, [STEPS] * 3)
    assert [[len(t) for t in call] for call in want] == [[2, 1, 4], [5, 1], [7]]
    stored = _names(log, "add_many", "add")
    kept = [[t for t in call if len(t) >= K] for call in want]
    weights = [[t.weights.mean() if weight == "mean" else t.weights.sum() for t in call] for call in kept]
    if add_many:
        assert [e[0] for e in stored] == ["add_many"] * 3
        got, got_w = [e[1] for e in stored], [e[2] for e in stored]
    else:
        assert [e[0] for e in stored] == ["add"] * 4
        flat = iter(stored)
        got = [[next(flat)[1] for _ in call] for call in kept]
        flat = iter(stored)
        got_w = [[next(flat)[2] for _ in call] for call in kept]
    assert got_w == weights
    for g_call, w_call in zip(got, kept):
        assert len(g_call) == len(w_call)
        for g, w in zip(g_call, w_call):
            _same_trajectory(g, w)
    order = [e[0] for e in log if e[0] in ("add_many", "add", "sample", "update") or e in _acts(log)]
    if add_many:
        assert order == (["act"] * STEPS + ["add_many"] + ["sample", "update"] * 2) * 3
    else:
        assert order == (["act"] * STEPS + ["add"] * 2 + ["sample", "update"] * 2
                         + (["act"] * STEPS + ["add"] + ["sample", "update"] * 2) * 2)
    _same_rows(rows, _expected_rows(env, [True] * 3))
    assert [e[1] for e in _names(log, "sample")] == [SAMPLE_BASE] * 6
    assert _names(log, "reanalyse", "stalest", "update_priorities") == []
    assert _names(log, "test.reset") == [("test.reset",)]  # (iteration 0 alone is tested under test_interval=100)


def test_nothing_finished_is_a_nan_row_and_no_update(log):
    env = Env(ends=([], [], []), log=log)
    _, rows = _fit(log, venv=env, iterations=2)
    _same_rows(rows, _expected_rows(env, [False, False]))
    assert math.isnan(rows[0]["G"]) and "loss" not in rows[0] and rows[1]["training_step"] == 0
    assert _names(log, "sample", "update", "add") == [] and [e[1:] for e in _names(log, "add_many")] == [([], [])] * 2
    # episodes that finish but are all shorter than k_steps: counted, their returns in G, nothing stored or trained
    del log[:]
    env = Env(ends=([0, 1, 2, 3], [], []), log=log)
    _, rows = _fit(log, venv=env, iterations=1)
    _same_rows(rows, _expected_rows(env, [False]))
    assert rows[0]["episodes"] == 4 and rows[0]["G"] == float(np.mean(env.rewards[:4, 0]))


def test_reanalysis_takes_one_more_split_and_leaves_the_other_keys_alone(log):
    for masks in (False, True):
        del log[:]
        env = DeviceEnv(Env(log=log), masks=masks)
        model, rows = _fit(log, venv=env, buffer=make_buffer(log, store=True), device_collect=True, reanalyse_every=2,
                           reanalyse_episodes=None, trajectory_weight="sum")
        _, _, act_keys, reanalysed = _keys(5, 3, reanalyse_at=(1,))
        assert [e[1] for e in _acts(log)] == [k for it in act_keys for k in it]
        (_, count), = _names(log, "stalest")
        (_, m, key, n, gamma, alpha, kw), = _names(log, "reanalyse")
        assert count == 3 and m is model and (key, n, gamma, alpha) == (reanalysed[0], N_STEP, GAMMA, ALPHA)
        want = dict(weight="sum", serials=[100, 101, 102], num_simulations=7)
        if masks:
            want["mask_fn"] = env.invalid_actions_of
        assert kw == want
        names = [e[0] for e in log if e[0] in ("add_steps", "stalest", "reanalyse", "sample")]
        assert names == ["add_steps", "sample", "sample", "add_steps", "stalest", "reanalyse", "sample", "sample",
                         "add_steps", "sample", "sample"]
        # the collector hands the environment's own mask to every act(), the same object
        for e in _acts(log):
            assert ("invalid_actions" in e[2]) == masks
            assert not masks or e[2]["invalid_actions"] is env.invalid_actions_device()
    # reanalyse_episodes bounds the count; a buffer without reanalyse, or reanalyse_every=0, splits nothing
    del log[:]
    _fit(log, reanalyse_every=1, reanalyse_episodes=2)
    assert _names(log, "stalest") == [("stalest", 2)] * 3
    assert [e[2] for e in _names(log, "reanalyse")] == _keys(5, 3, reanalyse_at=(0, 1, 2))[3]
    for kw in (dict(reanalyse_every=1, buffer=make_buffer(log, reanalyse=False)), dict(reanalyse_every=0)):
        del log[:]
        _fit(log, **kw)
        assert [e[1] for e in _acts(log)] == [k for it in _keys(5, 3)[2] for k in it]
        assert _names(log, "reanalyse", "stalest") == []
    # nothing held yet: no reanalysis and no split
    del log[:]
    _fit(log, venv=Env(ends=([], [], [7]), log=log), reanalyse_every=1, iterations=3)
    assert [e[2] for e in _names(log, "reanalyse")] == _keys(5, 3, reanalyse_at=(1, 2))[3][:2]
    assert [e[1] for e in _acts(log)] == [k for it in _keys(5, 3, reanalyse_at=(1, 2))[2] for k in it]


def test_the_stop_the_temperature_and_the_test_cadence(log):
    env = Env(log=log)
    _, rows = _fit(log, venv=env, iterations=6, max_training_steps=8, test_interval=2)
    assert len(rows) == 4  # training_step reaches 8 after the fourth iteration
    assert [r["training_step"] for r in rows] == [2, 4, 6, 8]
    assert [r.get("test_G") for r in rows] == [TEST_G, None, TEST_G, None]
    # the default schedule: 1.0 below half of max_training_steps, 0.5 below three quarters, then 0.25
    temps = [e[2]["temperature"] for e in _acts(log)]
    assert temps == [1.0] * 2 * STEPS + [0.5] * STEPS + [0.25] * STEPS
    del log[:]
    seen = []
    _fit(log, iterations=2, temperature_fn=lambda max_training_steps, training_steps:
         seen.append((max_training_steps, training_steps)) or 0.75)
    assert seen == [(10000, 0), (10000, 2)]
    assert {e[2]["temperature"] for e in _acts(log)} == {0.75}


# --------------------------------------------------------------------------------------------------------- the tester
def test_a_vector_test_env_is_evaluated_by_test_vector(log):
    test_env = Env(ends=([1], [0], [2]), steps=6, log=log, name="test", max_episode_steps=5)
    _, rows = _fit(log, test_env=test_env, iterations=1, test_interval=1)
    _, test_key, _, _ = _keys(5, 1)
    tests = _test_acts(log)
    key, want = test_key, []
    for _ in range(3):  # all three first episodes are over after the third step
        key, sub = prng.split(key)
        want.append((_k(sub), dict(obs_from_batch=True, num_simulations=7, temperature=0.)))
    assert [e[1:] for e in tests] == want
    r = test_env.rewards
    assert rows[0]["test_G"] == float(np.mean([r[0, 0] + r[1, 0], r[0, 1], r[0, 2] + r[1, 2] + r[2, 2]]))
    assert _names(log, "test.reset") == [("test.reset",)] and len(_names(log, "test.step")) == 3


def test_a_device_test_env_is_evaluated_by_test_vector_device(log):
    for masks in (False, True):
        del log[:]
        test_env = DeviceEnv(Env(ends=([1], [0], [2]), steps=6, log=log, name="test", max_episode_steps=5), masks=masks)
        _, rows = _fit(log, test_env=test_env, iterations=1, test_interval=1)
        tests = _test_acts(log)
        key, want = _keys(5, 1)[1], []
        for _ in range(5):  # the "all finished" check comes after every 16th step only: max_episode_steps steps
            key, sub = prng.split(key)
            want.append(_k(sub))
        assert [e[1] for e in tests] == want
        for e in tests:
            assert {k: v for k, v in e[2].items() if k != "invalid_actions"} == dict(
                obs_from_batch=True, device_outputs=True, num_simulations=7, temperature=0.)
            assert ("invalid_actions" in e[2]) == masks
            assert not masks or e[2]["invalid_actions"] is test_env.invalid_actions_device()
        r = test_env.host.rewards
        assert rows[0]["test_G"] == float(np.mean([r[0, 0] + r[1, 0], r[0, 1], r[0, 2] + r[1, 2] + r[2, 2]]))
        assert _names(log, "test.reset_device") == [("test.reset_device",)] and _names(log, "test.reset") == []
    with pytest.raises(ValueError) as ei:
        mx.test_vector_device(Model(log), Env(), prng.PRNGKey(0), 3)
    assert str(ei.value) == ("test_vector_device needs a device environment (one with step_device); Env has none: "
                             "use test_vector")


def test_a_gym_style_test_env_is_evaluated_by_the_reference_test(log):
    _, rows = _fit(log, test_env=GymEnv(log), iterations=1, test_interval=1, num_test_episodes=3)
    tests = _test_acts(log)
    key, want = _keys(5, 1)[1], []
    for _ in range(3 * 2):
        key, sub = prng.split(key)
        want.append((_k(sub), dict(num_simulations=7, temperature=0.)))
    assert [e[1:] for e in tests] == want and rows[0]["test_G"] == 3.0
    assert _names(log, "gym.reset") == [("gym.reset", {})] * 3 and len(_names(log, "gym.step")) == 6


def test_test_vector_passes_a_host_environments_mask(log):
    env = Env(ends=([0], [0], [0]), steps=2)
    mask = np.zeros((N, 2), np.uint8)
    env.invalid_actions = lambda: mask
    mx.test_vector(Model(log), env, prng.PRNGKey(3), 4)
    (_, _, kw), = _test_acts(log)
    assert kw["invalid_actions"] is mask and set(kw) == {"obs_from_batch", "num_simulations", "temperature",
                                                         "invalid_actions"}


# ------------------------------------------------------------------------------------------------- the device route
@pytest.mark.parametrize("on_device", [False, True])
def test_the_device_route_hands_out_the_host_routes_rows(log, on_device):
    _, host_rows = _fit(log)
    host_acts = [e[1] for e in _acts(log)]
    del log[:]
    env = Env(log=log)
    venv = DeviceEnv(env) if on_device else env
    _, rows = _fit(log, venv=venv, buffer=make_buffer(log, store=True), device_collect=True, trajectory_weight="sum")
    assert rows == host_rows and [e[1] for e in _acts(log)] == host_acts
    for e in _acts(log):
        assert e[2] == dict(ACT_KW, device_outputs=True)
    # the episodes of at least k_steps go into the store in one call per iteration, whatever else the buffer offers
    S = env.spec.max_episode_steps + STEPS
    stores = _names(log, "add_steps")
    assert [e[2] for e in stores] == [[(0, 0, 2), (1, 0, 4)], [(0, 3, 5)], [(1, 5, 7)]]
    assert all(e[3:] == (N_STEP, GAMMA, ALPHA, "sum") for e in stores) and _names(log, "add_many", "add") == []
    assert [e[1] for e in _names(log, "stage")] == [s % S for s in range(3 * STEPS)]
    assert (_names(log, "env.reset_device") == [("env.reset_device",)]) == on_device
    assert len(_names(log, "env.reset")) == (1 if on_device else 2)  # (model.init's sample; the collector's own)


# ----------------------------------------------------------------------------------------------------- VectorCollector
def test_vector_collector_cuts_the_stream_into_the_per_environment_episodes(log):
    """Three calls of four steps.  Environment 0: an episode over all three calls; environment 1: one that ends on the
    last step of the first call, one of one step on the first step of the second, one on the last step of the third;
    environment 2: no episode ends."""
    env = Env(ends=([9], [3, 4, 11], []), obs_dim=5)
    model, col, key = Model(log), mx.VectorCollector(env, N_STEP, GAMMA, ALPHA), prng.PRNGKey(9)
    got = []
    for _ in range(3):
        trajs, key2, count = col.collect(model, key, STEPS, num_simulations=7, temperature=0.5, extra=1)
        want_key = key
        for _ in range(STEPS):
            want_key, _ = prng.split(want_key)
        assert _k(key2) == _k(want_key) and count == STEPS * N
        key = key2
        got.append(trajs)
    assert all(e[2] == dict(ACT_KW, temperature=0.5, extra=1) for e in _acts(log))
    want = _episodes(model, env, [STEPS] * 3)
    assert [[len(t) for t in call] for call in want] == [[4], [1], [10, 7]]
    for g_call, w_call in zip(got, want):
        assert len(g_call) == len(w_call)
        for g, w in zip(g_call, w_call):
            _same_trajectory(g, w)
    # alpha None: every priority weight is one
    env = Env(ends=([9], [3, 4, 11], []))
    model, col = Model(log), mx.VectorCollector(env, N_STEP, GAMMA, None)
    trajs, _, _ = col.collect(model, prng.PRNGKey(9), STEPS)
    assert [t.weights.tolist() for t in trajs] == [[1.0] * 4]


# ----------------------------------------------------------------------------------------------- DeviceVectorCollector
def test_device_vector_collector_with_a_host_environment_and_a_ring_that_wraps(log):
    """ring_steps = 5, three calls of three steps: the second call's rows wrap past the ring's end.  What is staged where,
    the episode list handed to add_steps (ring_plan's, first row modulo the ring) and the rows handed out (the host
    collector's lengths and returns, a serial for every episode of at least min_length steps)."""
    S, steps, ends = 5, 3, ([1, 4, 7], [2, 3, 8], [0, 5, 6])
    env = Env(ends=ends, steps=9, log=log)
    buf = make_buffer(log, store=True)
    col = mx.DeviceVectorCollector(env, buf, N_STEP, GAMMA, ALPHA, weight="sum", min_length=2, ring_steps=S)
    host = mx.VectorCollector(Env(ends=ends, steps=9), N_STEP, GAMMA, ALPHA)
    model, key, step0, open_start, serial = Model(log), prng.PRNGKey(2), 0, [0] * N, 0
    for call in range(3):
        del log[:]
        rows, key2, count = col.collect(model, key, steps, num_simulations=7, temperature=0.5)
        trajs, host_key, host_count = host.collect(Model([]), key, steps, num_simulations=7, temperature=0.5)
        assert _k(key2) == _k(host_key) and count == host_count == steps * N
        key = key2
        want_rows = []
        for t in trajs:
            want_rows.append((len(t), float(np.sum(t.rewards)), serial if len(t) >= 2 else None))
            serial += len(t) >= 2
        assert rows == want_rows and any(r[2] is None for r in want_rows)
        finished, dropped, open_start = cref.ring_plan(env.done[step0:step0 + steps].tolist(), open_start, step0, 2)
        (_, ring, episodes, n, gamma, alpha, weight), = _names(log, "add_steps")
        assert episodes == [(e, first % S, T) for e, first, T in finished] and dropped
        assert (n, gamma, alpha, weight) == (N_STEP, GAMMA, ALPHA, "sum") and ring is col._ring
        assert _names(log, "stage") == [("stage", (step0 + i) % S, (S, N, 4, 2), "stream") for i in range(steps)]
        assert all(e[2] == dict(ACT_KW, temperature=0.5, device_outputs=True) for e in _acts(log))
        # the collector's state has moved on before add_steps is called
        assert [e[0] for e in log if e[0] in ("stage", "add_steps")] == ["stage"] * steps + ["add_steps"]
        step0 += steps
        # the call's rewards are in the ring's `r` rows
        for s in range(step0 - steps, step0):
            assert np.array_equal(col._fields["r"][s % S].numpy(), env.rewards[s])
    assert _names(log, "check_dims") == [] and col._step0 == 9  # (allocated once, in the first call)
    # the ring-fit refusal, before anything is stepped
    del log[:]
    with pytest.raises(ValueError) as ei:
        col.collect(model, key, 5)
    assert str(ei.value) == "collect: an open episode of 2 steps plus 5 more does not fit the ring of 5 steps (ring_steps)"
    with pytest.raises(ValueError) as ei:
        col.collect(model, key, 0)
    assert str(ei.value) == "collect: steps must be at least 1" and log == []


def test_device_vector_collectors_own_refusals(log):
    env, store = Env(), make_buffer(log, store=True)
    for args, kw, text in (
            ((env, make_buffer(log), 3, 0.9), {}, "DeviceVectorCollector needs a buffer with the device store "
                                                   "(DeviceReplayBuffer); Buffer has none"),
            ((env, store, 3, 0.9), dict(weight="max"), "weight must be 'mean' or 'sum'"),
            ((env, store, 0, 0.9), {}, N_AT_LEAST_1),
            ((env, store, 3, 0.9), dict(ring_steps=0), "ring_steps must be positive"),
            ((env, store, 3, 0.9), dict(device_plan=True),
             "DeviceVectorCollector: device_plan needs a device environment (one with step_device, e.g. DeviceCartPole): "
             "the plan kernel reads the rewards and flags the environment wrote on the device; Env has no step_device"),
            ((DeviceEnv(env), store, 3, 0.9), dict(device_plan=True, min_length=0), PLAN_MIN_LENGTH)):
        with pytest.raises(ValueError) as ei:
            mx.DeviceVectorCollector(*args, **kw)
        assert str(ei.value) == text
    # ring_steps defaults to max_episode_steps plus the first call's steps
    col = mx.DeviceVectorCollector(Env(max_episode_steps=6), store, 3, 0.9)
    col.collect(Model(log), prng.PRNGKey(0), 3)
    assert col.ring_steps == 9
