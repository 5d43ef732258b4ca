"""CPU tests of MuZero.act()'s routing (muax_amd/model.py): which library calls an act() makes, in which order and with
which arguments, on every route -- the fused host round trip, the fused device call, the on-demand build, the wide and
generic opt-ins, the step-wise policies, the stochastic callables route -- and how the results are delivered.  No GPU and
no library: `muax_amd.model.MuZeroSearch` is a fake that records every call and can be told to decline, `_dirichlet` and
`_jit` are recorders, and the policy classes' `__call__` is a recorder (the instance keeps its exact type, which the
routing looks at).  The GPU suites check what the routes compute; this file pins the routing itself.

`_lib.check`'s mapping of status codes and library messages onto exception classes is tested at the end."""
import warnings

import numpy as np
import pytest
import torch

import muax_amd as mx
from muax_amd import _jit, _lib
from muax_amd import model as model_mod
from muax_amd.search import PolicyOutput

F32 = np.float32
B = 3
NO_INSTANCE = "mzs_act_mlp: no fused kernel instance for this (A, E, F, S)"
# the typed refusals and the route names of the non-stochastic policies arrived together
TYPED = hasattr(_lib, "Unsupported")


class World:
    """What one test's fakes share: the log of calls, how many fused calls still decline, and the error they raise."""

    def __init__(self):
        self.events = []
        self.handles = []         # every fake handle constructed
        self.decline = 0
        self.error = None
        self.ensure = False       # what _jit.ensure_instance answers
        self.log_tail = ""        # what _jit.build_log_tail answers

    def names(self, start=0):
        return [e[0] for e in self.events[start:]]

    def of(self, name):
        return [e for e in self.events if e[0] == name]


class FakeSearch:
    world = None

    def __init__(self, batch, cfg, device=None):
        self.batch, self.cfg, self.device = batch, cfg, device
        A = cfg.num_actions
        self._out = torch.zeros(batch * (2 + A))
        self.root_value = torch.full((batch,), 0.5)
        self.world.events.append(("create", batch, cfg))
        self.world.handles.append(self)

    def _serve(self, name, kw):
        w = self.world
        w.events.append((name, kw))
        if w.decline > 0:
            w.decline -= 1
            raise w.error or getattr(_lib, "NoKernelInstance", ValueError)(NO_INSTANCE)

    def set_mlp_weights(self, weights, obs_dim, support_size=10, discount=0.99, recurrent_pred_on="child"):
        assert len(weights) == 18 and not any(v.requires_grad for v in weights.values())
        self.world.events.append(("set_mlp_weights", obs_dim, support_size, discount, recurrent_pred_on))

    def allow_wide(self, allow=True, gumbel=False):
        self.world.events.append(("allow_wide", allow, gumbel))

    def allow_generic(self, allow=True):
        self.world.events.append(("allow_generic", allow))

    def act_mlp(self, obs, key, **kw):
        self._serve("act_mlp", dict(kw, obs=obs, key=key))
        A = self.cfg.num_actions
        self.dev = PolicyOutput(torch.zeros(self.batch, dtype=torch.int32), torch.full((self.batch, A), 1.0 / A), None)
        return self.dev

    def act_mlp_host(self, obs, key, **kw):
        self._serve("act_mlp_host", dict(kw, obs=obs, key=key))
        A = self.cfg.num_actions
        self.host = (np.zeros(self.batch, np.int32), np.full((self.batch, A), 1.0 / A, F32), np.full(self.batch, 0.5, F32))
        return self.host

    def outputs_to_host(self):
        self.world.events.append(("outputs_to_host",))
        A = self.cfg.num_actions
        self.host = (np.ones(self.batch, np.int32), np.full((self.batch, A), 1.0 / A, F32), np.full(self.batch, 0.25, F32))
        return self.host

    def outputs_clone(self):
        self.world.events.append(("outputs_clone",))
        A = self.cfg.num_actions
        self.clone = (torch.ones(self.batch, dtype=torch.int32), torch.full((self.batch, A), 1.0 / A),
                      torch.full((self.batch,), 0.25))
        return self.clone


@pytest.fixture
def world(monkeypatch):
    w = World()
    monkeypatch.setattr(model_mod, "MuZeroSearch", type("Fake", (FakeSearch,), {"world": w}))
    monkeypatch.setattr(model_mod.MuZero, "_warned_stepwise", set())
    for name in ("MUAX_AMD_WIDE", "MUAX_AMD_GENERIC"):
        monkeypatch.delenv(name, raising=False)

    def dirichlet(key_words, alpha, shape, device, global_batch=None, root_offset=0):
        w.events.append(("dirichlet", tuple(int(k) for k in key_words), alpha, tuple(shape), global_batch, root_offset))
        w.noise = torch.full(tuple(shape), 1.0 / shape[1])
        return w.noise

    def ensure_instance(A, E, F, S, verbose=False, gumbel=True, extra_flags=()):
        w.events.append(("ensure_instance", A, E, F, S, gumbel))
        return w.ensure

    monkeypatch.setattr(model_mod, "_dirichlet", dirichlet)
    monkeypatch.setattr(_jit, "ensure_instance", ensure_instance)
    monkeypatch.setattr(_jit, "build_log_tail", lambda lines=6: w.log_tail)
    monkeypatch.setattr(_jit, "last_build_log", "/nowhere/mzfused_test.log")

    def policy_call(self, params, rng_key, root, *fns, **kwargs):
        w.events.append(("policy", type(self).__name__, params, rng_key, root, fns, kwargs))
        Bq, A = root[0].shape
        return PolicyOutput(torch.arange(Bq, dtype=torch.int32) % A, torch.full((Bq, A), 1.0 / A), None)

    w.policy_call = policy_call
    for cls in (mx.MuZeroPolicy, mx.GumbelMuZeroPolicy, mx.StochasticMuZeroPolicy):
        monkeypatch.setattr(cls, "__call__", policy_call)
    return w


def _model(policy="muzero", A=2, **kw):
    g = torch.Generator().manual_seed(0)
    net = mx.nn.MZNetwork(mx.nn.Representation(8, generator=g), mx.nn.Prediction(A, 21, generator=g),
                          mx.nn.Dynamic(8, A, 21, generator=g))
    m = mx.MuZero(net, device="cpu", **(kw if "policy_class" in kw else dict(kw, policy=policy)))
    m.init(0, np.zeros((1, 4)))
    return m


def _obs(seed=0, n=B):
    return np.random.default_rng(seed).uniform(-1, 1, (n, 4)).astype(F32)


def _route(m, name):
    """The route's name: new with the typed refusals for the MuZero and Gumbel policies, always there for the stochastic one."""
    if TYPED or name in ("hip_stochastic_mlp", "callables"):
        assert m._last_route == name


def _dirichlet_key(seed):
    return tuple(int(k) for k in mx.prng.split(mx.prng.as_key(seed), 3)[1])


BATCHED = dict(with_pi=True, with_value=True, obs_from_batch=True)
MUZERO_POLICY_KW = {"num_simulations", "temperature", "invalid_actions", "max_depth", "dirichlet_fraction", "dirichlet_noise",
                    "pb_c_init", "pb_c_base", "gumbel", "tiebreak", "with_tree", "graph", "graph_version", "global_batch",
                    "root_offset", "native_loop"}
GUMBEL_POLICY_KW = {"num_simulations", "invalid_actions", "max_depth", "qtransform", "max_num_considered_actions",
                    "gumbel_scale", "gumbel", "with_tree", "graph", "graph_version", "global_batch", "root_offset",
                    "native_loop"}


# ------------------------------------------------------------------------------------------------ served at once
def test_numpy_in_numpy_out_is_one_host_call_without_a_noise_draw(world):
    m = _model()
    obs = _obs()
    a, pi, v = m.act(7, obs, num_simulations=5, temperature=0.5, dirichlet_fraction=0.3, dirichlet_alpha=0.4,
                     pb_c_init=1.5, pb_c_base=100, tiebreak=False, max_depth=3, **BATCHED)
    assert world.names() == ["create", "set_mlp_weights", "act_mlp_host"]
    _, batch, cfg = world.events[0]
    assert batch == B and cfg == mx.SearchConfig(2, 5, 8, max_depth=3, tiebreak=False, pb_c_init=1.5, pb_c_base=100.0)
    assert world.events[1] == ("set_mlp_weights", 4, 10, 0.99, "child")
    kw = dict(world.events[2][1])
    assert kw.pop("obs") is not None and np.array_equal(kw.pop("key"), mx.prng.as_key(7))
    # no noise array unless the caller gave one: the C call draws it from the key
    assert kw == dict(dirichlet_noise=None, dirichlet_fraction=0.3, dirichlet_alpha=0.4, invalid_actions=None,
                      temperature=0.5)
    h, = world.handles
    assert isinstance(a, np.ndarray) and a is h.host[0] and pi is h.host[1] and v is h.host[2]
    _route(m, "fused_host")


def test_unbatched_host_call_returns_python_scalars_and_keeps_the_weights_leading_one(world):
    m = _model(A=3)
    a, pi, v = m.act(7, _obs()[0], with_pi=True, with_value=True)
    assert world.names() == ["create", "set_mlp_weights", "act_mlp_host"] and world.events[0][1] == 1
    assert world.events[2][1]["obs"].shape == (1, 4)
    assert type(a) is int and type(v) is float and v == 0.5 and pi.shape == (1, 3)
    assert m.act(7, _obs()[0]) == 0 and m.act(7, _obs()[0], with_value=True) == (0, 0.5)
    assert len(m.act(7, _obs()[0], with_pi=True)) == 2
    _route(m, "fused_host")


def test_a_given_noise_array_reaches_the_host_call(world):
    m = _model()
    noise = np.full((B, 2), 0.5, F32)
    inv = np.zeros((B, 2), np.uint8)
    m.act(7, _obs(), dirichlet_noise=noise, invalid_actions=inv, **BATCHED)
    assert world.names() == ["create", "set_mlp_weights", "act_mlp_host"]
    assert world.events[2][1]["dirichlet_noise"] is noise and world.events[2][1]["invalid_actions"] is inv


def test_device_outputs_take_the_device_call_one_noise_draw_and_clones(world):
    m = _model()
    obs = _obs()
    a, pi, v = m.act(7, obs, device_outputs=True, global_batch=8, root_offset=2, **BATCHED)
    assert world.names() == ["dirichlet", "create", "set_mlp_weights", "act_mlp", "outputs_clone"]
    assert world.events[0] == ("dirichlet", _dirichlet_key(7), 0.3, (B, 2), 8, 2)
    cfg = world.events[1][2]
    assert cfg == mx.SearchConfig(2, 5, 8, pb_c_base=19652.0, global_batch=8, root_offset=2)
    kw = dict(world.events[3][1])
    assert kw.pop("obs") is not None and np.array_equal(kw.pop("key"), mx.prng.as_key(7))
    assert kw.pop("dirichlet_noise") is world.noise
    assert kw == dict(dirichlet_fraction=0.25, invalid_actions=None, temperature=1.0, gumbel=None, with_tree=False)
    h, = world.handles
    assert a is h.clone[0] and pi is h.clone[1] and v is h.clone[2] and isinstance(a, torch.Tensor)
    _route(m, "fused")


def test_no_noise_draw_without_a_dirichlet_fraction(world):
    m = _model()
    m.act(7, _obs(), device_outputs=True, dirichlet_fraction=0.0, **BATCHED)
    assert world.names() == ["create", "set_mlp_weights", "act_mlp", "outputs_clone"]
    assert world.events[2][1]["dirichlet_noise"] is None and world.events[2][1]["dirichlet_fraction"] == 0.0


def test_tensor_observations_with_host_outputs_take_the_device_call_and_one_download(world):
    m = _model()
    obs = torch.from_numpy(_obs())
    a, pi, v = m.act(7, obs, **BATCHED)
    assert world.names() == ["dirichlet", "create", "set_mlp_weights", "act_mlp", "outputs_to_host"]
    assert world.events[3][1]["obs"] is obs  # (float32 already: handed on as it is, for act_mlp's argument cache)
    h, = world.handles
    assert a is h.host[0] and pi is h.host[1] and v is h.host[2]
    _route(m, "fused")
    # unbatched: python scalars from the download
    a, pi, v = m.act(7, obs[0], with_pi=True, with_value=True)
    assert type(a) is int and a == 1 and type(v) is float and v == 0.25 and pi.shape == (1, 2)


@pytest.mark.parametrize("drop", ["with_tree", "gumbel", "invalid_actions", "dirichlet_noise"])
def test_what_drops_the_host_round_trip(world, drop):
    """with_tree, a gumbel array, or any tensor-typed input: the device call, although observations are NumPy and the
    caller wants NumPy."""
    m = _model()
    extra = {"with_tree": dict(with_tree=True), "gumbel": dict(gumbel=np.zeros((B, 2), F32)),
             "invalid_actions": dict(invalid_actions=torch.zeros(B, 2)), "dirichlet_noise": dict(dirichlet_noise=torch.ones(B, 2))}[drop]
    out = m._plan(m.params, 7, _obs(), host_io=True, **extra)
    assert isinstance(out, tuple) and len(out) == 2 and isinstance(out[0], PolicyOutput)
    h, = world.handles
    assert out[0] is h.dev and out[1] is h.root_value
    draw = [] if drop == "dirichlet_noise" else ["dirichlet"]
    assert world.names() == draw + ["create", "set_mlp_weights", "act_mlp"]
    kw = world.events[-1][1]
    for k, v in extra.items():
        assert kw[k] is v
    _route(m, "fused")
    if drop != "with_tree":  # (act() itself has no with_tree argument)
        world.events.clear()
        a, pi, v = m.act(7, _obs(), **BATCHED, **extra)
        assert world.names() == draw + ["act_mlp", "outputs_to_host"] and isinstance(a, np.ndarray)


def test_plan_keeps_the_references_signature_and_defaults(world):
    m = _model()
    out, root_value = m._plan(m.params, 7, torch.from_numpy(_obs()), num_simulations=4, loop_fn=None)
    assert world.names() == ["dirichlet", "create", "set_mlp_weights", "act_mlp"]  # host_io defaults to False
    assert world.events[1][2].num_simulations == 4 and isinstance(out, PolicyOutput)
    m2 = mx.MuZero(m.network, device="cpu")
    with pytest.raises(ValueError, match="call init"):
        m2._plan(None, 7, _obs())


# ------------------------------------------------------------------------------------------------ the ladder on a decline
def test_a_decline_then_a_built_instance_is_served_without_opt_ins(world):
    m = _model()
    world.decline, world.ensure = 1, True
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        a, pi, v = m.act(7, _obs(), **BATCHED)
    assert world.names() == ["create", "set_mlp_weights", "act_mlp_host", "ensure_instance", "act_mlp_host"]
    assert world.of("ensure_instance") == [("ensure_instance", 2, 8, 21, 5, False)]
    assert world.events[2][1].keys() == world.events[4][1].keys() and isinstance(a, np.ndarray)
    _route(m, "fused_host")


@pytest.mark.parametrize("env,opt_ins", [({}, [("allow_wide", True, False), ("allow_generic", True)]),
                                         ({"MUAX_AMD_WIDE": "0"}, [("allow_generic", True)]),
                                         ({"MUAX_AMD_GENERIC": "0"}, [("allow_wide", True, False)])])
def test_a_decline_without_a_build_opts_in_to_the_wide_and_generic_kernels(world, monkeypatch, env, opt_ins):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = _model()
    world.decline = 1
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # (no compiler log: not a failed build, nothing to say)
        a, pi, v = m.act(7, _obs(), **BATCHED)
    assert world.names() == (["create", "set_mlp_weights", "act_mlp_host", "ensure_instance"] + [e[0] for e in opt_ins]
                             + ["act_mlp_host"])
    assert world.events[4:4 + len(opt_ins)] == opt_ins and isinstance(a, np.ndarray)
    _route(m, "fused_host")


def test_a_failed_build_is_reported_once_per_compiler_log(world):
    m = _model()
    world.decline, world.log_tail = 1, "error: boom"
    with pytest.warns(RuntimeWarning) as rec:
        m.act(7, torch.from_numpy(_obs()), **BATCHED)
    assert len(rec) == 1
    text = str(rec[0].message)
    assert text.startswith("muax_amd: the on-demand build of a fused act() instance for num_actions=2, embedding_dim=8, "
                           "num_simulations=5 failed; compiler log /nowhere/mzfused_test.log:\nerror: boom")
    assert rec[0].filename == model_mod.__file__  # (the act() frame, as it has always been)
    assert world.names() == ["dirichlet", "create", "set_mlp_weights", "act_mlp", "ensure_instance", "allow_wide",
                             "allow_generic", "act_mlp", "outputs_to_host"]
    m2 = _model(A=3)
    world.decline = 1
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m2.act(7, torch.from_numpy(_obs()), **BATCHED)


def test_everything_declines_one_warning_then_the_stepwise_policy(world):
    m = _model()
    world.decline = 10 ** 6
    obs = torch.from_numpy(_obs())
    with pytest.warns(RuntimeWarning) as rec:
        a, pi, v = m.act(7, obs, num_simulations=6, temperature=0.5, max_depth=4, pb_c_init=1.5, pb_c_base=100,
                         tiebreak=False, global_batch=8, root_offset=2, **BATCHED)
    assert len(rec) == 1 and rec[0].filename == __file__  # the user's act() line
    text = str(rec[0].message)
    assert text.startswith("muax_amd: no in-library act() route for num_actions=2, embedding_dim=8, support_size=10, "
                           f"num_simulations=6 ({NO_INSTANCE}); falling back to the step-wise search with torch modules")
    assert "last failed on-demand build" not in text
    assert world.names() == ["dirichlet", "create", "set_mlp_weights", "act_mlp", "ensure_instance", "allow_wide",
                             "allow_generic", "act_mlp", "policy"]
    _, cls, params, key, root, fns, kw = world.events[-1]
    assert cls == "MuZeroPolicy" and params is m.params and np.array_equal(key, mx.prng.as_key(7))
    assert len(root) == 3 and root[0].shape == (B, 2) and root[1].shape == (B,) and root[2].shape == (B, 8)
    assert fns == (m._recurrent_inference,)
    assert set(kw) == MUZERO_POLICY_KW
    assert kw.pop("dirichlet_noise") is world.noise
    assert kw == dict(num_simulations=6, temperature=0.5, invalid_actions=None, max_depth=4, dirichlet_fraction=0.25,
                      pb_c_init=1.5, pb_c_base=100, gumbel=None, tiebreak=False, with_tree=False, graph=False,
                      graph_version=m._weights_version, global_batch=8, root_offset=2, native_loop=None)
    # delivery: the one concatenated download; root_value is the NETWORK value of the root
    assert a.dtype == np.int32 and a.tolist() == [0, 1, 0] and pi.shape == (B, 2) and pi.dtype == F32
    assert np.array_equal(v, root[1].numpy())
    _route(m, "stepwise")
    world.events.clear()
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # once per shape
        m.act(7, obs, num_simulations=6, **BATCHED)
    assert world.names() == ["dirichlet", "create", "set_mlp_weights", "act_mlp", "ensure_instance", "allow_wide",
                             "allow_generic", "act_mlp", "policy"]
    a, pi, v = m.act(7, obs, num_simulations=6, device_outputs=True, **BATCHED)
    assert isinstance(a, torch.Tensor) and isinstance(v, torch.Tensor) and "outputs_clone" not in world.names()
    _route(m, "stepwise")


def test_everything_declines_on_the_host_round_trip_too(world):
    """NumPy in and out: the host call leads; after the decline the noise is drawn once, for the step-wise search."""
    m = _model()
    world.decline = 10 ** 6
    with pytest.warns(RuntimeWarning) as rec:
        a, pi, v = m.act(7, _obs(), **BATCHED)
    assert len(rec) == 1 and rec[0].filename == __file__ and "no in-library act() route" in str(rec[0].message)
    names = world.names()
    assert names[:3] == ["create", "set_mlp_weights", "act_mlp_host"] and names[-1] == "policy"
    assert names.count("dirichlet") == 1 and names.count("policy") == 1 and names.count("create") == 1
    assert names.index("dirichlet") > names.index("act_mlp_host")
    assert world.events[-1][6]["dirichlet_noise"] is world.noise and isinstance(a, np.ndarray)
    if TYPED:  # (the decline of the host call is the answer: no second attempt on the device call)
        assert names == ["create", "set_mlp_weights", "act_mlp_host", "ensure_instance", "allow_wide", "allow_generic",
                         "act_mlp_host", "dirichlet", "policy"]
    _route(m, "stepwise")


def test_both_opt_ins_switched_off_go_straight_to_the_stepwise_policy(world, monkeypatch):
    monkeypatch.setenv("MUAX_AMD_WIDE", "0")
    monkeypatch.setenv("MUAX_AMD_GENERIC", "0")
    m = _model()
    world.decline = 10 ** 6
    with pytest.warns(RuntimeWarning) as rec:
        m.act(7, torch.from_numpy(_obs()), **BATCHED)
    assert len(rec) == 1 and rec[0].filename == __file__
    assert world.names() == ["dirichlet", "create", "set_mlp_weights", "act_mlp", "ensure_instance", "policy"]
    _route(m, "stepwise")


def test_an_error_that_is_no_missing_instance_propagates_unchanged(world):
    m = _model()
    world.decline, world.error = 1, ValueError("mzs_act_mlp: dirichlet_fraction != 0 needs dirichlet_noise")
    with pytest.raises(ValueError, match="dirichlet_fraction != 0 needs dirichlet_noise") as ei:
        m.act(7, _obs(), **BATCHED)
    assert ei.value is world.error and world.names() == ["create", "set_mlp_weights", "act_mlp_host"]
    # another refusal of the library (the generic route's) is no missing instance either
    world.decline = 1
    world.error = getattr(_lib, "TooLargeForLds", ValueError)(
        "mzs_act_mlp (generic route): num_simulations / embedding too large for the LDS of a workgroup")
    with pytest.raises(ValueError, match="too large for the LDS") as ei:
        m.act(7, torch.from_numpy(_obs()), **BATCHED)
    assert ei.value is world.error and "ensure_instance" not in world.names() and "policy" not in world.names()


def test_a_new_weights_version_rebinds_the_weights_on_the_same_handle(world):
    m = _model()
    m.act(7, _obs(), **BATCHED)
    m.act(8, _obs(1), **BATCHED)
    assert world.names() == ["create", "set_mlp_weights", "act_mlp_host", "act_mlp_host"]
    m.weights_changed()
    m.act(9, _obs(2), **BATCHED)
    m.act(9, torch.from_numpy(_obs(2)), device_outputs=True, **BATCHED)  # the device call: the same handle
    assert world.names(4) == ["set_mlp_weights", "act_mlp_host", "dirichlet", "act_mlp", "outputs_clone"]
    assert len(world.handles) == 1
    m.act(9, _obs(2), num_simulations=6, **BATCHED)  # another configuration: another handle
    assert len(world.handles) == 2


# ------------------------------------------------------------------------------------------------ Gumbel policy
def test_gumbel_policy_served_with_its_own_handle_configuration(world):
    m = _model("gumbel", A=3)
    a, pi, v = m.act(7, _obs(), max_num_considered_actions=4, gumbel_scale=0.5, pb_c_init=2.0, pb_c_base=5, tiebreak=True,
                     temperature=0.5, **BATCHED)
    assert world.names() == ["create", "set_mlp_weights", "act_mlp_host"]
    assert world.events[0][2] == mx.SearchConfig(3, 5, 8, tiebreak=False, pb_c_init=1.25, pb_c_base=19652.0, policy="gumbel",
                                                 max_num_considered_actions=4, gumbel_scale=0.5)
    kw = dict(world.events[2][1])
    kw.pop("obs"), kw.pop("key")
    assert kw == dict(dirichlet_fraction=0.0, invalid_actions=None)  # no noise, no temperature
    assert isinstance(a, np.ndarray)
    _route(m, "fused_host")
    world.events.clear()
    g = torch.zeros(B, 3)
    a, pi, v = m.act(7, _obs(), max_num_considered_actions=4, gumbel_scale=0.5, gumbel=g, **BATCHED)
    assert world.names() == ["act_mlp", "outputs_to_host"]
    kw = dict(world.events[0][1])
    kw.pop("obs"), kw.pop("key")
    assert kw.pop("gumbel") is g and kw == dict(invalid_actions=None, with_tree=False)
    _route(m, "fused")


def test_gumbel_policy_decline_path(world):
    m = _model("gumbel", A=3)
    world.decline = 1
    m.act(7, _obs(), **BATCHED)
    assert world.names() == ["create", "set_mlp_weights", "act_mlp_host", "ensure_instance", "allow_wide", "allow_generic",
                             "act_mlp_host"]
    assert world.events[3] == ("ensure_instance", 3, 8, 21, 5, True) and world.events[4] == ("allow_wide", True, True)
    world.events.clear()
    world.decline = 10 ** 6
    obs = torch.from_numpy(_obs())
    with pytest.warns(RuntimeWarning) as rec:
        a, pi, v = m.act(7, obs, max_num_considered_actions=4, gumbel_scale=0.5, **BATCHED)
    assert len(rec) == 1 and rec[0].filename == __file__ and "num_actions=3, embedding_dim=8" in str(rec[0].message)
    assert world.names() == ["create", "set_mlp_weights", "act_mlp", "ensure_instance", "allow_wide", "allow_generic",
                             "act_mlp", "policy"]
    _, cls, params, key, root, fns, kw = world.events[-1]
    assert cls == "GumbelMuZeroPolicy" and params is m.params and fns == (m._recurrent_inference,)
    assert kw == dict(num_simulations=5, invalid_actions=None, max_depth=None, qtransform="qtransform_by_parent_and_siblings",
                      max_num_considered_actions=4, gumbel_scale=0.5, gumbel=None, with_tree=False, graph=False,
                      graph_version=m._weights_version, global_batch=None, root_offset=0, native_loop=None)
    assert set(kw) == GUMBEL_POLICY_KW and np.array_equal(v, root[1].numpy())
    _route(m, "stepwise")


def test_qtransform_completed_by_mix_value_is_for_the_gumbel_policy(world):
    m = _model("gumbel")
    m.act(7, _obs(), qtransform="qtransform_completed_by_mix_value", **BATCHED)
    assert world.events[0][2].qtransform == "qtransform_completed_by_mix_value"

    def qtransform_completed_by_mix_value():  # (mctx hands the function itself)
        pass

    m.act(7, _obs(), qtransform=qtransform_completed_by_mix_value, **BATCHED)
    assert len(world.handles) == 1
    with pytest.raises(ValueError, match="'qtransform_completed_by_mix_value' is not implemented for this policy"):
        _model().act(7, _obs(), qtransform="qtransform_completed_by_mix_value", **BATCHED)
    with pytest.raises(ValueError, match="is not implemented for this policy"):
        m.act(7, _obs(), qtransform="qtransform_by_min_max", **BATCHED)


# ------------------------------------------------------------------------------------------------ never fused
@pytest.mark.parametrize("base", ["MuZeroPolicy", "GumbelMuZeroPolicy"])
def test_a_user_subclass_of_a_policy_never_takes_a_fused_route(world, base):
    Mine = type("Mine", (getattr(mx, base),), {})
    m = _model(policy_class=Mine)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        a, pi, v = m.act(7, _obs(), **BATCHED)
    assert world.names() == (["dirichlet"] if base == "MuZeroPolicy" else []) + ["policy"]
    assert world.events[-1][1] == "Mine" and isinstance(a, np.ndarray)
    assert set(world.events[-1][6]) == (MUZERO_POLICY_KW if base == "MuZeroPolicy" else GUMBEL_POLICY_KW)
    _route(m, "stepwise")


def test_plugin_nets_never_take_a_fused_route(world):
    class Wrap(torch.nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, *a):
            return self.inner(*a)

    net = _model(A=3).network
    m = mx.MuZero(Wrap(net.representation_fn), Wrap(net.prediction_fn), Wrap(net.dynamic_fn), device="cpu")
    m.init(0, np.zeros((1, 4)))
    m.act(7, _obs(), **BATCHED)
    # (no num_actions on the prediction net: one forward pass of a single row tells the noise's width)
    assert world.names() == ["dirichlet", "policy"] and world.events[0][3] == (B, 3)
    _route(m, "stepwise")


def test_stochastic_policy_on_the_callables_route(world):
    g = torch.Generator().manual_seed(0)
    m = mx.MuZero(mx.nn.create_stochastic_muzero_network(8, 3, 4, 21, generator=g), device="cpu")
    m.init(0, np.zeros((1, 4)))
    a, pi, v = m.act(7, _obs(), global_batch=8, root_offset=2, **BATCHED)
    assert world.names() == ["dirichlet", "policy"]
    assert world.events[0] == ("dirichlet", _dirichlet_key(7), 0.3, (B, 3), 8, 2)
    _, cls, params, key, root, fns, kw = world.events[-1]
    assert cls == "StochasticMuZeroPolicy" and params is m.params and fns == ()
    assert kw.pop("decision_recurrent_fn") == m._decision_inference and kw.pop("chance_recurrent_fn") == m._chance_inference
    assert kw.pop("dirichlet_noise") is world.noise
    assert kw == dict(num_simulations=5, temperature=1.0, invalid_actions=None, max_depth=None, dirichlet_fraction=0.25,
                      pb_c_init=1.25, pb_c_base=19652, gumbel=None, tiebreak=True, with_tree=False, graph=False,
                      graph_version=m._weights_version, global_batch=8, root_offset=2, num_chance_outcomes=4,
                      afterstate_shape=(8,))
    assert isinstance(a, np.ndarray) and np.array_equal(v, root[1].numpy())
    _route(m, "callables")
    with pytest.raises(ValueError, match="is not implemented for this policy"):
        m.act(7, _obs(), qtransform="qtransform_completed_by_mix_value", **BATCHED)


# ------------------------------------------------------------------------------------------------ _lib.check
class _StubLibrary:
    def __init__(self, message):
        self.message = message

    def mzs_last_error(self, handle):
        return self.message.encode() if self.message is not None else None


@pytest.mark.skipif(not TYPED, reason="the typed refusals are what this test is about")
@pytest.mark.parametrize("message,cls", [
    ("mzs_act_mlp: no fused kernel instance for this (A, E, F, S) (muax_amd/csrc/mz_instances.def); use the step-wise path",
     "NoKernelInstance"),
    ("mzs_mlp_loss_grad: no kernel instance for this (A, E, F): support_size must be 8..31", "NoKernelInstance"),
    ("unroll_steps 9 too large for the LDS (at most 8 for this (A, E, F))", "TooLargeForLds"),
    ("mzs_resnet_search: this handle's tree has no cached decisions (too large, or MZS_STEP_WALK=1)", "NoCachedDecisions"),
    ("mzs_create: num_actions + num_chance_outcomes must be at most 64", "Unsupported")])
def test_check_raises_a_class_per_refusal_and_passes_the_message_through(monkeypatch, message, cls):
    monkeypatch.setattr(_lib, "load", lambda build_if_missing=True: _StubLibrary(message))
    assert _lib.check(_lib.MZS_OK) is None
    with pytest.raises(ValueError) as ei:
        _lib.check(_lib.MZS_E_UNSUPPORTED, object())
    assert type(ei.value) is getattr(_lib, cls) and isinstance(ei.value, _lib.Unsupported) and str(ei.value) == message
    assert getattr(mx, cls) is getattr(_lib, cls)
    # the same words under another status code are not a refusal of a configuration
    with pytest.raises(ValueError) as ei:
        _lib.check(_lib.MZS_E_INVALID)
    assert type(ei.value) is ValueError and str(ei.value) == message
    for code in (_lib.MZS_E_RUNTIME, _lib.MZS_E_NODEVICE):
        with pytest.raises(RuntimeError) as ei:
            _lib.check(code)
        assert type(ei.value) is RuntimeError and str(ei.value) == message


@pytest.mark.skipif(not TYPED, reason="the typed refusals are what this test is about")
def test_refusal_classes_are_value_errors_one_level_deep(monkeypatch):
    for name in ("NoKernelInstance", "TooLargeForLds", "NoCachedDecisions"):
        assert getattr(_lib, name).__bases__ == (_lib.Unsupported,)
    assert _lib.Unsupported.__bases__ == (ValueError,)
    monkeypatch.setattr(_lib, "load", lambda build_if_missing=True: _StubLibrary(None))
    with pytest.raises(_lib.Unsupported, match="mzsearch error -2"):
        _lib.check(_lib.MZS_E_UNSUPPORTED)
