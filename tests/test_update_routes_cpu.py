"""CPU tests of the routing of MuZero.update() and MuZero.unroll_values() (muax_amd/model.py): which step object is
constructed, which calls are made in which order and with which arguments, which route is named and what is raised, for
the default MLP trio and the default stochastic MLP family.  No GPU and no library: `loss.FusedLossGrad`,
`loss.StochasticFusedLossGrad`, `unroll.FusedUnrollValues`, `unroll.StochasticFusedUnrollValues`, the two loss functions,
the two torch unrolls, `_jit.ensure_train_instance` / `ensure_wide_train_instance` and `sharding.allreduce_mean_flat` are
recorders, and the model is a CPU model whose `device` attribute says "cuda", so that the routing's predicates hold.
The GPU suites check what the routes compute; this file pins the routing itself."""
import numpy as np
import pytest
import torch

import muax_amd as mx
from muax_amd import _jit, _lib, sharding
from muax_amd import loss as loss_mod
from muax_amd import unroll as unroll_mod

F32 = np.float32
B, L = 3, 2
CUDA = torch.device("cuda")
NO_INSTANCE = "mzs_mlp_loss_grad: no kernel instance for this (A, E, F)"
TOO_LARGE = "unroll_steps 9 too large for the LDS (at most 8 for this (A, E, F))"
HIP_TRIO = "backend='hip' needs the default MLP trio on a GPU and the default loss"
HIP_STOCHASTIC = (HIP_TRIO + " (the stochastic loss of an SMZNetwork runs on torch autograd only, unless the model was made "
                  "with stochastic_fused_update=True: the default stochastic MLP family on a GPU, obs_dim up to 32)")


class World:
    """What one test's fakes share: the log of calls, how many fused calls still decline and with which error, and what
    the two on-demand builders answer."""

    def __init__(self):
        self.events = []
        self.decline, self.error = 0, None
        self.ensure = self.ensure_wide = False

    def names(self, start=0):
        return [e[0] for e in self.events[start:]]

    def of(self, name):
        return [e for e in self.events if e[0] == name]


def _all_params(model):
    return [p for mod in model.network for p in mod.parameters()]


class FakeStep:
    """In place of a fused training step: `params`, `views` into a flat gradient, a loss tensor; A / E / S for the
    on-demand build."""
    world, name = None, None

    def __init__(self, model):
        self.world.events.append(("construct", self.name))
        self.params = _all_params(model)
        self.grads = torch.full((sum(p.numel() for p in self.params),), 0.5)
        self.views, off = [], 0
        for p in self.params:
            self.views.append(self.grads[off:off + p.numel()].view_as(p))
            off += p.numel()
        self.loss = torch.tensor([1.5])
        self.A, self.E, self.S = model.pred_func.num_actions, model.repr_func.embedding_dim, model._support_size

    def __call__(self, batch, **kw):
        w = self.world
        w.events.append(("step", self.name, batch, kw))
        if w.decline > 0:
            w.decline -= 1
            raise w.error
        return self.loss, self.grads


class FakeUnroll:
    world, name = None, None

    def __init__(self, model):
        self.world.events.append(("construct", self.name))

    def __call__(self, batch, kp, codes=False):
        self.world.events.append(("unroll", self.name, batch, kp))
        self.out = torch.zeros(B, kp), torch.ones(B, kp)
        return self.out


def _replace(monkeypatch, module, name, fake):
    """`module.name = fake`, and the same in a module-level record (a NamedTuple) that holds the object itself."""
    real = getattr(module, name)
    monkeypatch.setattr(module, name, fake)
    for attr, rec in list(vars(module).items()):
        if isinstance(rec, tuple) and hasattr(rec, "_fields") and any(x is real for x in rec):
            monkeypatch.setattr(module, attr, type(rec)(*[fake if x is real else x for x in rec]))


@pytest.fixture
def world(monkeypatch):
    w = World()
    for module, name, cls, tag in ((loss_mod, "FusedLossGrad", FakeStep, "trio"),
                                   (loss_mod, "StochasticFusedLossGrad", FakeStep, "stochastic"),
                                   (unroll_mod, "FusedUnrollValues", FakeUnroll, "trio"),
                                   (unroll_mod, "StochasticFusedUnrollValues", FakeUnroll, "stochastic")):
        _replace(monkeypatch, module, name, type(name, (cls,), {"world": w, "name": tag}))

    def loss_fn(tag):
        def fn(model, batch, *args, **kwargs):
            w.events.append(("loss_fn", tag, batch, args, kwargs))
            return sum((p ** 2).sum() for p in _all_params(model))
        return fn

    def torch_unroll(tag):
        def fn(model, batch, kp, **kwargs):
            w.events.append(("torch_unroll", tag, batch, kp))
            w.out = torch.zeros(B, kp), torch.ones(B, kp)
            return w.out
        return fn

    w.loss_fn = loss_fn
    monkeypatch.setattr(loss_mod, "default_loss_fn", loss_fn("default"))
    monkeypatch.setattr(loss_mod, "stochastic_loss_fn", loss_fn("stochastic"))
    _replace(monkeypatch, unroll_mod, "torch_unroll_values", torch_unroll("trio"))
    _replace(monkeypatch, unroll_mod, "torch_stochastic_unroll_values", torch_unroll("stochastic"))

    def ensure(name, answer):
        def fn(A, E, F, **kw):
            w.events.append((name, A, E, F))
            return getattr(w, answer)
        return fn

    monkeypatch.setattr(_jit, "ensure_train_instance", ensure("ensure_train_instance", "ensure"))
    monkeypatch.setattr(_jit, "ensure_wide_train_instance", ensure("ensure_wide_train_instance", "ensure_wide"))
    monkeypatch.setattr(sharding, "allreduce_mean_flat", lambda tensors, **kw: w.events.append(("mean", list(tensors))))
    return w


def _recording_optimizer(w):
    opt = mx.optimizers.create_optimizer("adam", 1e-2)
    for name in ("init", "load_state_dict", "step"):
        def recorded(*a, _real=getattr(opt, name), _name=name, **k):
            w.events.append(("opt_" + _name,))
            return _real(*a, **k)
        setattr(opt, name, recorded)
    return opt


def _trio(w=None, A=2, E=8, obs_dim=4, support=10, device=CUDA, **kw):
    g = torch.Generator().manual_seed(0)
    F = 2 * support + 1
    net = mx.nn.MZNetwork(mx.nn.Representation(E, generator=g), mx.nn.Prediction(A, F, generator=g),
                          mx.nn.Dynamic(E, A, F, generator=g))
    m = mx.MuZero(net, device="cpu", support_size=support, optimizer=_recording_optimizer(w) if w else None, **kw)
    m.init(0, np.zeros((1, obs_dim)))
    m.device = device
    return m


def _stochastic(w=None, A=3, C=4, E=8, obs_dim=4, support=10, device=CUDA, fused=True, unroll=True, **kw):
    g = torch.Generator().manual_seed(0)
    net = mx.nn.create_stochastic_muzero_network(E, A, C, 2 * support + 1, generator=g)
    m = mx.MuZero(net, device="cpu", support_size=support, optimizer=_recording_optimizer(w) if w else None,
                  stochastic_fused_update=fused, stochastic_unroll_values=unroll, **kw)
    m.init(0, np.zeros((1, obs_dim)))
    m.device = device
    return m


class _Wrap(torch.nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, *a):
        return self.inner(*a)


def _plugin(w=None):
    net = _trio().network
    m = mx.MuZero(_Wrap(net.representation_fn), _Wrap(net.prediction_fn), _Wrap(net.dynamic_fn), device="cpu",
                  optimizer=_recording_optimizer(w) if w else None)
    m.init(0, np.zeros((1, 4)))
    m.device = CUDA
    return m


def _batch(A=2, obs_dim=4, all_obs=True, seed=0):
    rng = np.random.default_rng(seed)
    return mx.Transition(obs=rng.uniform(-1, 1, (B, L, obs_dim) if all_obs else (B, obs_dim)).astype(F32),
                         a=rng.integers(0, A, (B, L)), r=rng.uniform(-2, 3, (B, L)).astype(F32),
                         Rn=rng.uniform(-3, 6, (B, L)).astype(F32), pi=rng.dirichlet(np.ones(A), (B, L)).astype(F32))


def _refusal(cls, text):
    return getattr(_lib, cls)(text)


TRIO_KW = dict(divide_by_length=False, sample_weight=None)
STOCHASTIC_KW = dict(vqvae_beta=0.25, divide_by_length=False, sample_weight=None)
MAKE = {"trio": _trio, "stochastic": _stochastic}
CACHE = {"trio": "_fused_train", "stochastic": "_fused_stoch_train"}
ROUTE = {"trio": "hip_fused", "stochastic": "hip_stochastic_fused"}
BATCH_A = {"trio": 2, "stochastic": 3}


# ------------------------------------------------------------------------------------------------ update(): served
@pytest.mark.parametrize("family", ["trio", "stochastic"])
def test_update_served_by_the_fused_step(world, family):
    m = MAKE[family](world)
    b = _batch(BATCH_A[family])
    v0 = m._weights_version
    out = m.update(b)
    assert world.names() == ["opt_init", "construct", "step", "mean", "opt_step"]
    step = getattr(m, CACHE[family])
    assert world.events[1] == ("construct", family) and step.name == family
    assert getattr(m, CACHE["stochastic" if family == "trio" else "trio"]) is None
    _, _, got_batch, kw = world.events[2]
    assert got_batch is b and kw == (TRIO_KW if family == "trio" else STOCHASTIC_KW)
    (_, meant), = world.of("mean")
    assert len(meant) == 1 and meant[0] is step.grads
    assert out == {"loss": 1.5} and m._last_update_route == ROUTE[family] and m._weights_version == v0 + 1
    # the optimiser consumed the views (Adam's first step moves every weight by the learning rate) and cleared them
    assert all(p.grad is None for p in step.params)
    world.events.clear()
    m.update(b, divide_by_length=True, backend="hip")
    assert world.names() == ["step", "mean", "opt_step"] and getattr(m, CACHE[family]) is step
    assert world.events[0][3]["divide_by_length"] is True and m._weights_version == v0 + 2


def test_update_hands_the_stochastic_step_its_three_keywords(world):
    m = _stochastic(world)
    sw = torch.ones(B)
    m.update(_batch(3), vqvae_beta=0.5, divide_by_length=True, sample_weight=sw)
    kw = world.of("step")[0][3]
    assert kw.keys() == STOCHASTIC_KW.keys() and kw["vqvae_beta"] == 0.5 and kw["divide_by_length"] is True
    assert kw["sample_weight"] is sw and m._last_update_route == "hip_stochastic_fused"


@pytest.mark.parametrize("family", ["trio", "stochastic"])
def test_dp_mean_false_skips_the_mean(world, family):
    m = MAKE[family](world)
    m.update(_batch(BATCH_A[family]), dp_mean=False)
    assert world.names() == ["opt_init", "construct", "step", "opt_step"] and m._last_update_route == ROUTE[family]
    world.events.clear()
    m.update(_batch(BATCH_A[family]), dp_mean=False, backend="torch")
    assert world.names() == ["loss_fn", "opt_step"] and m._last_update_route == "torch"
    world.events.clear()
    m.update(_batch(BATCH_A[family]), backend="torch")
    assert world.names() == ["loss_fn", "mean", "opt_step"]
    (_, meant), = world.of("mean")
    assert len(meant) == len(_all_params(m)) and all(g is not None for g in meant)


# ------------------------------------------------------------------------------------------------ update(): refusals
def test_trio_no_instance_builds_one_on_demand_and_calls_again(world):
    m = _trio(world, A=3, E=8)
    world.decline, world.error, world.ensure = 1, _refusal("NoKernelInstance", NO_INSTANCE), True
    b = _batch(3)
    m.update(b, divide_by_length=True)
    assert world.names() == ["opt_init", "construct", "step", "ensure_train_instance", "step", "mean", "opt_step"]
    assert world.of("ensure_train_instance") == [("ensure_train_instance", 3, 8, 21)]
    first, second = world.of("step")
    assert first[2] is b and second[2] is b and first[3] == second[3] == dict(divide_by_length=True, sample_weight=None)
    assert m._last_update_route == "hip_fused"
    # the narrow builder says no: the wide one is asked
    world.events.clear()
    world.decline, world.ensure, world.ensure_wide = 1, False, True
    m.update(b, backend="hip")
    assert world.names() == ["step", "ensure_train_instance", "ensure_wide_train_instance", "step", "mean", "opt_step"]
    assert world.of("ensure_wide_train_instance") == [("ensure_wide_train_instance", 3, 8, 21)]
    assert m._last_update_route == "hip_fused"


def test_trio_no_instance_and_no_build_is_torch_under_auto_and_raises_under_hip(world):
    m = _trio(world)
    world.decline, world.error = 1, _refusal("NoKernelInstance", NO_INSTANCE)
    v0 = m._weights_version
    b = _batch()
    m.update(b)
    assert world.names() == ["opt_init", "construct", "step", "ensure_train_instance", "ensure_wide_train_instance",
                             "loss_fn", "mean", "opt_step"]
    assert world.of("loss_fn")[0][1:] == ("default", b, (), {})
    assert m._last_update_route == "torch" and m._fused_train is not None and m._weights_version == v0 + 1
    world.events.clear()
    world.decline = 1
    with pytest.raises(_lib.NoKernelInstance) as ei:
        m.update(b, backend="hip")
    assert ei.value is world.error and m._weights_version == v0 + 1
    assert world.names() == ["step", "ensure_train_instance", "ensure_wide_train_instance"]
    # the call after a build fails too: the same ladder, no second build
    world.events.clear()
    world.decline, world.ensure = 2, True
    m.update(b)
    assert world.names() == ["step", "ensure_train_instance", "step", "loss_fn", "mean", "opt_step"]
    assert m._last_update_route == "torch"


def test_trio_too_large_for_the_lds_never_builds(world):
    m = _trio(world)
    world.decline, world.error, world.ensure = 1, _refusal("TooLargeForLds", TOO_LARGE), True
    m.update(_batch())
    assert world.names() == ["opt_init", "construct", "step", "loss_fn", "mean", "opt_step"]
    assert m._last_update_route == "torch" and m._fused_train is not None
    world.events.clear()
    world.decline = 1
    with pytest.raises(_lib.TooLargeForLds) as ei:
        m.update(_batch(), backend="hip")
    assert ei.value is world.error and world.names() == ["step"]


@pytest.mark.parametrize("cls,text", [("NoKernelInstance", NO_INSTANCE), ("TooLargeForLds", TOO_LARGE)])
def test_stochastic_refusal_is_torch_under_auto_and_raises_under_hip_without_a_build(world, cls, text):
    m = _stochastic(world)
    world.decline, world.error, world.ensure, world.ensure_wide = 1, _refusal(cls, text), True, True
    b = _batch(3)
    m.update(b, vqvae_beta=0.5)
    assert world.names() == ["opt_init", "construct", "step", "loss_fn", "mean", "opt_step"]
    assert world.of("loss_fn")[0][1:] == ("stochastic", b, (), dict(vqvae_beta=0.5))
    assert m._last_update_route == "torch" and m._fused_stoch_train is not None and m._fused_train is None
    world.events.clear()
    world.decline = 1
    with pytest.raises(getattr(_lib, cls)) as ei:
        m.update(b, backend="hip")
    assert ei.value is world.error and world.names() == ["step"]


def test_an_error_that_is_no_typed_refusal_propagates_under_auto(world):
    for m, A in ((_trio(world), 2), (_stochastic(world), 3)):
        world.events.clear()
        world.decline, world.error = 1, ValueError("batch.obs has 5 features, the network takes 4")
        with pytest.raises(ValueError) as ei:
            m.update(_batch(A))
        assert ei.value is world.error and world.names() == ["opt_init", "construct", "step"]


# ------------------------------------------------------------------------------------------------ update(): never fused
@pytest.mark.parametrize("why", ["flag_off", "args", "keyword", "obs_dim"])
def test_what_keeps_the_stochastic_family_off_its_kernel(world, why):
    m = _stochastic(world, fused=why != "flag_off", obs_dim=33 if why == "obs_dim" else 4)
    b = _batch(3, obs_dim=33 if why == "obs_dim" else 4)
    args = (0.5,) if why == "args" else ()
    kwargs = dict(pi_all_pairs=False) if why == "keyword" else {}
    v0 = m._weights_version
    m.update(b, *args, **kwargs)
    assert world.names() == ["opt_init", "loss_fn", "mean", "opt_step"]
    assert world.of("loss_fn")[0][1:] == ("stochastic", b, args, kwargs)
    assert m._last_update_route == "torch" and m._fused_stoch_train is None and m._fused_train is None
    assert m._weights_version == v0 + 1
    with pytest.raises(ValueError) as ei:
        m.update(b, *args, backend="hip", **kwargs)
    assert str(ei.value) == HIP_STOCHASTIC and m._fused_stoch_train is None and m._weights_version == v0 + 1


def test_the_trio_takes_obs_dim_up_to_128(world):
    m = _trio(world, obs_dim=128)
    m.update(_batch(obs_dim=128))
    assert m._last_update_route == "hip_fused"
    m = _trio(world, obs_dim=129)
    m.update(_batch(obs_dim=129))
    assert m._last_update_route == "torch" and m._fused_train is None
    m = _stochastic(world, obs_dim=32)
    m.update(_batch(3, obs_dim=32))
    assert m._last_update_route == "hip_stochastic_fused"


@pytest.mark.parametrize("why", ["loss_fn", "pi_all_pairs", "torch", "cpu"])
def test_what_keeps_the_trio_off_its_kernel(world, why):
    m = _trio(world, device=torch.device("cpu") if why == "cpu" else CUDA)
    if why == "loss_fn":
        m.loss_fn = world.loss_fn("custom")
    kwargs = dict(pi_all_pairs=True) if why == "pi_all_pairs" else {}
    b = _batch()
    v0 = m._weights_version
    m.update(b, backend="torch" if why == "torch" else "auto", **kwargs)
    assert world.names() == ["opt_init", "loss_fn", "mean", "opt_step"]
    assert world.of("loss_fn")[0][1:] == ("custom" if why == "loss_fn" else "default", b, (), kwargs)
    assert m._last_update_route == "torch" and m._fused_train is None and m._weights_version == v0 + 1
    if why != "torch":
        with pytest.raises(ValueError) as ei:
            m.update(b, backend="hip", **kwargs)
        assert str(ei.value) == HIP_TRIO and m._fused_train is None


def test_backend_hip_refuses_plugin_nets_and_an_smznetwork_without_its_flag(world):
    m = _plugin(world)
    with pytest.raises(ValueError) as ei:
        m.update(_batch(), backend="hip")
    assert str(ei.value) == HIP_TRIO and "construct" not in world.names() and "loss_fn" not in world.names()
    m.update(_batch())
    assert m._last_update_route == "torch" and world.of("loss_fn")[0][1] == "default"
    m = _stochastic(world, fused=False)
    with pytest.raises(ValueError) as ei:
        m.update(_batch(3), backend="hip")
    assert str(ei.value) == HIP_STOCHASTIC and "construct" not in world.names()
    with pytest.raises(ValueError, match="call init"):
        mx.MuZero(_trio().network, device="cpu").update(_batch())


# ------------------------------------------------------------------------------------------------ update(): sample_weight
@pytest.mark.parametrize("family", ["trio", "stochastic"])
@pytest.mark.parametrize("a_is_tensor", [False, True])
def test_sample_weight_of_a_wrong_shape_raises_before_anything_runs(world, family, a_is_tensor):
    m = MAKE[family](world)
    b = _batch(BATCH_A[family])
    if a_is_tensor:
        b = mx.Transition(obs=b.obs, a=torch.from_numpy(b.a), r=b.r, Rn=b.Rn, pi=b.pi)
    v0 = m._weights_version
    for bad, shape in ((torch.ones(B + 1), (B + 1,)), (np.ones((B, 1), F32), (B, 1)), (1.0, ())):
        for backend in ("auto", "hip", "torch"):
            with pytest.raises(ValueError) as ei:
                m.update(b, sample_weight=bad, backend=backend)
            assert str(ei.value) == f"sample_weight must be [B] with B = {B}, got {shape}"
    assert world.events == [] and m._optimizer.opt is None and m._weights_version == v0


def test_a_sample_weight_reaches_the_fused_step_its_retry_and_the_loss_function(world):
    m = _trio(world)
    sw = torch.full((B,), 0.5)
    b = _batch()
    world.decline, world.error, world.ensure = 1, _refusal("NoKernelInstance", NO_INSTANCE), True
    m.update(b, sample_weight=sw)
    first, second = world.of("step")
    assert first[3] == second[3] and first[3].keys() == TRIO_KW.keys() and second[3]["sample_weight"] is sw
    # the torch route: the default loss and a custom one get it as the keyword, and only when it was given
    world.events.clear()
    m.update(b, sample_weight=sw, backend="torch")
    (_, tag, _, args, kwargs), = world.of("loss_fn")
    assert tag == "default" and args == () and kwargs.keys() == {"sample_weight"} and kwargs["sample_weight"] is sw
    custom = _trio(world)
    custom.loss_fn = world.loss_fn("custom")
    world.events.clear()
    custom.update(b, 7, sample_weight=sw, divide_by_length=True)
    (_, tag, _, args, kwargs), = world.of("loss_fn")
    assert tag == "custom" and args == (7,) and kwargs.keys() == {"sample_weight", "divide_by_length"}
    assert kwargs["sample_weight"] is sw and custom._fused_train is None
    world.events.clear()
    custom.update(b)
    assert world.of("loss_fn")[0][3:] == ((), {})


# ------------------------------------------------------------------------------------------------ update(): the optimiser
@pytest.mark.parametrize("backend", ["auto", "torch"])
def test_the_optimiser_is_bound_once_and_a_loaded_state_is_resumed_once(world, backend):
    donor = _trio(world)
    donor.update(_batch(), backend=backend)
    state = donor.optimizer_state
    assert state["opt"]["state"][0]["step"] == 1
    world.events.clear()
    m = _trio(world)
    m._loaded_opt_state = state  # (what load() leaves when no optimiser is bound yet)
    m.update(_batch(), backend=backend)
    assert world.names()[:2] == ["opt_init", "opt_load_state_dict"] and m._loaded_opt_state is None
    assert m.optimizer_state["opt"]["state"][0]["step"] == 2  # resumed, then stepped
    m.update(_batch(), backend=backend)
    m.update(_batch(), backend=backend)
    assert world.names().count("opt_init") == 1 and world.names().count("opt_load_state_dict") == 1
    assert world.names().count("opt_step") == 3


def test_update_makes_the_default_optimiser_when_none_was_given(world):
    m = _trio()
    assert m._optimizer is None
    m.update(_batch())
    assert isinstance(m._optimizer, mx.optimizers.Optimizer) and isinstance(m._optimizer.opt, torch.optim.Adam)
    opt = m._optimizer
    m.update(_batch())
    assert m._optimizer is opt


# ------------------------------------------------------------------------------------------------ unroll_values()
UNROLL_FUSED = {"trio": "FusedUnrollValues", "stochastic": "StochasticFusedUnrollValues"}
HIP_UNROLL = {"trio": "backend='hip' needs the default MLP trio on a GPU",
              "stochastic": "backend='hip' needs the default stochastic MLP family on a GPU"}
# one model beyond each limit of the family's table, at hi + 1 (unroll.LIMITS / unroll.STOCHASTIC_LIMITS)
BEYOND = {"trio": {"obs_dim": dict(obs_dim=129), "embed_dim": dict(E=65), "num_actions": dict(A=65),
                   "support_size": dict(support=32)},
          "stochastic": {"obs_dim": dict(obs_dim=129), "embed_dim": dict(E=65), "num_actions": dict(A=64, C=1),
                         "num_chance_outcomes": dict(A=1, C=64), "actions_and_outcomes": dict(A=33, C=32),
                         "support_size": dict(support=32)}}
TABLE = {"trio": "LIMITS", "stochastic": "STOCHASTIC_LIMITS"}
WITHIN = {"trio": "within_limits", "stochastic": "within_stochastic_limits"}


@pytest.mark.parametrize("family", ["trio", "stochastic"])
def test_unroll_served_by_one_fused_object_over_three_calls(world, family):
    m = MAKE[family]()
    b = _batch(BATCH_A[family])
    outs = [m.unroll_values(b), m.unroll_values(b, 1, backend="hip"), m.unroll_values(b, k_prio=L)]
    assert world.names() == ["construct", "unroll", "unroll", "unroll"] and world.events[0] == ("construct", family)
    assert [e[3] for e in world.of("unroll")] == [L, 1, L] and all(e[2] is b for e in world.of("unroll"))
    assert type(m._fused_unroll).__name__ == UNROLL_FUSED[family] and outs[2] is m._fused_unroll.out
    assert outs[1][0].shape == (B, 1)


@pytest.mark.parametrize("family", ["trio", "stochastic"])
def test_unroll_backend_torch_never_constructs(world, family):
    m = MAKE[family]()
    b = _batch(BATCH_A[family])
    out = m.unroll_values(b, 1, backend="torch")
    assert world.events == [("torch_unroll", family, b, 1)] and out is world.out and m._fused_unroll is None
    # off the GPU: "auto" is torch too, "hip" says what it needs
    cpu = MAKE[family](device=torch.device("cpu"))
    cpu.unroll_values(b)
    assert world.events[1:] == [("torch_unroll", family, b, L)] and cpu._fused_unroll is None
    with pytest.raises(ValueError) as ei:
        cpu.unroll_values(b, backend="hip")
    assert str(ei.value) == HIP_UNROLL[family] and len(world.events) == 2


def test_unroll_hip_refuses_plugin_nets(world):
    m = _plugin()
    with pytest.raises(ValueError) as ei:
        m.unroll_values(_batch(), backend="hip")
    assert str(ei.value) == HIP_UNROLL["trio"]
    m.unroll_values(_batch())
    assert world.names() == ["torch_unroll"] and m._fused_unroll is None
    # six plugin modules with the flag on: not the family
    net = _stochastic().network
    s = mx.MuZero(mx.nn.SMZNetwork(*[_Wrap(x) for x in net]), device="cpu", stochastic_unroll_values=True)
    s.init(0, np.zeros((1, 4)))
    s.device = CUDA
    with pytest.raises(ValueError) as ei:
        s.unroll_values(_batch(3), backend="hip")
    assert str(ei.value) == HIP_UNROLL["stochastic"]
    s.unroll_values(_batch(3))
    assert world.events[-1][:2] == ("torch_unroll", "stochastic") and s._fused_unroll is None


@pytest.mark.parametrize("family,key", [(f, k) for f in BEYOND for k in BEYOND[f]])
def test_unroll_beyond_a_limit_is_torch_under_auto_and_the_librarys_answer_under_hip(world, family, key):
    assert set(BEYOND[family]) == set(getattr(unroll_mod, TABLE[family]))
    shape = BEYOND[family][key]
    m = MAKE[family](**shape)
    assert not getattr(unroll_mod, WITHIN[family])(m) and getattr(unroll_mod, WITHIN[family])(MAKE[family]())
    b = _batch(shape.get("A", BATCH_A[family]), obs_dim=shape.get("obs_dim", 4))
    m.unroll_values(b)
    assert world.events == [("torch_unroll", family, b, L)] and m._fused_unroll is None
    m.unroll_values(b, backend="hip")  # (reaches the kernel's wrapper: the library names the limit)
    assert world.names(1) == ["construct", "unroll"] and m._fused_unroll is not None


def test_unroll_checks_come_in_order_and_before_anything_is_constructed(world):
    m = _stochastic(unroll=False)
    assert not m.unrolls_stochastic
    for backend in ("auto", "hip", "torch"):
        with pytest.raises(NotImplementedError) as ei:
            m.unroll_values(_batch(3), backend=backend)
        assert str(ei.value) == "unroll_values is not built for an SMZNetwork (its unroll needs every step's chance code)"
    with pytest.raises(ValueError, match="backend must be 'auto', 'hip' or 'torch', got 'cuda'"):
        m.unroll_values(_batch(3), backend="cuda")
    with pytest.raises(ValueError, match="call init"):
        mx.MuZero(_trio().network, device="cpu").unroll_values(_batch())
    m = _stochastic()
    assert m.unrolls_stochastic
    with pytest.raises(ValueError, match=r"k_prio must be in 1\.\.2 \(the window length\), got 3"):
        m.unroll_values(_batch(3), 3)
    for backend in ("auto", "hip", "torch"):
        with pytest.raises(ValueError) as ei:
            m.unroll_values(_batch(3, all_obs=False), backend=backend)
        assert str(ei.value) == ("the stochastic unroll needs every step's observation: batch.obs must be [B, L, ...] with "
                                 f"L = {L} rows per window, got {(B, 4)} (DeviceReplayBuffer.sample hands them out with "
                                 "all_obs=True)")
    assert world.events == [] and m._fused_unroll is None
    # the trio reads the first observation of a window only: [B, obs_dim] will do
    t = _trio()
    t.unroll_values(_batch(all_obs=False))
    assert world.names() == ["construct", "unroll"]
