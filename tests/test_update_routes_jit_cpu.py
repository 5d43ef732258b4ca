"""CPU tests of update()'s retry ladder for the stochastic family with `stochastic_train_on_demand=True`, in the fake
world of test_update_routes_cpu.py (imported, not edited): a refusal, ONE call of _jit.ensure_stochastic_train_instance
with (A, C, E, F, obs_dim), a second step; a build that is unavailable is torch under "auto" and a raise under "hip";
observations 33 to 128 wide are admitted only with the flag."""
import pytest

from muax_amd import _jit, _lib
from test_update_routes_cpu import (HIP_STOCHASTIC, NO_INSTANCE, TOO_LARGE, FakeStep, _batch, _refusal, _stochastic,  # noqa: F401
                                    world)


@pytest.fixture
def jit_world(world, monkeypatch):
    """... plus the stochastic builder as a recorder, and C / obs_dim on the fake step as on the real one."""
    world.ensure_stochastic = False

    def ensure(A, C, E, F, obs_dim, **kw):
        world.events.append(("ensure_stochastic_train_instance", A, C, E, F, obs_dim))
        return world.ensure_stochastic
    monkeypatch.setattr(_jit, "ensure_stochastic_train_instance", ensure)
    init = FakeStep.__init__

    def with_c(self, model):
        init(self, model)
        self.C, self.obs_dim = model.after_pred_func.num_actions, model.repr_func.obs_dim
    monkeypatch.setattr(FakeStep, "__init__", with_c)
    return world


def test_a_refusal_builds_once_and_calls_again(jit_world):
    w = jit_world
    m = _stochastic(w, A=3, C=4, E=8, obs_dim=40, stochastic_train_on_demand=True)
    w.decline, w.error, w.ensure_stochastic = 1, _refusal("NoKernelInstance", NO_INSTANCE), True
    w.ensure = w.ensure_wide = True  # (the trio's builders are never asked)
    b = _batch(3, obs_dim=40)
    m.update(b, vqvae_beta=0.5)
    assert w.names() == ["opt_init", "construct", "step", "ensure_stochastic_train_instance", "step", "mean", "opt_step"]
    assert w.of("ensure_stochastic_train_instance") == [("ensure_stochastic_train_instance", 3, 4, 8, 21, 40)]
    first, second = w.of("step")
    assert first[2] is b and second[2] is b and first[3] == second[3] == dict(vqvae_beta=0.5, divide_by_length=False, sample_weight=None)
    assert m._last_update_route == "hip_stochastic_fused"
    w.events.clear()
    m.update(b, backend="hip")  # served: no build
    assert w.names() == ["step", "mean", "opt_step"] and m._last_update_route == "hip_stochastic_fused"


def test_no_build_is_torch_under_auto_and_raises_under_hip(jit_world):
    w = jit_world
    m = _stochastic(w, stochastic_train_on_demand=True)
    w.decline, w.error = 1, _refusal("NoKernelInstance", NO_INSTANCE)
    b = _batch(3)
    m.update(b)
    assert w.names() == ["opt_init", "construct", "step", "ensure_stochastic_train_instance", "loss_fn", "mean", "opt_step"]
    assert m._last_update_route == "torch" and m._fused_stoch_train is not None
    w.events.clear()
    w.decline = 1
    with pytest.raises(_lib.NoKernelInstance) as ei:
        m.update(b, backend="hip")
    assert ei.value is w.error and w.names() == ["step", "ensure_stochastic_train_instance"]
    # the call after a build refuses too: the same ladder, no second build
    w.events.clear()
    w.decline, w.ensure_stochastic = 2, True
    m.update(b)
    assert w.names() == ["step", "ensure_stochastic_train_instance", "step", "loss_fn", "mean", "opt_step"]
    assert m._last_update_route == "torch"


def test_too_large_for_the_lds_never_builds(jit_world):
    w = jit_world
    m = _stochastic(w, stochastic_train_on_demand=True)
    w.decline, w.error, w.ensure_stochastic = 1, _refusal("TooLargeForLds", TOO_LARGE), True
    m.update(_batch(3))
    assert w.names() == ["opt_init", "construct", "step", "loss_fn", "mean", "opt_step"] and m._last_update_route == "torch"


@pytest.mark.parametrize("obs_dim", [33, 128, 129])
def test_wide_observations_are_admitted_only_with_the_flag(jit_world, obs_dim):
    w = jit_world
    b = _batch(3, obs_dim=obs_dim)
    on = _stochastic(w, obs_dim=obs_dim, stochastic_train_on_demand=True)
    on.update(b)
    assert on._last_update_route == ("hip_stochastic_fused" if obs_dim <= 128 else "torch")
    off = _stochastic(w, obs_dim=obs_dim)
    off.update(b)
    assert off._last_update_route == "torch" and off._fused_stoch_train is None
    with pytest.raises(ValueError) as ei:
        off.update(b, backend="hip")
    assert str(ei.value) == HIP_STOCHASTIC
    # the new flag alone changes nothing: it takes effect together with stochastic_fused_update
    alone = _stochastic(w, obs_dim=obs_dim, fused=False, stochastic_train_on_demand=True)
    alone.update(b)
    assert alone._last_update_route == "torch" and alone._fused_stoch_train is None
    assert w.of("ensure_stochastic_train_instance") == []


def test_the_plain_obs_dim_refusal_beyond_32_builds_too(jit_world):
    """With nothing registered the library answers 33 observations with its plain "obs_dim must be 1..32"."""
    w = jit_world
    text = "mzs_stochastic_mlp_loss_grad: obs_dim must be 1..32"
    m = _stochastic(w, obs_dim=33, stochastic_train_on_demand=True)
    b = _batch(3, obs_dim=33)
    w.decline, w.error, w.ensure_stochastic = 1, _refusal("Unsupported", text), True
    m.update(b, backend="hip")
    assert w.names() == ["opt_init", "construct", "step", "ensure_stochastic_train_instance", "step", "mean", "opt_step"]
    assert w.of("ensure_stochastic_train_instance")[0][1:] == (3, 4, 8, 21, 33) and m._last_update_route == "hip_stochastic_fused"
    # no build: a NoKernelInstance that carries the library's words -- torch under "auto", raised under "hip"
    w.events.clear()
    w.decline, w.ensure_stochastic = 1, False
    m.update(b)
    assert w.names() == ["step", "ensure_stochastic_train_instance", "loss_fn", "mean", "opt_step"] and m._last_update_route == "torch"
    w.decline = 1
    with pytest.raises(_lib.NoKernelInstance, match=r"obs_dim must be 1\.\.32"):
        m.update(b, backend="hip")
    # at 32 observations or fewer the same words are no missing instance: they propagate as they are
    narrow = _stochastic(w, stochastic_train_on_demand=True)
    w.events.clear()
    w.decline = 1
    with pytest.raises(_lib.Unsupported) as ei:
        narrow.update(_batch(3))
    assert ei.value is w.error and "ensure_stochastic_train_instance" not in w.names()
