"""The fused stochastic training step without a GPU: the parameter count of the C entry, the model flag on a CPU model,
and the float64 reference of tests/stochastic_train_reference.py against central differences of an independent NumPy
loop (tests/test_stochastic_loss_cpu.py::numpy_loss) at that file's tiny shape."""
import ctypes

import numpy as np
import pytest
import torch

import muax_amd as mx
import stochastic_train_reference as ref
from muax_amd import _lib
from test_stochastic_loss_cpu import A, B, CN, E, L, OD, SUP, numpy_loss


def test_num_params_is_the_summed_numel():
    lib = _lib.load(build_if_missing=True)  # (loads without a device, as in test_host_cpu.py)
    for a, c, e, s, od in ref.SHAPES + [(4, 32, 32, 31, 16)]:
        m = ref.smz_model(a, c, e, s, od, seed=1, device="cpu")
        w = mx.nn.stochastic_train_weights(m.network)
        assert list(w) == _lib.STOCHASTIC_TRAIN_WEIGHT_NAMES and len(w) == 34
        n = sum(t.numel() for t in w.values())
        assert n == sum(p.numel() for mod in m.network for p in mod.parameters())
        assert lib.mzs_stochastic_mlp_num_params(od, e, a, c, s) == n
        assert lib.mzs_stochastic_mlp_train_workspace_bytes(17, od, e, a, c, s) == 8 * (n + 1) * 4
    assert ctypes.sizeof(_lib.MzsStochasticTrainWeights) == 16 + 34 * 8
    assert ctypes.sizeof(_lib.MzsStochasticTrainArgs) == 32 + 6 * 8 + 16 + 3 * 8 + 8


def test_flag_is_accepted_on_a_cpu_model_and_the_torch_route_runs():
    m = ref.smz_model(A, CN, E, SUP, OD, seed=2, device="cpu", stochastic_fused_update=True)
    assert m.stochastic_fused_update and m._last_update_route is None
    b = ref.smz_batch(B, L, A, OD, seed=2)
    assert np.isfinite(m.update(b)["loss"]) and m._last_update_route == "torch"
    assert np.isfinite(m.update(b, backend="auto", vqvae_beta=0.5)["loss"]) and m._last_update_route == "torch"
    with pytest.raises(ValueError, match="torch autograd only"):
        m.update(b, backend="hip")
    off = ref.smz_model(A, CN, E, SUP, OD, seed=2, device="cpu")
    assert not off.stochastic_fused_update
    off.update(b)
    assert off._last_update_route == "torch"


def test_reference_matches_central_differences_of_the_numpy_loop(monkeypatch):
    """The 30 non-encoder arrays (the loss is piecewise smooth in them; the encoder's straight-through gradient is not a
    derivative of the loss), scale_gradient switched to the identity as in test_stochastic_loss_cpu.py.  h = 1e-6 in
    float64: truncation ~ h^2, rounding ~ eps |f| / h ~ 1e-9; the bound is that file's 1e-6 absolute."""
    monkeypatch.setattr(mx.loss.mx_utils, "scale_gradient", lambda g, scale=1.0: g)
    m = ref.smz_model(A, CN, E, SUP, OD, seed=5, device="cpu")
    b32 = ref.smz_batch(B, L, A, OD, seed=3)
    b = mx.Transition(obs=b32.obs.astype(np.float64), a=b32.a, r=b32.r.astype(np.float64), Rn=b32.Rn.astype(np.float64),
                      pi=b32.pi.astype(np.float64).reshape(B, L, A))
    loss, grads = ref.autograd(m, b)
    m64 = ref.copy_model(m)
    assert abs(loss - numpy_loss(m64, b)) < 1e-10
    w = mx.nn.stochastic_train_weights(m64.network)
    rng = np.random.default_rng(0)
    h = 1e-6
    for name, g in zip(_lib.STOCHASTIC_TRAIN_WEIGHT_NAMES, grads):
        if name.startswith("en_"):
            continue
        flat = w[name].data.view(-1)
        for k in rng.choice(flat.numel(), min(4, flat.numel()), replace=False):
            old = float(flat[k])
            flat[k] = old + h
            up = numpy_loss(m64, b)
            flat[k] = old - h
            dn = numpy_loss(m64, b)
            flat[k] = old
            assert abs((up - dn) / (2 * h) - g.reshape(-1)[k]) < 1e-6, (name, int(k))


def test_conditions_report_what_they_say():
    """The condition helper on a batch whose numbers are known: an integer scaled target, a tied normaliser input."""
    m = ref.smz_model(A, CN, E, SUP, OD, seed=5, device="cpu")
    b = ref.smz_batch(B, L, A, OD, seed=3)
    c = ref.conditions(m, b)
    assert c["encoder_gap"].shape == (B, L - 1) and c["minmax_gap"].shape == (B, 2 * L - 1)
    assert c["target_distance"].shape == (B, 2 * L) and (c["encoder_gap"] >= 0).all() and (c["minmax_gap"] >= 0).all()
    b.r[0, 0] = 0.0  # h(0) = 0, an integer
    b.obs[1, 0] = 0.0  # the representation's pre-activation is its bias; make two entries the smallest
    with torch.no_grad():
        m.repr_func.repr_func.b[:2] = -5.0
    c = ref.conditions(m, b)
    assert c["target_distance"][0, 0] == 0.0 and c["minmax_gap"][1, 0] == 0.0 and not ref.well_conditioned(c)
