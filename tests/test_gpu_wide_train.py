"""GPU tests of the fused training step (mzs_mlp_loss_grad, muax_amd/csrc/mz_train.cuh) for 17 to 64 actions -- the
on-demand instances of muax_amd/_jit.py::ensure_wide_train_instance, policy head over ceil(A / 16) lane slots -- and for
observations up to 128 wide, against fp64 CPU autograd of muax_amd/loss.py's formula (helpers.train_autograd).

Bars (those of test_gpu_train.py and test_gpu_train_edges.py): loss within 1e-5 relative of fp64, each of the 18
gradient arrays within 2e-4 of its largest fp64 entry, and a second call bit-identical.  _check prints the torch fp32
route's errors beside the kernel's."""
import warnings

import numpy as np
import pytest
import torch

import muax_amd as mx
from helpers import train_autograd, train_batch, train_model
from muax_amd import _jit
from muax_amd._lib import MLP_WEIGHT_NAMES

pytestmark = pytest.mark.gpu
F32 = np.float32
LDS_BYTES = 160 * 1024  # dynamic LDS one workgroup may take
SAMPLES_PER_WORKGROUP = 16


def lds_max_unroll(A, E, F, H=16):
    """Longest unroll whose workgroup fits LDS_BYTES: the eight head / dynamics layers as [K][16 ceil(N / 16) + 1] fp32
    blocks, each followed by its bias padded to a multiple of 16 (in all rounded up to 4 words), plus 16 ceil(E / 16)
    words of kept hidden state per sample and step."""
    def up16(n):
        return 16 * -(-n // 16)
    X = E + A
    layers = [(E, H), (H, F), (E, H), (H, A), (X, H), (H, F), (X, H), (H, E)]
    words = sum(k * (up16(n) + 1) + up16(n) for k, n in layers)
    words = 4 * -(-words // 4)
    return (LDS_BYTES // 4 - words) // (SAMPLES_PER_WORKGROUP * up16(E))


def _fused(m):
    """FusedLossGrad of the model, its wide instance registered first (update() does that itself)."""
    f = mx.loss.FusedLossGrad(m)
    if f.A > 16:
        assert _jit.ensure_wide_train_instance(f.A, f.E, 2 * f.S + 1), _jit.build_log_tail()
    return f


def _rel_errors(views, ref):
    return [float(np.abs(g - d).max() / max(np.abs(d).max(), 1e-6)) for g, d in zip(views, ref)]


def _check(m, b, **kw):
    """The kernel's loss and gradients against fp64 autograd, and a second call bit-identical; prints (loss error,
    worst gradient error), relative, for the kernel and for the torch fp32 route."""
    fused = _fused(m)
    loss, flat = fused(b, **kw)
    loss, views = float(loss.item()), [v.detach().cpu().double().numpy() for v in fused.views]
    flat = flat.clone()
    l64, g64 = train_autograd(m, b, torch.float64, "cpu", **kw)
    l32, g32 = train_autograd(m, b, torch.float32, "cuda", **kw)
    ek, et = _rel_errors(views, g64), _rel_errors(g32, g64)
    lk, lt = abs(loss - l64) / abs(l64), abs(l32 - l64) / abs(l64)
    print(f"[kernel loss {lk:.1e} grad {max(ek):.1e} | torch fp32 loss {lt:.1e} grad {max(et):.1e}]", end=" ")
    assert all(np.isfinite(v).all() for v in views) and np.isfinite(loss)
    for n, gh, gd, e_k, e_t in zip(MLP_WEIGHT_NAMES, views, g64, ek, et):
        assert gh.shape == gd.shape
        assert e_k <= 2e-4, (n, e_k, e_t)
    assert lk <= 1e-5, (loss, l64, l32)
    loss2, flat2 = fused(b, **kw)  # fixed-order reduction: bit-reproducible
    assert float(loss2.item()) == loss and torch.equal(flat2, flat)
    return lk, max(ek), lt, max(et)


# ---- a. every slot count of the policy head, the embedding and the observation, both sides of each slot edge ----
@pytest.mark.parametrize("A,E,obs_dim", [(17, 8, 4), (18, 8, 128), (18, 32, 8), (32, 16, 16), (33, 8, 4), (48, 8, 17),
                                         (64, 64, 16)])
def test_wide_shapes_match_fp64(A, E, obs_dim):
    seed = A + E + obs_dim
    _check(train_model(A, E, obs_dim, seed=seed, support=31), train_batch(40, 3, A, obs_dim, seed=seed))


# ---- b. policy targets whose mass sits in one slot, or is not 1; large policy logits ----
@pytest.mark.parametrize("A,E,obs_dim", [(18, 8, 128), (33, 8, 4), (64, 64, 16)])
def test_policy_targets_per_slot_and_large_logits(A, E, obs_dim):
    """Rows with all mass on action 0, on action A - 1, on an action of each 16-lane slot, all-zero rows (padded steps)
    and rows of mass 3; then the same batch with pp_w2 / pp_b2 scaled until the policy logits reach about +-50."""
    B, L, slots = 48, 3, -(-A // 16)
    m, b = train_model(A, E, obs_dim, seed=A, support=31), train_batch(B, L, A, obs_dim, seed=A)
    rng = np.random.default_rng(A)
    pi = np.zeros((B, L, A), F32)
    seen = set()
    for i in range(B):
        for t in range(L):
            kind = (i + t) % (4 + slots)
            if kind == 0:
                pi[i, t, 0] = 1.0
            elif kind == 1:
                pi[i, t, A - 1] = 1.0
            elif kind == 2:
                pass
            elif kind == 3:
                pi[i, t] = 3.0 * rng.dirichlet(np.ones(A))
            else:
                s = kind - 4
                a = int(rng.integers(16 * s, min(A, 16 * s + 16)))
                seen.add(a // 16)
                pi[i, t, a] = 1.0
    assert seen == set(range(slots))
    b.pi[:] = pi.reshape(B, L, 1, A)
    _check(m, b)
    w = mx.nn.mlp_trio_weights(m.network)
    with torch.no_grad():
        s = m.repr_func(torch.as_tensor(b.obs[:, 0], device="cuda"))
        f = 50.0 / float(m.pred_func(s)[1].abs().max())
        w["pp_w2"].mul_(f)
        w["pp_b2"].mul_(f)
        reach = float(m.pred_func(s)[1].abs().max())
    assert 35.0 <= reach <= 65.0
    _check(m, b)


# ---- c. observation widths on either side of each 16-feature slot, at a shape the library lists ----
@pytest.mark.parametrize("obs_dim", [1, 16, 17, 32, 127, 128])
def test_observation_widths_on_a_listed_instance(obs_dim):
    _check(train_model(2, 8, obs_dim, seed=obs_dim), train_batch(33, 3, 2, obs_dim, seed=obs_dim))


def test_observation_width_129_is_refused_with_the_limit_named():
    m, b = train_model(2, 8, 129, seed=1), train_batch(20, 2, 2, 129, seed=1)
    with pytest.raises(ValueError, match=r"obs_dim must be 1\.\.128"):
        mx.loss.FusedLossGrad(m)(b)
    with pytest.raises(ValueError):
        train_model(2, 8, 129, seed=1).update(b, backend="hip")
    mt = train_model(2, 8, 129, seed=1)
    la, lt = m.update(b)["loss"], mt.update(b, backend="torch")["loss"]  # auto: the torch route
    assert np.isclose(la, lt, rtol=1e-6)


# ---- d. unroll lengths ----
@pytest.mark.parametrize("A,E,support,obs_dim", [(18, 8, 10, 4), (64, 64, 31, 16)])
def test_unroll_length_limits(A, E, support, obs_dim):
    """L = 1 and the longest unroll the LDS admits (from the layout formula, independently of the launcher) match fp64;
    one step longer is refused on the host with the limit named, and update() then takes the torch route under
    backend="auto" and raises under backend="hip"."""
    F = 2 * support + 1
    Lmax = lds_max_unroll(A, E, F)
    assert (A, E, Lmax) in ((18, 8, 147), (64, 64, 29))
    for L in (1, Lmax):
        _check(train_model(A, E, obs_dim, seed=L, support=support), train_batch(20, L, A, obs_dim, seed=L))
    b = train_batch(20, Lmax + 1, A, obs_dim, seed=1)
    m = train_model(A, E, obs_dim, seed=1, support=support)
    with pytest.raises(ValueError, match=f"unroll_steps {Lmax + 1} too large for the LDS \\(at most {Lmax} "):
        _fused(m)(b)
    with pytest.raises(ValueError, match=f"at most {Lmax} "):
        train_model(A, E, obs_dim, seed=1, support=support).update(b, backend="hip")
    mt = train_model(A, E, obs_dim, seed=1, support=support)
    la, lt = m.update(b)["loss"], mt.update(b, backend="torch")["loss"]
    assert np.isclose(la, lt, rtol=1e-6)
    for p, q in zip([p for mod in m.network for p in mod.parameters()], [p for mod in mt.network for p in mod.parameters()]):
        assert torch.allclose(p, q, rtol=1e-6, atol=1e-7)


# ---- e. batch sizes ----
@pytest.mark.parametrize("B", [1, 17, 4096])
def test_batch_sizes(B):
    _check(train_model(18, 8, 4, seed=B, support=31), train_batch(B, 3, 18, 4, seed=B))


# ---- f. end to end ----
@pytest.mark.parametrize("opt,lr", [("adam", 1e-2), ("sgd", 1e-2)])
def test_update_routes_take_the_same_steps(opt, lr):
    """Ten update() steps of the HIP and the torch routes from the same fresh 18-action model end at the same
    parameters, within the tolerances of test_fresh_model_on_all_zero_observations_routes_take_the_same_steps."""
    b = train_batch(256, 6, 18, 4, seed=13)
    out = {}
    for backend in ("hip", "torch"):
        m = train_model(18, 8, 4, seed=17, bias_noise=False, optimizer=(opt, lr))
        losses = [m.update(b, backend=backend)["loss"] for _ in range(10)]
        out[backend] = (losses, torch.cat([p.detach().reshape(-1) for mod in m.network for p in mod.parameters()]).cpu())
    assert out["hip"][0][-1] < out["hip"][0][0]
    assert np.allclose(out["hip"][0], out["torch"][0], rtol=2e-4)
    assert torch.allclose(out["hip"][1], out["torch"][1], rtol=5e-3, atol=5e-4)


def test_act_update_act_stays_on_the_library(monkeypatch):
    """One 18-action model: act() on the wide-action kernel, update(backend="hip") on the wide training instance, act()
    again -- warnings as errors and the generic search route switched off, so neither the step-wise search nor the
    torch route can stand in.  The second act equals that of a fresh model given the updated weights."""
    monkeypatch.setenv("MUAX_AMD_GENERIC", "0")
    A, E, obs_dim, S, B = 18, 8, 6, 30, 45
    m = train_model(A, E, obs_dim, seed=5)
    obs = np.random.default_rng(B).uniform(-1, 1, (B, obs_dim)).astype(F32)
    key = mx.prng.PRNGKey(4321)
    kw = dict(with_pi=True, with_value=True, obs_from_batch=True, num_simulations=S)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        first = m.act(key, obs, **kw)
        before = [p.detach().clone() for mod in m.network for p in mod.parameters()]
        loss = m.update(train_batch(64, 5, A, obs_dim, seed=3), backend="hip")["loss"]
        second = m.act(key, obs, **kw)
    assert np.isfinite(loss)
    assert any(not torch.equal(p, q) for p, q in zip(before, [p for mod in m.network for p in mod.parameters()]))
    fresh = train_model(A, E, obs_dim, seed=99)
    with torch.no_grad():
        for (n, p), q in zip(mx.nn.mlp_trio_weights(fresh.network).items(), mx.nn.mlp_trio_weights(m.network).values()):
            p.copy_(q)
    fresh.weights_changed()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        third = fresh.act(key, obs, **kw)
    for x, y in zip(second, third):
        assert np.array_equal(x, y)
    assert not all(np.array_equal(x, y) for x, y in zip(first, second))  # the update was seen by the search
