"""GPU tests of the fused training step (mzs_mlp_loss_grad, muax_amd/csrc/mz_train.cuh) at the edges of its inputs and
shapes, against fp64 CPU autograd of muax_amd/loss.py's formula (helpers.train_autograd, the reference of
test_gpu_train.py): value targets at the codec's integers and clip, policy targets whose mass is not 1, large logits,
ties and near-degenerate ranges in the min-max normaliser, the longest unroll the LDS admits and the first it refuses,
obs_dim 1 / 16, batches on either side of the 16-sample workgroup and one long enough for the reduction's in-order sums,
and the on-demand instance at every limit at once.

Bars (those of test_gpu_train.py): loss within 1e-5 relative of fp64, each gradient array within 2e-4 of its largest
fp64 entry, and a second call bit-identical.  They hold at every case here, the logits of about +-300 included, so
no case needs a bar relative to the torch fp32 route (whose errors _check prints beside the kernel's)."""
import copy

import numpy as np
import pytest
import torch

import muax_amd as mx
from helpers import support_edge_scalars, train_autograd, train_batch, train_model
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


def _weights(m):
    return mx.nn.mlp_trio_weights(m.network)


def _set(m, **arrays):
    w = _weights(m)
    with torch.no_grad():
        for n, v in arrays.items():
            w[n].copy_(torch.as_tensor(np.asarray(v), dtype=torch.float32))


def _rel_errors(views, ref):
    return [float(np.abs(g - d).max() / max(np.abs(d).max(), 1e-6)) for g, d in zip(views, ref)]


def _check(m, b, capture=None, **kw):
    """The kernel's loss and gradients against fp64 autograd; returns (loss error, worst gradient error) relative,
    for the kernel and for the torch fp32 route."""
    fused = mx.loss.FusedLossGrad(m)
    loss, flat = fused(b, **kw)
    loss, views = float(loss.item()), [v.detach().cpu().double().numpy() for v in fused.views]
    flat = flat.clone()
    l64, g64 = train_autograd(m, b, torch.float64, "cpu", capture=capture, **kw)
    l32, g32 = train_autograd(m, b, torch.float32, "cuda", **kw)
    assert all(np.isfinite(v).all() for v in views) and np.isfinite(loss)
    ek, et = _rel_errors(views, g64), _rel_errors(g32, g64)
    lk, lt = abs(loss - l64) / abs(l64), abs(l32 - l64) / abs(l64)
    for n, gh, gd, e_k, e_t in zip(MLP_WEIGHT_NAMES, views, g64, ek, et):
        assert gh.shape == gd.shape
        assert e_k <= 2e-4, (n, e_k, e_t)
    assert lk <= 1e-5, (loss, l64, l32)
    loss2, flat2 = fused(b, **kw)  # fixed-order reduction: bit-reproducible
    assert float(loss2.item()) == loss and torch.equal(flat2, flat)
    print(f"[kernel loss {lk:.1e} grad {max(ek):.1e} | torch fp32 loss {lt:.1e} grad {max(et):.1e}]", end=" ")
    return lk, max(ek), lt, max(et)


# ---- a. value targets: 0, +-1, h(x) on / one ulp either side of an integer, the clip, far beyond it ----
@pytest.mark.parametrize("support", [10, 15, 20])
def test_value_targets_at_codec_edges(support):
    x = support_edge_scalars(support)
    B, L = len(x), 2
    m, b = train_model(2, 8, 4, seed=support, support=support), train_batch(B, L, 2, 4, seed=support)
    b.r[:] = np.stack([x, x[::-1]], 1)
    b.Rn[:] = np.stack([np.roll(x, 7), -x], 1)
    _check(m, b)


# ---- b. policy targets whose mass is not spread over every action, or is not 1 ----
def test_policy_targets_one_hot_zero_and_unnormalised():
    """One-hot rows, rows with zeros, all-zero rows (padded steps: no loss, no gradient) and rows summing to 0.5 / 3:
    the kernel's cross entropy is T lse - sum t l with T = sum t, its logit gradient p T - t."""
    A, B, L = 4, 40, 3
    m, b = train_model(A, 8, 4, seed=11), train_batch(B, L, A, 4, seed=11)
    rng = np.random.default_rng(1)
    pi = np.zeros((B, L, A), F32)
    for i in range(B):
        for t in range(L):
            kind = (i + t) % 5
            if kind == 0:
                pi[i, t, rng.integers(A)] = 1.0
            elif kind == 1:
                row = rng.dirichlet(np.ones(A)).astype(F32)
                row[rng.choice(A, 2, replace=False)] = 0.0
                pi[i, t] = row / row.sum()
            elif kind == 3:
                pi[i, t] = 0.5 * rng.dirichlet(np.ones(A))
            elif kind == 4:
                pi[i, t] = 3.0 * rng.dirichlet(np.ones(A))
    b.pi[:] = pi.reshape(B, L, 1, A)
    _check(m, b)
    # all-zero policy rows are padding: they change neither the loss nor the gradient beyond the other two heads
    b0 = copy.deepcopy(b)
    b0.pi[:] = 0.0
    f = mx.loss.FusedLossGrad(m)
    l0 = float(f(b0)[0].item())
    l64, _ = train_autograd(m, b0, torch.float64, "cpu")
    assert abs(l0 - l64) <= 1e-5 * abs(l64)


# ---- c. large logits ----
@pytest.mark.parametrize("reach", [50.0, 300.0])
def test_large_logits(reach):
    """Head output layers scaled until the logits reach about +-reach: at 300 the softmax's exp is 0 below -87 for
    most bins, and the bars still hold."""
    m, b = train_model(2, 8, 4, seed=3), train_batch(48, 3, 2, 4, seed=3)
    w = _weights(m)
    with torch.no_grad():
        s = m.repr_func(torch.as_tensor(b.obs[:, 0], device="cuda"))
        v, lg = m.pred_func(s)
        r, _ = m.dy_func(s, torch.as_tensor(b.a[:, 0], device="cuda"))
        for (wn, bn), out in ((("pv_w2", "pv_b2"), v), (("pp_w2", "pp_b2"), lg), (("dr_w2", "dr_b2"), r)):
            f = reach / float(out.abs().max())
            w[wn].mul_(f)
            w[bn].mul_(f)
        v, lg = m.pred_func(s)
    assert 0.7 * reach <= float(v.abs().max()) <= 1.3 * reach
    _check(m, b)


# ---- d. ties and near-degenerate ranges in the min-max normaliser ----
def _ties(u, cols):
    return bool((u[:, cols] == u[:, cols[:1]]).all())


def test_fresh_net_on_all_zero_observations_ties_every_entry():
    """Zero biases (haiku's init) and all-zero first observations: the E entries of obs W + b all tie, c = 0 takes the
    +1e-5 branch, and every entry is both the min and the max."""
    m, b = train_model(2, 8, 4, seed=21, bias_noise=False), train_batch(32, 4, 2, 4, seed=21)
    b.obs[:, 0] = 0.0
    cap = []
    _check(m, b, capture=cap)
    assert _ties(cap[0].numpy(), list(range(8))) and float(cap[0].abs().max()) == 0.0


def _dyadic(rng, shape, step, lim):
    return (rng.integers(-int(lim / step), int(lim / step) + 1, shape) * step).astype(F32)


def test_duplicated_representation_columns_tie_at_min_and_max():
    """repr_w columns 0 / 1 and 2 / 3 duplicated (with their biases) far below / above the rest; observations and
    weights dyadic, so that obs W + b is exact and the ties hold in fp32 and fp64 alike."""
    E, od = 8, 4
    m, b = train_model(2, E, od, seed=23), train_batch(40, 3, 2, od, seed=23)
    rng = np.random.default_rng(5)
    W, bias = _dyadic(rng, (od, E), 1 / 16, 0.5), _dyadic(rng, E, 1 / 16, 0.5)
    W[:, 1], W[:, 3] = W[:, 0], W[:, 2]
    bias[:2], bias[2:4] = -6.0, 6.0
    b.obs[:] = _dyadic(rng, b.obs.shape, 1 / 8, 1.0)
    _set(m, repr_w=W, repr_b=bias)
    cap = []
    _check(m, b, capture=cap)
    u = cap[0].numpy()
    assert _ties(u, [0, 1]) and _ties(u, [2, 3])
    assert (u[:, 0] == u.min(1)).all() and (u[:, 2] == u.max(1)).all()


def test_duplicated_dynamics_columns_tie_in_every_step():
    """dn_w2 columns 0 / 1 and 2 / 3 duplicated (with their biases) below / above the rest: the next state's min and
    max tie at every unroll step."""
    E, L = 8, 5
    m, b = train_model(2, E, 4, seed=27), train_batch(36, L, 2, 4, seed=27)
    w = {n: t.detach().cpu().numpy().copy() for n, t in _weights(m).items()}
    W2, b2 = w["dn_w2"], w["dn_b2"]
    W2[:, 1], W2[:, 3] = W2[:, 0], W2[:, 2]
    b2[:2], b2[2:4] = -20.0, 20.0
    _set(m, dn_w2=W2, dn_b2=b2)
    cap = []
    _check(m, b, capture=cap)
    assert len(cap) == L + 1  # the representation's, then one per dynamics step (the last next state is unused)
    for u in cap[1:]:
        u = u.numpy()
        assert _ties(u, [0, 1]) and _ties(u, [2, 3])
        assert (u[:, 0] == u.min(1)).all() and (u[:, 2] == u.max(1)).all()


@pytest.mark.parametrize("log2_range", [-18, -16])
def test_near_degenerate_representation_range(log2_range):
    """Rows whose range is 2^-18 (below 1e-5: the +1e-5 branch) or 2^-16 (above it): repr_w's columns equal and
    dyadic, the biases 0.25 + range * (dyadic fractions), so that every row's range is exactly 2^log2_range in both
    precisions and fp32 and fp64 take the same branch."""
    E, od = 8, 4
    m, b = train_model(2, E, od, seed=29), train_batch(32, 3, 2, od, seed=29)
    rng = np.random.default_rng(7)
    col = _dyadic(rng, od, 1 / 64, 0.5)
    W = np.repeat(col[:, None], E, 1)
    c = 2.0 ** log2_range
    bias = (0.25 + c * np.array([0, 1, .5, .25, .75, .125, .375, .625])).astype(F32)
    b.obs[:] = _dyadic(rng, b.obs.shape, 1 / 8, 1.0)
    _set(m, repr_w=W, repr_b=bias)
    cap = []
    _check(m, b, capture=cap)
    u = cap[0].numpy()
    assert ((u.max(1) - u.min(1)) == c).all() and (c < 1e-5) == (log2_range == -18)


# ---- e. shape limits ----
@pytest.mark.parametrize("A,E", [(2, 8), (4, 32)])
def test_unroll_length_limits(A, E):
    """L = 1 and the longest unroll the LDS admits (computed here from the layout, independently of the launcher) match
    fp64; one step longer is refused on the host with the limit named, and update() then takes the torch route under
    backend="auto" and raises under backend="hip"."""
    Lmax = lds_max_unroll(A, E, 21)
    assert (A, E, Lmax) in ((2, 8, 150), (4, 32, 71))
    for L in (1, Lmax):
        _check(train_model(A, E, 4, seed=L), train_batch(20, L, A, 4, seed=L))
    b = train_batch(20, Lmax + 1, A, 4, seed=1)
    m = train_model(A, E, 4, seed=1)
    with pytest.raises(ValueError, match=f"unroll_steps {Lmax + 1} too large for the LDS \\(at most {Lmax} "):
        mx.loss.FusedLossGrad(m)(b)
    with pytest.raises(ValueError, match=f"at most {Lmax} "):
        train_model(A, E, 4, seed=1).update(b, backend="hip")
    mt = train_model(A, E, 4, seed=1)
    la, lt = m.update(b)["loss"], mt.update(b, backend="torch")["loss"]
    assert np.isclose(la, lt, rtol=1e-6)
    for p, q in zip([p for mod in m.network for p in mod.parameters()], [p for mod in mt.network for p in mod.parameters()]):
        assert torch.allclose(p, q, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("obs_dim", [1, 16])
def test_obs_dim_limits(obs_dim):
    _check(train_model(2, 8, obs_dim, seed=obs_dim), train_batch(33, 3, 2, obs_dim, seed=obs_dim))


@pytest.mark.parametrize("B", [1, 15, 16, 17, 63, 65])
def test_batch_sizes_around_the_workgroup(B):
    _check(train_model(2, 8, 4, seed=B), train_batch(B, 3, 2, 4, seed=B))


def test_large_batch_reduction():
    """B = 65536: 16384 wavefront partials per gradient entry, 2048 in-order sums per reduction group."""
    _check(train_model(2, 8, 4, seed=9), train_batch(65536, 2, 2, 4, seed=9))


def test_on_demand_instance_at_every_limit():
    """(A, E, F) = (16, 64, 63), the on-demand instance at the largest action count, embedding and support it builds,
    at the longest unroll its LDS admits; one step longer is refused by the on-demand launcher too."""
    from muax_amd import _jit
    A, E, F = 16, 64, 63
    Lmax = lds_max_unroll(A, E, F)
    assert Lmax == 31
    assert _jit.ensure_train_instance(A, E, F)
    _check(train_model(A, E, 16, seed=31, support=31), train_batch(20, Lmax, A, 16, seed=31))
    with pytest.raises(ValueError, match=f"at most {Lmax} "):
        mx.loss.FusedLossGrad(train_model(A, E, 16, seed=31, support=31))(train_batch(20, Lmax + 1, A, 16, seed=3))


# ---- f. end to end ----
@pytest.mark.parametrize("opt,lr", [("adam", 1e-2), ("sgd", 1e-6)])
def test_fresh_model_on_all_zero_observations_routes_take_the_same_steps(opt, lr):
    """A fresh model (zero biases) on a batch whose first observations are all zero: every embedding entry ties in the
    first step (c = 0, so its gradient is about 1e5 times the others).  Ten update() steps of the HIP and the torch
    routes end at the same parameters, within the tolerances of test_update_hip_and_torch_routes_take_the_same_step.
    Adam's first step moves every entry by about +-lr whatever its gradient, which hides most of the tie rule; under
    SGD the step is the gradient itself, and a route that gave a tie's whole share to one index would be 2e-2 away."""
    b = train_batch(256, 6, 2, 4, seed=13)
    b.obs[:, 0] = 0.0
    out = {}
    for backend in ("hip", "torch"):
        m = train_model(2, 8, 4, seed=17, bias_noise=False, optimizer=(opt, lr))
        losses = [m.update(b, backend=backend)["loss"] for _ in range(10)]
        out[backend] = (losses, torch.cat([p.detach().reshape(-1) for mod in m.network for p in mod.parameters()]).cpu())
    assert np.allclose(out["hip"][0], out["torch"][0], rtol=2e-4)
    assert torch.allclose(out["hip"][1], out["torch"][1], rtol=5e-3, atol=5e-4)
