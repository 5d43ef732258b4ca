"""loss.stochastic_loss_fn on the CPU in float64 at B = 2, L = 3, A = 3, C = 2, E = 4, support 8: the value against a
plain NumPy loop, the gradients against central differences, where the encoder's gradient comes from, what
sample_weight scales, and the refusal of a batch without per-step observations."""
import copy

import numpy as np
import pytest
import torch

import muax_amd as mx

B, L, A, CN, E, SUP, OD = 2, 3, 3, 2, 4, 8, 5
NAMES = ("representation", "prediction", "afterstate_dynamic", "afterstate_prediction", "chance_dynamic", "encoder")


@pytest.fixture(scope="module")
def case():
    g = torch.Generator().manual_seed(5)
    net = mx.create_stochastic_muzero_network(E, A, CN, 2 * SUP + 1, generator=g)
    m = mx.MuZero(net, policy="stochastic", support_size=SUP, device="cpu")
    m.init(0, np.zeros((1, OD)))
    for mod in net:
        mod.double()
        with torch.no_grad():
            for p in mod.parameters():  # (haiku's zero biases would hide every bias path)
                p.add_(0.1 * torch.randn(p.shape, generator=g, dtype=torch.float64))
    rng = np.random.default_rng(3)
    batch = mx.Transition(obs=rng.uniform(-1, 1, (B, L, OD)), a=rng.integers(0, A, (B, L)), r=rng.uniform(-2, 3, (B, L)),
                          Rn=rng.uniform(-20, 40, (B, L)), pi=rng.dirichlet(np.ones(A), (B, L)))
    return m, batch


# ---------------------------------------------------------------- the NumPy loop
def _np(p):
    return p.detach().numpy()


def _mlp2(m, x):
    h = x @ _np(m[0].w) + _np(m[0].b)
    h = np.where(h > 0, h, np.expm1(np.minimum(h, 0)))
    return h @ _np(m[1].w) + _np(m[1].b)


def _mmn(s):
    mn, mx_ = s.min(1, keepdims=True), s.max(1, keepdims=True)
    sc = mx_ - mn
    return (s - mn) / np.where(sc < 1e-5, sc + 1e-5, sc)


def _two_hot(x, S):
    x = np.sign(x) * (np.sqrt(np.abs(x) + 1) - 1) + 0.001 * x
    x = np.clip(x, -S, S)
    lo = np.floor(x)
    out = np.zeros(x.shape + (2 * S + 1,))
    for idx in np.ndindex(x.shape):
        k = int(lo[idx]) + S
        out[idx + (k,)] += 1 - (x[idx] - lo[idx])
        if k + 1 < 2 * S + 1:
            out[idx + (k + 1,)] += x[idx] - lo[idx]
    return out


def _ce(logits, labels):
    z = logits - logits.max(-1, keepdims=True)
    return -(labels * (z - np.log(np.exp(z).sum(-1, keepdims=True)))).sum(-1)


def numpy_loss(m, b, beta=0.25, sw=None, divide=False):
    rep, pred, ad, ap, cd, enc = m.network
    w = np.ones(B) if sw is None else np.asarray(sw, float)
    mean = lambda x: float((x * w).mean())  # noqa: E731
    onehot = lambda a, n: np.eye(n)[a]  # noqa: E731
    r_t, Rn_t = _two_hot(np.asarray(b.r, float), SUP), _two_hot(np.asarray(b.Rn, float), SUP)
    s = _mmn(b.obs[:, 0] @ _np(rep.repr_func.w) + _np(rep.repr_func.b))
    loss = mean(_ce(_mlp2(pred.v_func, s), Rn_t[:, 0])) + mean(_ce(_mlp2(pred.pi_func, s), b.pi[:, 0]))
    for i in range(1, L):
        e = _mlp2(enc.enc_func, b.obs[:, i])
        code = onehot(e.argmax(1), CN)
        after = _mmn(_mlp2(ad.as_func, np.concatenate([s, onehot(b.a[:, i - 1], A)], 1)))
        x = np.concatenate([after, code], 1)
        r, s = _mlp2(cd.r_func, x), _mmn(_mlp2(cd.ns_func, x))
        loss += (mean(_ce(r, r_t[:, i - 1])) + mean(_ce(_mlp2(pred.v_func, s), Rn_t[:, i]))
                 + mean(_ce(_mlp2(pred.pi_func, s), b.pi[:, i])) + mean(_ce(_mlp2(ap.pi_func, after), code))
                 + mean(_ce(_mlp2(ap.v_func, after), Rn_t[:, i - 1])) + beta * mean(((e - code) ** 2).mean(1)))
    if divide:
        loss /= L
    return loss + 1e-4 * 0.5 * sum(float((_np(p) ** 2).sum()) for mod in m.network for p in mod.parameters())


def test_loss_matches_numpy_loop(case):
    m, b = case
    assert mx.loss.stochastic_loss_fn(m, b).dtype == torch.float64
    for kw, kn in ((dict(), dict()), (dict(vqvae_beta=0.7), dict(beta=0.7)), (dict(divide_by_length=True), dict(divide=True)),
                   (dict(sample_weight=np.array([0.25, 1.75])), dict(sw=[0.25, 1.75]))):
        assert abs(float(mx.loss.stochastic_loss_fn(m, b, **kw)) - numpy_loss(m, b, **kn)) < 1e-10, kw


def test_it_is_the_default_loss_of_an_smz_model(case):
    m, b = case
    m2 = copy.deepcopy(m)
    m2._optimizer = mx.optimizers.create_optimizer("sgd", 0.0)
    assert abs(m2.update(b)["loss"] - numpy_loss(m, b)) < 1e-10
    with pytest.raises(ValueError, match="torch autograd only"):
        m2.update(b, backend="hip")


def test_gradients_match_central_differences(case, monkeypatch):
    """The five non-encoder modules (the loss is piecewise smooth in them: away from the encoder's argmax nothing
    switches).  The halved hidden-state gradient makes autograd's result differ from the loss's derivative on purpose, so
    the comparison runs with scale_gradient switched to the identity; the halving itself is the next test.  h = 1e-6 in
    float64: truncation ~ h^2 |f'''| ~ 1e-12, rounding ~ eps |f| / h ~ 1e-9 on a loss of order 10; the bound 1e-6
    (absolute, on gradients of order 1e-2 .. 1) leaves three decades."""
    m, b = case
    monkeypatch.setattr(mx.loss.mx_utils, "scale_gradient", lambda g, scale=1.0: g)
    for mod in m.network:
        mod.zero_grad()
    mx.loss.stochastic_loss_fn(m, b).backward()
    h = 1e-6
    rng = np.random.default_rng(0)
    for name, mod in zip(NAMES[:5], m.network[:5]):
        for p in mod.parameters():
            flat = p.data.view(-1)
            for k in rng.choice(flat.numel(), min(6, flat.numel()), replace=False):
                old = float(flat[k])
                flat[k] = old + h
                up = float(mx.loss.stochastic_loss_fn(m, b))
                flat[k] = old - h
                dn = float(mx.loss.stochastic_loss_fn(m, b))
                flat[k] = old
                assert abs((up - dn) / (2 * h) - float(p.grad.view(-1)[k])) < 1e-6, (name, tuple(p.shape), int(k))


def test_hidden_state_gradient_is_halved_before_each_afterstate_step(case, monkeypatch):
    """At L = 2 the representation's gradient is that of step 0's terms plus HALF of what the one transition sends back:
    g = g(L = 1) + (g(unscaled) - g(L = 1)) / 2, the L2 term being in both."""
    m, b = case
    cut = lambda n: mx.Transition(obs=b.obs[:, :n], a=b.a[:, :n], r=b.r[:, :n], Rn=b.Rn[:, :n], pi=b.pi[:, :n])  # noqa: E731

    def grads(batch):
        for mod in m.network:
            mod.zero_grad()
        mx.loss.stochastic_loss_fn(m, batch).backward()
        return [p.grad.clone() for p in m.network[0].parameters()]
    halved, first = grads(cut(2)), grads(cut(1))
    monkeypatch.setattr(mx.loss.mx_utils, "scale_gradient", lambda g, scale=1.0: g)
    whole = grads(cut(2))
    for h_, f, w in zip(halved, first, whole):
        assert (w - f).abs().max() > 1e-4 and torch.allclose(h_, f + 0.5 * (w - f), rtol=0, atol=1e-14)


def _encoder_grads(m, b, **kw):
    for mod in m.network:
        mod.zero_grad()
    mx.loss.stochastic_loss_fn(m, b, **kw).backward()
    return [p.grad.clone() for p in m.network[5].parameters()]


def test_where_the_encoder_gradient_comes_from(case):
    """Through the chance dynamics' input (the straight-through code) and through the commitment term; none through the
    chance cross entropy's target.  beta = 0 leaves the first; zeroing the chance dynamics' one-hot rows of both first
    layers as well leaves nothing but the L2 term -- the target's path, if there were one, would still be there."""
    m, b = case
    enc = list(m.network[5].parameters())
    l2 = [1e-4 * p.detach() for p in enc]
    full, no_commit = _encoder_grads(m, b), _encoder_grads(m, b, vqvae_beta=0.0)
    assert any((f - n).abs().max() > 1e-6 for f, n in zip(full, no_commit))        # the commitment term's share
    assert any((n - r).abs().max() > 1e-6 for n, r in zip(no_commit, l2))           # the straight-through share
    m2 = copy.deepcopy(m)
    with torch.no_grad():
        for f in (m2.network[4].r_func, m2.network[4].ns_func):
            f[0].w[E:] = 0.0
    rest = _encoder_grads(m2, b, vqvae_beta=0.0)
    for g, p in zip(rest, m2.network[5].parameters()):
        assert torch.allclose(g, 1e-4 * p.detach(), rtol=0, atol=1e-15)


def test_sample_weight_scales_the_rows_not_the_l2_term(case):
    m, b = case
    l2 = 1e-4 * 0.5 * sum(float((p.detach() ** 2).sum()) for mod in m.network for p in mod.parameters())
    one = float(mx.loss.stochastic_loss_fn(m, b))
    three = float(mx.loss.stochastic_loss_fn(m, b, sample_weight=torch.full((B,), 3.0)))
    assert abs((three - l2) - 3 * (one - l2)) < 1e-10
    rows = [float(mx.loss.stochastic_loss_fn(m, b, sample_weight=np.eye(B)[k])) - l2 for k in range(B)]
    assert abs(sum(rows) - (one - l2)) < 1e-10
    with pytest.raises(ValueError, match="sample_weight"):
        mx.loss.stochastic_loss_fn(m, b, sample_weight=np.ones(B + 1))


def test_short_observations_are_refused(case):
    m, b = case
    short = b._replace(obs=b.obs[:, :1]) if hasattr(b, "_replace") else mx.Transition(b.obs[:, :1], b.a, b.r, b.Rn, b.pi)
    with pytest.raises(ValueError, match="needs every step's observation"):
        mx.loss.stochastic_loss_fn(m, short)


def test_model_surface_without_a_gpu():
    net = mx.create_stochastic_muzero_network(E, A, CN, 2 * SUP + 1)
    assert mx.nn.is_default_stochastic_mlp(net) and not mx.nn.is_default_mlp_trio(net)
    m = mx.MuZero(net, device="cpu", support_size=SUP)
    params = m.init(0, np.zeros((1, OD)))
    assert params._fields == NAMES and all(len(p) > 0 for p in params)
    w = mx.nn.stochastic_mlp_weights(net)
    from muax_amd import _lib
    assert list(w) == _lib.STOCHASTIC_MLP_WEIGHT_NAMES
    assert tuple(w["ad_w1"].shape) == (E + A, 16) and tuple(w["ac_w2"].shape) == (16, CN) and tuple(w["cn_w1"].shape) == (E + CN, 16)
    trio = mx.create_muzero_network(mx.nn.Representation, mx.nn.Prediction, mx.nn.Dynamic, E, A, 2 * SUP + 1)
    with pytest.raises(NotImplementedError, match="SMZNetwork"):
        mx.MuZero(trio, policy="stochastic")
    with pytest.raises(ValueError):
        mx.MuZero(net, policy="gumbel")
    with pytest.raises(NotImplementedError, match="SMZNetwork"):
        m.save("unused")
