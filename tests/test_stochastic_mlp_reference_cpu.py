"""tests/stochastic_mlp_reference.py (the decision and the chance function composed from the oracle's own
recurrent_inference) against the float64 torch modules of nn.create_stochastic_muzero_network, at the shapes of the GPU
kernel test.  The tolerance is derived, not measured: a running first-order bound on the fp32 evaluation's error,
carried through the float64 evaluation layer by layer (u = 2^-24, the fp32 unit round-off):

  linear   y = x W + b by an n-term fma chain and one add: |dy| <= |dx| |W| + (n + 1) u (|x| |W| + |b|)  (the classic
           gamma_{n+1} bound, first order) -- a few ulps of the largest term of each output;
  elu      1-Lipschitz, evaluated by the spec to 4 ulps: |de| <= |dh| + 4 u |e|;
  min-max  y = (x - min) / scale in [0, 1]: numerator and scale each carry 2 max|dx| and one rounding, the division one
           more: |dy| <= 4 max|dx| / scale + 3 u;
  decode   h = sum_j (j - S) softmax(l)_j, x = inv_scaling(h).  A logit error d moves the softmax by ||dp||_1 <=
           exp(2 d) - 1, hence h by S times that; the fp32 softmax itself (exp to 2 ulps, a sum of F terms, a division,
           then F products summed) adds S (F + 16) u.  inv_scaling in fp32 (oracle/mz_oracle.c) computes
           e = (sqrt(1 + 0.004 (|h| + 1.001)) - 1) / 0.002: the three roundings before the subtraction, each about u, are
           divided by 0.002, so |de| <= 1500 u; x = e^2 - 1 with e = sqrt(|x| + 1).  The propagated part goes through the
           inverse's slope 1 / h'(x) <= 2 sqrt(|x| + 1), the same factor: |dx| <= 2 sqrt(|x| + 1) (|dh| + 1500 u) + 2 u (|x| + 1).

The decoded values are compared through the same bound.  The reference must also sit well INSIDE the bound on average
(it is a bound, not an estimate): the test prints the largest ratio."""
import numpy as np
import pytest
import torch

import muax_amd as mx
import stochastic_mlp_reference as smr

U = 2.0 ** -24
SHAPES = [(4, 3, 5, 8, 3), (4, 32, 16, 10, 7), (18, 40, 64, 31, 5), (2, 2, 70, 10, 2), (1, 1, 1, 8, 1)]


def _lin(x, dx, W, b):
    return x @ W + b, dx @ np.abs(W) + (W.shape[0] + 1) * U * (np.abs(x) @ np.abs(W) + np.abs(b))


def _mlp2(w, h, x, dx):
    a, da = _lin(x, dx, w[h + "_w1"], w[h + "_b1"])
    e = np.where(a > 0, a, np.expm1(np.minimum(a, 0)))
    return _lin(e, da + 4 * U * np.abs(e), w[h + "_w2"], w[h + "_b2"])


def _mmn(x, dx):
    mn, sc = x.min(1, keepdims=True), x.max(1, keepdims=True) - x.min(1, keepdims=True)
    sc = np.where(sc < 1e-5, sc + 1e-5, sc)
    return (x - mn) / sc, np.broadcast_to(4 * dx.max(1, keepdims=True) / sc + 3 * U, x.shape)


def _decode(logits, dl, S):
    F = logits.shape[1]
    z = np.exp(logits - logits.max(1, keepdims=True))
    h = (np.arange(-S, S + 1) * z / z.sum(1, keepdims=True)).sum(1)
    x = np.sign(h) * (((np.sqrt(1 + 4 * 0.001 * (np.abs(h) + 1 + 0.001)) - 1) / 0.002) ** 2 - 1)
    dh = S * np.expm1(2 * dl.max(1)) + S * (F + 16) * U
    return x, 2 * np.sqrt(np.abs(x) + 1) * (dh + 1500 * U) + 2 * U * (np.abs(x) + 1)


def _bounds(w32, A, Cn, E, S, emb, action, outcome):
    """float64 values and error bounds of both functions on the rows of `emb`."""
    w = {k: v.astype(np.float64) for k, v in w32.items()}
    x = emb.astype(np.float64)
    sa = np.concatenate([x, np.eye(A)[action]], 1)
    after = _mmn(*_mlp2(w, "ad", sa, np.zeros_like(sa)))
    dec = dict(afterstate=after, chance_logits=_mlp2(w, "ac", *after), afterstate_value=_decode(*_mlp2(w, "av", *after), S))
    sc = np.concatenate([x, np.eye(Cn)[outcome]], 1)
    state = _mmn(*_mlp2(w, "cn", sc, np.zeros_like(sc)))
    cha = dict(state=state, reward=_decode(*_mlp2(w, "cr", sc, np.zeros_like(sc)), S), action_logits=_mlp2(w, "pp", *state),
               value=_decode(*_mlp2(w, "pv", *state), S))
    return dec, cha


def _modules(w32, A, Cn, E, S):
    """The family's torch modules in float64 holding the weights `w32`."""
    net = mx.create_stochastic_muzero_network(E, A, Cn, 2 * S + 1)
    m = mx.MuZero(net, device="cpu", support_size=S, discount=0.97)
    m.init(0, np.zeros((1, 3)))
    with torch.no_grad():
        for mod in net:
            mod.double()
        for k, p in mx.nn.stochastic_mlp_weights(net).items():
            p.copy_(torch.from_numpy(w32[k].astype(np.float64)))
    return m


@pytest.mark.parametrize("A,Cn,E,S,B", SHAPES)
def test_reference_matches_fp64_modules_within_the_derived_bound(oracle, A, Cn, E, S, B):
    w = smr.random_weights(3, A, Cn, E, S)
    ref = smr.StochasticMlpReference(oracle, w, A, Cn, E, S, 0.97)
    rng = np.random.default_rng([A, Cn, E, B])
    emb = rng.uniform(0, 1, (B, E)).astype(np.float32)
    action, outcome = rng.integers(0, A, B).astype(np.int32), rng.integers(0, Cn, B).astype(np.int32)
    dec, cha = _bounds(w, A, Cn, E, S, emb, action, outcome)
    # the bound's own float64 values are the modules' (the derivation follows the modules, not the reference)
    m = _modules(w, A, Cn, E, S)
    t = lambda x: torch.from_numpy(np.asarray(x)).double() if np.asarray(x).dtype.kind == "f" else torch.from_numpy(np.asarray(x))  # noqa: E731
    d_out, after = m._decision_inference(None, None, t(action), t(emb))
    c_out, state = m._chance_inference(None, None, t(outcome), t(emb))
    mods = dict(afterstate=after, chance_logits=d_out.chance_logits, afterstate_value=d_out.afterstate_value, state=state,
                reward=c_out.reward, action_logits=c_out.action_logits, value=c_out.value)
    for k, v in mods.items():
        x = (dec if k in dec else cha)[k][0]
        assert np.allclose(v.numpy(), x, rtol=0, atol=1e-9), k
    assert float(c_out.discount[0]) == 0.97
    cl, av, ae = ref.decision(action, emb)
    al, v, r, d, se = ref.chance(outcome, emb)
    assert (d == np.float32(0.97)).all()
    got = dict(afterstate=ae, chance_logits=cl, afterstate_value=av, state=se, reward=r, action_logits=al, value=v)
    worst = 0.0
    for k, g in got.items():
        x, dx = (dec if k in dec else cha)[k]
        err = np.abs(g.astype(np.float64) - x)
        worst = max(worst, float((err / dx).max()))
        assert (err <= dx).all(), (k, float(err.max()), float(dx.max()))
    print(f"largest error / bound: {worst:.3f}")
    assert worst > 0 or E == 1  # (the comparison is not vacuous: fp32 and fp64 do differ)
