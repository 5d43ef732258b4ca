"""Independent NumPy float64 restatement of the Stochastic MuZero training step (TEST INFRASTRUCTURE): the unrolled
loss of the default stochastic MLP family and a HAND-DERIVED backward pass -- no autograd, no torch, no muax_amd.

It arbitrates between the two product routes (the fused HIP kernel, and muax_amd/loss.py's stochastic_loss_fn under
torch autograd), as oracle/mz_train_numpy.py does for the plain trio.  Written from the loss's definition:

  s_0 = norm(obs_0 repr_w + repr_b);  (v_0, p_0) = (pv, pp)(s_0);  loss_0 = CE(v_0, twohot(Rn_0)) + CE(p_0, pi_0)
  transition i = 1 .. L-1, with action a_{i-1} and the observation obs_i:
      e     = en(obs_i)                         chance-code logits [C]
      k     = first argmax of e,  o = onehot(k) the code; its VALUE is o, its GRADIENT is e's (straight through)
      as    = norm(ad([g(s_{i-1}), onehot(a_{i-1})]))      g: same value, HALF the gradient (Appendix G)
      (av, ac) = (av, ac)(as)                   afterstate value logits, chance logits
      (r, u)   = (cr, cn)([as, code]);  s_i = norm(u);  (v_i, p_i) = (pv, pp)(s_i)
      loss_i = CE(r, twohot(r_{i-1})) + CE(v_i, twohot(Rn_i)) + CE(p_i, pi_i) + CE(ac, o) + CE(av, twohot(Rn_{i-1}))
               + vqvae_beta * mean_C (e - o)^2                 (o a constant in the last two uses)
  loss = sum_i mean_B (sample_weight * loss_i)  (/ L with divide_by_length)  +  1e-4 * 0.5 * sum ||param||^2, 34 arrays

  every head is Linear(16)-ELU-Linear, [in][out] weights; h(x) = sign(x) (sqrt(|x| + 1) - 1) + 1e-3 x, clipped to
  +-support, two-hot on 2 support + 1 bins;  norm(u) = (u - min u) / c, c = max u - min u, + 1e-5 where below 1e-5;
  tied minima / maxima share the gradient evenly (jax reduce_min / reduce_max).

Backward, per layer (g = gradient of the loss w.r.t. the layer's output):
  CE(l, t) = T lse(l) - sum t l, T = sum t                 dl = softmax(l) T - t
  y = x W + b                                              dW = x^T g, db = sum_B g, dx = g W^T
  a = elu(h)                                               dh = g (h > 0 ? 1 : exp(h))
  s = norm(u)    du_k = g_k / c + [u_k = min] (sum g s - sum g) / (c n_min) + [u_k = max] (-sum g s) / (c n_max)
  beta mean_C (e - o)^2                                    de = 2 beta (e - o) / C
  code (straight through)                                  de += the gradient of [as, code]'s code columns
  g(s)                                                     ds += 0.5 (the gradient of [s, onehot(a)]'s state columns)
"""
from __future__ import annotations

import numpy as np

F64 = np.float64
HEADS = ("ad", "av", "ac", "cr", "cn", "pv", "pp")
WEIGHT_NAMES = (("repr_w", "repr_b") + tuple(f"{h}_{n}" for h in HEADS for n in ("w1", "b1", "w2", "b2"))
                + ("en_w1", "en_b1", "en_w2", "en_b2"))
L2_COEFF = 1e-4


def scaling(x):
    return np.sign(x) * (np.sqrt(np.abs(x) + 1.0) - 1.0) + 1e-3 * x


def two_hot(x, support):
    """[..., 2 support + 1] two-hot target of the scalars x."""
    h = np.clip(scaling(np.asarray(x, F64)), -support, support)
    lo, hi = np.floor(h), np.ceil(h)
    p_hi = h - lo
    out = np.zeros(h.shape + (2 * support + 1,), F64)
    idx = np.indices(h.shape)
    np.add.at(out, tuple(idx) + (lo.astype(np.int64) + support,), 1.0 - p_hi)
    np.add.at(out, tuple(idx) + (hi.astype(np.int64) + support,), p_hi)
    return out


def _elu(h):
    return np.where(h > 0, h, np.expm1(np.minimum(h, 0.0)))


def _minmax(u):
    mn, mx = u.min(1, keepdims=True), u.max(1, keepdims=True)
    c = mx - mn
    c = np.where(c < 1e-5, c + 1e-5, c)
    return (u - mn) / c, (u, mn, mx, c)


def _minmax_bwd(g, s, kept):
    u, mn, mx, c = kept
    is_min, is_max = u == mn, u == mx
    sg, sgs = g.sum(1, keepdims=True), (g * s).sum(1, keepdims=True)
    d_mn, d_mx = (sgs - sg) / c, -sgs / c
    return g / c + is_min * d_mn / is_min.sum(1, keepdims=True) + is_max * d_mx / is_max.sum(1, keepdims=True)


def _mlp(w, p, x):
    h = x @ w[p + "_w1"] + w[p + "_b1"]
    a = _elu(h)
    return a @ w[p + "_w2"] + w[p + "_b2"], (x, h, a)


def _mlp_bwd(w, p, kept, g, grads):
    x, h, a = kept
    grads[p + "_w2"] += a.T @ g
    grads[p + "_b2"] += g.sum(0)
    dh = (g @ w[p + "_w2"].T) * np.where(h > 0, 1.0, np.exp(np.minimum(h, 0.0)))
    grads[p + "_w1"] += x.T @ dh
    grads[p + "_b1"] += dh.sum(0)
    return dh @ w[p + "_w1"].T


def _ce(l, t):
    m = l.max(1, keepdims=True)
    e = np.exp(l - m)
    z = e.sum(1, keepdims=True)
    T = t.sum(1, keepdims=True)
    return T * (m + np.log(z)) - (t * l).sum(1, keepdims=True), e / z * T - t


def loss_and_grads(w, obs, a, r, Rn, pi, support, vqvae_beta=0.25, divide_by_length=False, sample_weight=None,
                   trace=None):
    """(loss, {name: gradient}) in float64.  w: the 34 arrays by name; obs [B, L, obs_dim], an observation for every
    step; a [B, L] actions; r, Rn [B, L] scalars; pi [B, L, A] policy targets; sample_weight [B] or None.  `trace`, a
    dict, receives "norm" (the 2 L - 1 normaliser inputs: the representation's, then the afterstate's and the next
    state's of every transition), "enc" (the L - 1 encoder logit arrays) and "codes" ([B, L - 1])."""
    w = {n: np.asarray(w[n], F64) for n in WEIGHT_NAMES}
    obs, a = np.asarray(obs, F64), np.asarray(a).astype(np.int64)
    B, L = a.shape[:2]
    a = a.reshape(B, L)
    obs = obs.reshape(B, -1, obs.shape[-1])
    A, Cn, E = w["pp_b2"].shape[0], w["en_b2"].shape[0], w["repr_b"].shape[0]
    pi = np.asarray(pi, F64).reshape(B, L, A)
    t_r, t_v = two_hot(np.asarray(r, F64).reshape(B, L), support), two_hot(np.asarray(Rn, F64).reshape(B, L), support)
    sw = np.ones(B, F64) if sample_weight is None else np.asarray(sample_weight, F64).reshape(B)
    row = (sw / (B * L if divide_by_length else B))[:, None]  # what one row's term counts in the loss
    eye_a, eye_c = np.eye(A, dtype=F64), np.eye(Cn, dtype=F64)

    s, k0 = _minmax(obs[:, 0] @ w["repr_w"] + w["repr_b"])
    lv, kv = _mlp(w, "pv", s)
    lp, kp = _mlp(w, "pp", s)
    cv, dlv = _ce(lv, t_v[:, 0])
    cp, dlp = _ce(lp, pi[:, 0])
    data = float(((cv + cp) * row).sum())
    first = (s, k0, kv, kp, dlv * row, dlp * row)
    norm_in, enc_out, codes, steps = [k0[0]], [], [], []
    for i in range(1, L):
        e, ke = _mlp(w, "en", obs[:, i])
        code = e.argmax(1)  # the first of tied maxima
        o = eye_c[code]
        ua, kad = _mlp(w, "ad", np.concatenate([s, eye_a[a[:, i - 1]]], 1))
        after, kna = _minmax(ua)
        lav, kav = _mlp(w, "av", after)
        lac, kac = _mlp(w, "ac", after)
        xc = np.concatenate([after, o], 1)
        lr, kcr = _mlp(w, "cr", xc)
        un, kcn = _mlp(w, "cn", xc)
        s, kns = _minmax(un)
        lv, kv = _mlp(w, "pv", s)
        lp, kp = _mlp(w, "pp", s)
        c_r, dlr = _ce(lr, t_r[:, i - 1])
        c_v, dlv = _ce(lv, t_v[:, i])
        c_p, dlp = _ce(lp, pi[:, i])
        c_c, dlc = _ce(lac, o)
        c_a, dla = _ce(lav, t_v[:, i - 1])
        commit = ((e - o) ** 2).mean(1, keepdims=True)
        data += float(((c_r + c_v + c_p + c_c + c_a + vqvae_beta * commit) * row).sum())
        de = 2.0 * vqvae_beta * (e - o) / Cn * row
        norm_in += [ua, un]
        enc_out.append(e)
        codes.append(code)
        steps.append((ke, de, kad, after, kna, kav, kac, kcr, kcn, s, kns, kv, kp,
                      dlr * row, dlv * row, dlp * row, dlc * row, dla * row))
    loss = data + L2_COEFF * 0.5 * sum(float((w[n] ** 2).sum()) for n in WEIGHT_NAMES)
    if trace is not None:
        trace["norm"], trace["enc"] = norm_in, enc_out
        trace["codes"] = np.stack(codes, 1) if codes else np.zeros((B, 0), np.int64)

    grads = {n: np.zeros_like(w[n]) for n in WEIGHT_NAMES}
    carry = np.zeros((B, E), F64)  # what reaches s_i from transition i + 1, already halved
    for ke, de, kad, after, kna, kav, kac, kcr, kcn, s, kns, kv, kp, dlr, dlv, dlp, dlc, dla in reversed(steps):
        ds = carry + _mlp_bwd(w, "pv", kv, dlv, grads) + _mlp_bwd(w, "pp", kp, dlp, grads)
        dxc = _mlp_bwd(w, "cn", kcn, _minmax_bwd(ds, s, kns), grads) + _mlp_bwd(w, "cr", kcr, dlr, grads)
        _mlp_bwd(w, "en", ke, de + dxc[:, E:], grads)  # straight through: the code's gradient is the encoder output's
        dafter = dxc[:, :E] + _mlp_bwd(w, "av", kav, dla, grads) + _mlp_bwd(w, "ac", kac, dlc, grads)
        dxa = _mlp_bwd(w, "ad", kad, _minmax_bwd(dafter, after, kna), grads)
        carry = 0.5 * dxa[:, :E]
    s, k0, kv, kp, dlv, dlp = first
    ds = carry + _mlp_bwd(w, "pv", kv, dlv, grads) + _mlp_bwd(w, "pp", kp, dlp, grads)
    du0 = _minmax_bwd(ds, s, k0)
    grads["repr_w"] += obs[:, 0].T @ du0
    grads["repr_b"] += du0.sum(0)
    for n in WEIGHT_NAMES:
        grads[n] += L2_COEFF * w[n]
    return loss, grads
