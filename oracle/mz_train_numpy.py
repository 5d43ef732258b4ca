"""Independent NumPy float64 restatement of the training step (TEST INFRASTRUCTURE): the k-step unrolled MuZero loss
of the default MLP trio and a HAND-DERIVED backward pass -- no autograd, no torch, no muax_amd.

It arbitrates between the two product routes (the fused HIP kernel, and muax_amd/loss.py under torch autograd): a
reference that shares code with one of them cannot.  Written from the formulas of

  muax/loss.py:10-88    loss = sum_i [ mean_B CE(r_i, twohot(r)) + mean_B CE(v_i, twohot(Rn)) + mean_B CE(pi_i, pi) ]
                        (/ L in the coax variant)  +  1e-4 * 0.5 * sum ||param||^2 over all 18 arrays;
                        the state's gradient is halved where it enters the dynamics (Appendix G);
  muax/utils.py:65-91   h(x) = sign(x) (sqrt(|x| + 1) - 1) + 1e-3 x, clipped to +-support, two-hot on 2 support + 1 bins;
  muax/nn.py:37-44      s = (u - min u) / c,  c = max u - min u, + 1e-5 where that is below 1e-5;
  muax/nn.py:59-115     Linear / Linear-ELU-Linear heads, dynamics on [s, onehot(a)];
  jax reduce_min / reduce_max: tied extrema share the gradient evenly.

Backward, per layer (g = gradient of the loss w.r.t. the layer's output):
  CE(l, t) = T lse(l) - sum t l, T = sum t                 dl = softmax(l) T - t
  y = x W + b                                              dW = x^T g, db = sum_B g, dx = g W^T
  a = elu(h)                                               dh = g (h > 0 ? 1 : exp(h))
  s_k = (u_k - mn) / c, mn = min u, mx = max u, c = mx - mn (+ 1e-5: the same derivatives)
      direct:      ds_k / du_k = 1 / c
      through mn:  ds_k / dmn  = -1 / c + (u_k - mn) / c^2 = (s_k - 1) / c
      through mx:  ds_k / dmx  = -(u_k - mn) / c^2         = -s_k / c
      du_k = g_k / c + [u_k = mn] (sum g s - sum g) / (c n_min) + [u_k = mx] (-sum g s) / (c n_max)
"""
from __future__ import annotations

import numpy as np

F64 = np.float64
WEIGHT_NAMES = ("repr_w", "repr_b", "pv_w1", "pv_b1", "pv_w2", "pv_b2", "pp_w1", "pp_b1", "pp_w2", "pp_b2",
                "dr_w1", "dr_b1", "dr_w2", "dr_b2", "dn_w1", "dn_b1", "dn_w2", "dn_b2")
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
    return (u - mn) / c, mn, mx, c


def _minmax_bwd(g, u, s, mn, mx, c):
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
    return (T * (m + np.log(z)) - (t * l).sum(1, keepdims=True))[:, 0], e / z * T - t


def forward(w, obs0, a, r, Rn, pi, support, divide_by_length=False, trace=None, frozen_states=None):
    """The loss alone.  `trace`, a dict, receives "normalizer_inputs" (the representation's, then each dynamics
    step's, the unused last one included), "scaled_targets" (h(x) before the clip, rewards then returns),
    "elu_inputs" (every hidden pre-activation of the heads that reach the loss) and "states" (s_0 .. s_{L-1}).

    The halved state gradient is scale_gradient(s, 0.5) = 0.5 s + 0.5 stop_gradient(s) in front of the dynamics: the
    same value, half the derivative.  A finite difference of the plain forward would see the whole derivative, so
    `frozen_states` (the "states" of the point the difference is taken at) stands in for the stop_gradient half: with
    it, the central difference of this function in a weight is the derivative the backward pass below computes."""
    loss, _ = _run(w, obs0, a, r, Rn, pi, support, divide_by_length, False, trace, frozen_states)
    return loss


def loss_and_grads(w, obs0, a, r, Rn, pi, support, divide_by_length=False):
    """(loss, {name: gradient}) in float64.  w: the 18 arrays by name ([in][out] weights); obs0 [B, obs_dim] the first
    observations; a [B, L] actions; r, Rn [B, L] scalars; pi [B, L, A] policy targets."""
    return _run(w, obs0, a, r, Rn, pi, support, divide_by_length, True, None, None)


def _run(w, obs0, a, r, Rn, pi, support, divide_by_length, want_grads, trace, frozen):
    w = {n: np.asarray(w[n], F64) for n in WEIGHT_NAMES}
    obs0, a = np.asarray(obs0, F64), np.asarray(a).astype(np.int64)
    B, L = a.shape
    A = w["pp_b2"].shape[0]
    E = w["repr_b"].shape[0]
    pi = np.asarray(pi, F64).reshape(B, L, A)
    t_r, t_v = two_hot(np.asarray(r, F64).reshape(B, L), support), two_hot(np.asarray(Rn, F64).reshape(B, L), support)
    scale = 1.0 / (B * L) if divide_by_length else 1.0 / B
    eye = np.eye(A, dtype=F64)

    u0 = obs0 @ w["repr_w"] + w["repr_b"]
    s, *mm0 = _minmax(u0)
    norm_in, elu_in, steps, data_loss = [u0], [], [], 0.0
    for i in range(L):
        s_dyn = s if frozen is None else 0.5 * s + 0.5 * frozen[i]
        x = np.concatenate([s_dyn, eye[a[:, i]]], 1)
        lv, kv = _mlp(w, "pv", s)
        lp, kp = _mlp(w, "pp", s)
        lr, kr = _mlp(w, "dr", x)
        un, kn = _mlp(w, "dn", x)
        ns, *mmn = _minmax(un)
        cv, dlv = _ce(lv, t_v[:, i])
        cp, dlp = _ce(lp, pi[:, i])
        cr, dlr = _ce(lr, t_r[:, i])
        data_loss += (cv.sum() + cp.sum() + cr.sum()) * scale
        norm_in.append(un)
        elu_in += [kv[1], kp[1], kr[1]] + ([kn[1]] if i + 1 < L else [])
        steps.append((s, kv, kp, kr, kn, un, ns, mmn, dlv * scale, dlp * scale, dlr * scale))
        s = ns
    loss = data_loss + L2_COEFF * 0.5 * sum(float((w[n] ** 2).sum()) for n in WEIGHT_NAMES)
    if trace is not None:
        trace["normalizer_inputs"] = norm_in
        trace["scaled_targets"] = np.stack([scaling(np.asarray(r, F64).reshape(B, L)),
                                            scaling(np.asarray(Rn, F64).reshape(B, L))])
        trace["elu_inputs"] = elu_in
        trace["states"] = [st[0] for st in steps]
    if not want_grads:
        return loss, None

    grads = {n: np.zeros_like(w[n]) for n in WEIGHT_NAMES}
    ds_next = np.zeros((B, E), F64)  # gradient w.r.t. s_{i+1}
    for i in range(L - 1, -1, -1):
        s, kv, kp, kr, kn, un, ns, mmn, dlv, dlp, dlr = steps[i]
        dx = _mlp_bwd(w, "dr", kr, dlr, grads)
        if i + 1 < L:
            dx = dx + _mlp_bwd(w, "dn", kn, _minmax_bwd(ds_next, un, ns, *mmn), grads)
        ds = 0.5 * dx[:, :E]  # the state's gradient is halved where it enters the dynamics
        ds = ds + _mlp_bwd(w, "pv", kv, dlv, grads) + _mlp_bwd(w, "pp", kp, dlp, grads)
        ds_next = ds
    du0 = _minmax_bwd(ds_next, u0, steps[0][0], *mm0)
    grads["repr_w"] += obs0.T @ du0
    grads["repr_b"] += du0.sum(0)
    for n in WEIGHT_NAMES:
        grads[n] += L2_COEFF * w[n]
    return loss, grads
