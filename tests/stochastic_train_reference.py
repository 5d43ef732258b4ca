"""The fused stochastic training step's reference (test_stochastic_train_cpu.py, test_gpu_stochastic_train.py): torch
autograd through loss.stochastic_loss_fn on a copy of the model's six modules, float64 on the CPU by default.  The loss's
own `t()` casts every batch field to the modules' dtype, so the float64 copy evaluates the whole formula in float64.

`conditions()` measures, in float64, how far the inputs are from the places where float32 and float64 may legitimately
take different branches: the encoder's top-two logit gap (the argmax), the gap between the two smallest and between the
two largest inputs of every min_max_normalize (the tie rule), the distance of every scaled support target from an
integer (floor / ceil)."""
import copy

import numpy as np
import torch

from helpers import train_batch

F32 = np.float32

# (A, C, E, support, obs_dim) of the GPU tests: every vector in one slot and C < A; X = E + C = 48, chance logits in two
# slots, E + A across a slot boundary; C and obs_dim just past a slot boundary
SHAPES = [(3, 2, 4, 8, 5), (4, 32, 16, 10, 16), (4, 17, 8, 8, 20)]


def smz_model(A, Cn, E, support, obs_dim, seed, device=None, bias_noise=True, optimizer=("adam", 1e-2), **model_kw):
    """A default stochastic MLP family with haiku's init; `bias_noise` adds N(0, 0.1) to every bias so that every bias
    path carries a gradient.  The weights do not depend on the device (CPU generator)."""
    import muax_amd as mx
    g = torch.Generator().manual_seed(seed)
    net = mx.create_stochastic_muzero_network(E, A, Cn, 2 * support + 1, generator=g)
    m = mx.MuZero(net, optimizer=mx.optimizers.create_optimizer(*optimizer), support_size=support, device=device, **model_kw)
    m.init(0, np.zeros((1, obs_dim)))
    if bias_noise:
        with torch.no_grad():
            for p in [p for mod in m.network for p in mod.parameters()]:
                if p.dim() == 1:
                    p.add_(0.1 * torch.randn(p.shape, generator=g).to(p.device))
        m.weights_changed()
    return m


def smz_batch(B, L, A, obs_dim, seed):
    """obs [B, L, obs_dim] in (-1, 1), r in (-2, 3), Rn in (-30, 60) (inside the clip of support 8), Dirichlet pi."""
    return train_batch(B, L, A, obs_dim, seed)


def cut_rows(b, rows):
    import muax_amd as mx
    return mx.Transition(**{k: (np.asarray(v)[rows] if np.ndim(v) else v) for k, v in b.__dict__.items()})


def copy_model(m, dtype=torch.float64, device="cpu"):
    import muax_amd as mx
    mods = [copy.deepcopy(x).to(device=device, dtype=dtype) for x in m.network]
    m2 = mx.MuZero(mx.nn.SMZNetwork(*mods), device=device, support_size=m._support_size)
    m2._params = True
    return m2


def autograd(m, b, dtype=torch.float64, device="cpu", **kw):
    """(loss, [gradient of every STOCHASTIC_TRAIN_WEIGHT_NAMES array] as float64 NumPy) of loss.stochastic_loss_fn."""
    import muax_amd as mx
    from muax_amd._lib import STOCHASTIC_TRAIN_WEIGHT_NAMES
    m2 = copy_model(m, dtype, device)
    loss = mx.loss.stochastic_loss_fn(m2, b, **kw)
    assert loss.dtype == dtype
    loss.backward()
    w = mx.nn.stochastic_train_weights(m2.network)
    return float(loss.detach()), [w[n].grad.detach().cpu().double().numpy() for n in STOCHASTIC_TRAIN_WEIGHT_NAMES]


def conditions(m, b):
    """float64, per (row, step) or finer: dict(encoder_gap [B, L-1], minmax_gap [B, 2 L - 1] (the representation's, then
    the afterstate's and the next state's of every transition; the smaller of bottom-two and top-two gap),
    target_distance [B, 2 L] (r, then Rn))."""
    import muax_amd as mx
    m2 = copy_model(m)
    B, L = np.asarray(b.a).shape[:2]
    obs = torch.as_tensor(np.asarray(b.obs), dtype=torch.float64)
    with torch.no_grad():
        gaps = []
        for i in range(1, L):
            top = m2.enc_func(obs[:, i]).topk(2, dim=-1).values
            gaps.append((top[:, 0] - top[:, 1]).numpy())
        cap = []
        norm = mx.nn.min_max_normalize

        def recording(s):
            cap.append(s.detach().clone())
            return norm(s)
        mx.nn.min_max_normalize = recording
        try:
            mx.loss.stochastic_loss_fn(m2, b)
        finally:
            mx.nn.min_max_normalize = norm
    assert len(cap) == 2 * L - 1
    mm = []
    for u in cap:
        u = u.sort(dim=1).values
        mm.append(torch.minimum(u[:, 1] - u[:, 0], u[:, -1] - u[:, -2]).numpy())
    S = m._support_size
    x = np.concatenate([np.asarray(b.r, np.float64).reshape(B, L), np.asarray(b.Rn, np.float64).reshape(B, L)], 1)
    xs = np.clip(np.sign(x) * (np.sqrt(np.abs(x) + 1) - 1) + 1e-3 * x, -S, S)
    return dict(encoder_gap=np.stack(gaps, 1) if gaps else np.zeros((B, 0)), minmax_gap=np.stack(mm, 1),
                target_distance=np.abs(xs - np.round(xs)))


def well_conditioned(cond):
    enc, mm, td = cond["encoder_gap"], cond["minmax_gap"], cond["target_distance"]
    return (enc.size == 0 or enc.min() >= 1e-3) and mm.min() >= 1e-4 and td.min() >= 1e-4


def rel_errors(got, ref):
    """max |got - ref| per array over max(largest |ref| entry, 1e-6): the measure of tests/test_gpu_train.py"""
    return [float(np.abs(np.asarray(g, np.float64) - d).max() / max(np.abs(d).max(), 1e-6)) for g, d in zip(got, ref)]


# ---- the independent NumPy reference and the edge inputs, shared by the CPU arbitration test
# (test_stochastic_train_reference_cpu.py) and the GPU tests (test_gpu_stochastic_train_edges.py) ----
def arrays(m):
    """The 34 arrays of the model as float32 NumPy copies, by name."""
    import muax_amd as mx
    return {n: t.detach().cpu().numpy().copy() for n, t in mx.nn.stochastic_train_weights(m.network).items()}


def set_arrays(m, **new):
    import muax_amd as mx
    w = mx.nn.stochastic_train_weights(m.network)
    with torch.no_grad():
        for n, v in new.items():
            w[n].copy_(torch.as_tensor(np.asarray(v), dtype=torch.float32))
    m.weights_changed()


def numpy_reference(m, b, trace=None, **kw):
    """(loss, [gradient of every STOCHASTIC_TRAIN_WEIGHT_NAMES array]) of oracle/mz_stoch_train_numpy.py -- float64,
    hand-derived backward, no torch and no muax_amd inside -- on the model's float32 weights and the batch."""
    from muax_amd._lib import STOCHASTIC_TRAIN_WEIGHT_NAMES
    from oracle import mz_stoch_train_numpy as oracle
    loss, g = oracle.loss_and_grads(arrays(m), b.obs, b.a, b.r, b.Rn, b.pi, m._support_size, trace=trace, **kw)
    return loss, [g[n] for n in STOCHASTIC_TRAIN_WEIGHT_NAMES]


def captures(m, b, dtype=torch.float64, device="cpu"):
    """What stochastic_loss_fn's forward pass sees in `dtype`: dict(norm = the 2 L - 1 normaliser inputs [B, E] (the
    representation's, then the afterstate's and the next state's of every transition), enc = the L - 1 encoder logit
    arrays [B, C]), as NumPy arrays of that precision."""
    import muax_amd as mx
    m2 = copy_model(m, dtype, device)
    L = np.asarray(b.a).shape[1]
    obs = torch.as_tensor(np.asarray(b.obs), dtype=dtype, device=device)
    cap = []
    norm = mx.nn.min_max_normalize

    def recording(s):
        cap.append(s.detach().cpu().numpy().copy())
        return norm(s)
    with torch.no_grad():
        enc = [m2.enc_func(obs[:, i]).cpu().numpy() for i in range(1, L)]
        mx.nn.min_max_normalize = recording
        try:
            mx.loss.stochastic_loss_fn(m2, b)
        finally:
            mx.nn.min_max_normalize = norm
    assert len(cap) == 2 * L - 1
    return dict(norm=cap, enc=enc)


def edge_conditions(cap, b, support, tied=None):
    """conditions() on captured inputs, with the INTENDED ties taken out first: `tied` maps a normaliser's index in
    cap["norm"] to the column sets expected to tie there (all but the first column of each set are removed before the
    two-smallest / two-largest gaps are measured), or to "skip" (a normaliser whose spacing is the case's own subject).
    A normaliser left with one column has no gap to measure (inf).  Also runner_up_gap [B, L - 1]: the encoder's
    largest logit minus its third-largest."""
    tied = tied or {}
    B, L = np.asarray(b.a).shape[:2]
    mm = []
    for k, u in enumerate(cap["norm"]):
        u = np.asarray(u, np.float64)
        sets = tied.get(k, ())
        if isinstance(sets, str):
            mm.append(np.full(B, np.inf))
            continue
        drop = sorted({c for cols in sets for c in list(cols)[1:]})
        u = np.sort(np.delete(u, drop, axis=1), axis=1)
        mm.append(np.minimum(u[:, 1] - u[:, 0], u[:, -1] - u[:, -2]) if u.shape[1] > 1 else np.full(B, np.inf))
    top = [np.sort(np.asarray(e, np.float64), axis=1)[:, ::-1] for e in cap["enc"]]
    x = np.concatenate([np.asarray(b.r, np.float64).reshape(B, L), np.asarray(b.Rn, np.float64).reshape(B, L)], 1)
    xs = np.clip(np.sign(x) * (np.sqrt(np.abs(x) + 1) - 1) + 1e-3 * x, -support, support)
    stack = lambda f: np.stack([f(t) for t in top], 1) if top else np.zeros((B, 0))  # noqa: E731
    return dict(encoder_gap=stack(lambda t: t[:, 0] - t[:, 1]), runner_up_gap=stack(lambda t: t[:, 0] - t[:, 2]),
                minmax_gap=np.stack(mm, 1), target_distance=np.abs(xs - np.round(xs)))


class StochEdge:
    """One edge input: the model `m`, the batch `b`, the keyword arguments `kw` of the loss, `verify(cap)` asserting on
    captures() of either precision that the edge occurs and that every OTHER condition of well_conditioned holds for
    the whole batch; and what the data contribute exact zeros to: `absent_actions`, `absent_codes` (lists),
    `pi_zero`; `keep` (zero_weight_rows): the rows whose sample weight is not zero."""

    def __init__(self, m, b, verify, kw=None, absent_actions=None, absent_codes=None, pi_zero=False, keep=None):
        self.m, self.b, self.verify, self.kw = m, b, verify, dict(kw or {})
        self.absent_actions, self.absent_codes, self.pi_zero, self.keep = absent_actions, absent_codes, pi_zero, keep


def _verifier(b, support, tied=None, encoder=True, targets=True, extra=None):
    """verify(cap): `extra(cap)` (the edge itself), then the conditions that stay: the encoder's top-two gap at least
    1e-3 (`encoder`), every non-tied normaliser gap at least 1e-4, every target 1e-4 from an integer (`targets`)."""
    def verify(cap):
        if extra is not None:
            extra(cap)
        c = edge_conditions(cap, b, support, tied)
        assert c["minmax_gap"].min() >= 1e-4, ("pick another seed: normaliser gap", float(c["minmax_gap"].min()))
        if encoder and c["encoder_gap"].size:
            assert c["encoder_gap"].min() >= 1e-3, ("pick another seed: encoder gap", float(c["encoder_gap"].min()))
        if targets:
            assert c["target_distance"].min() >= 1e-4, ("pick another seed: target", float(c["target_distance"].min()))
    return verify


def dyadic(rng, shape, step, lim):
    return (rng.integers(-int(lim / step), int(lim / step) + 1, shape) * step).astype(F32)


WIDE, PAD, MID, TINY = (4, 32, 32, 31, 16), (4, 17, 8, 8, 20), (4, 32, 16, 10, 16), (3, 2, 4, 8, 5)  # listed instances
# (min partners, max partners) by E: at E = 32 and 17 the partners lie in different 16-lane slots, the three-way max
# with two in one slot and one in the other (E = 17: column 16 is the one real lane of slot 1)
TIE_COLS = {32: ((3, 19), (5, 9, 21)), 8: ((3, 6), (1, 4, 7)), 17: ((3, 9), (5, 14, 16))}
# seed per case, picked on the CPU as the first from 0 at which verify() passes on the float64 AND the float32 captures
# of the whole batch (nothing is filtered out afterwards)
EDGE_SEEDS = {
    "ties_repr-E32": 0, "ties_repr-E8": 0, "ties_after-E32": 3, "ties_after-E8": 2, "ties_next-E32": 3, "ties_next-E8": 2,
    "all_tied-E32": 2, "all_tied-E8": 0, "near_degenerate-2^-18": 0, "near_degenerate-2^-16": 0,
    "encoder_tie_first-C32": 1, "encoder_tie_first-C17": 0, "large_logits-F63-50": 0, "large_logits-F63-300": 0,
    "large_logits-C17-50": 1, "large_logits-C17-300": 1, "policy_targets": 0, "policy_targets-all_zero": 0,
    "support_edges-8": 0, "support_edges-31": 0, "absent_actions-first": 2, "absent_actions-last": 0,
    "zero_weight_rows": 0, "batch_edges-15": 0, "batch_edges-16": 0, "batch_edges-17": 0, "batch_edges-63": 2,
    "batch_edges-65": 2, "large_reduction": 0, "ties_repr-E17": 2, "encoder_tie_first-E17": 0,
}


def _tie_check(E, idx):
    mins, maxs = TIE_COLS[E]

    def extra(cap):
        assert len(cap["norm"]) > max(idx)
        for k in idx:
            u = np.asarray(cap["norm"][k])
            assert u.shape[1] == E
            for cols, ext in ((mins, u.min(1)), (maxs, u.max(1))):
                assert (u[:, list(cols)] == ext[:, None]).all()
                assert ((u == ext[:, None]).sum(1) == len(cols)).all()
    return extra


def _edge_ties_repr(shape, seed, d, B=40, L=3):
    """repr_w columns duplicated with their biases, -12 / +12 beside dyadic weights of at most 0.5: the min ties two
    ways and the max three ways.  Weights and ALL observations are dyadic (1/16 and 1/8), so obs W + b is exact in
    fp32 and fp64 and in any summation order."""
    A, _, E, S, od = shape
    m, b = smz_model(*shape, seed=seed, device=d), smz_batch(B, L, A, od, seed)
    rng = np.random.default_rng(5)
    W, bias = dyadic(rng, (od, E), 1 / 16, 0.5), dyadic(rng, E, 1 / 16, 0.5)
    mins, maxs = TIE_COLS[E]
    for cols, v in ((mins, -12.0), (maxs, 12.0)):
        W[:, list(cols[1:])] = W[:, [cols[0]]]
        bias[list(cols)] = v
    b.obs[:] = dyadic(rng, b.obs.shape, 1 / 8, 1.0)
    set_arrays(m, repr_w=W, repr_b=bias)
    return StochEdge(m, b, _verifier(b, S, {0: (mins, maxs)}, extra=_tie_check(E, [0])))


def _edge_ties_second_layer(shape, head, seed, d, B=36, L=5):
    """`head`_w2 columns ("ad": the afterstate's, "cn": the next state's normaliser) duplicated with their biases at
    -20 / +20: min and max tie in every transition.  Each tied column keeps ONE non-zero weight (row 2 for the min's
    partners, row 11 for the max's), as helpers._edge_ties_dn: elu(h) W2 + b2 is then one product plus the bias there
    whatever order a matrix product sums in, so the tie holds in every implementation and precision."""
    A, _, E, S, od = shape
    m, b = smz_model(*shape, seed=seed, device=d), smz_batch(B, L, A, od, seed)
    w = arrays(m)
    W2, b2 = w[head + "_w2"], w[head + "_b2"]
    mins, maxs = TIE_COLS[E]
    for cols, k, v in ((mins, 2, -20.0), (maxs, 11, 20.0)):
        keep = W2[k, cols[0]]
        W2[:, list(cols)] = 0.0
        W2[k, list(cols)] = keep
        b2[list(cols)] = v
    set_arrays(m, **{head + "_w2": W2, head + "_b2": b2})
    idx = list(range(1 if head == "ad" else 2, 2 * L - 1, 2))
    assert len(idx) == L - 1
    return StochEdge(m, b, _verifier(b, S, {k: (mins, maxs) for k in idx}, extra=_tie_check(E, idx)))


def _edge_all_tied(shape, seed, d, B=32, L=4):
    """A fresh net (zero biases) on all-zero first observations: all E entries of obs_0 W + b are 0, each both min and
    max, and c = 0 takes the +1e-5 branch."""
    A, _, E, S, od = shape
    m, b = smz_model(*shape, seed=seed, device=d, bias_noise=False), smz_batch(B, L, A, od, seed)
    b.obs[:, 0] = 0.0

    def extra(cap):
        u = np.asarray(cap["norm"][0])
        assert u.shape == (B, E) and float(np.abs(u).max()) == 0.0
    return StochEdge(m, b, _verifier(b, S, {0: (tuple(range(E)),)}, extra=extra))


def _edge_near_degenerate(log2_range, seed, d, B=32, L=3):
    """WIDE (E = 32): repr_w's columns equal and dyadic, the biases 0.25 + range * (eighths) with the single minimum
    in slot 1 (column 20), the single maximum in slot 0 (column 7) and the grades in between over both slots: every
    row's range is exactly 2^log2_range in fp32 and fp64 (2^-18 is below 1e-5: the +1e-5 branch)."""
    A, _, E, S, od = WIDE
    m, b = smz_model(*WIDE, seed=seed, device=d), smz_batch(B, L, A, od, seed)
    rng = np.random.default_rng(7)
    W = np.repeat(dyadic(rng, od, 1 / 64, 0.5)[:, None], E, 1)
    c = 2.0 ** log2_range
    frac = np.array([(1 + k % 7) / 8 for k in range(E)])
    frac[20], frac[7] = 0.0, 1.0
    b.obs[:] = dyadic(rng, b.obs.shape, 1 / 8, 1.0)
    set_arrays(m, repr_w=W, repr_b=(0.25 + c * frac).astype(F32))

    def extra(cap):
        u = np.asarray(cap["norm"][0])
        assert ((u.max(1) - u.min(1)) == c).all() and (c < 1e-5) == (log2_range == -18)
        assert (u.argmin(1) == 20).all() and (u.argmax(1) == 7).all()
        assert ((u == u.min(1, keepdims=True)).sum(1) == 1).all() and ((u == u.max(1, keepdims=True)).sum(1) == 1).all()
    return StochEdge(m, b, _verifier(b, S, {0: "skip"}, extra=extra))


def _edge_encoder_tie(shape, cols, seed, d, B=40, L=3):
    """en_w2 columns `cols` duplicated (one non-zero weight each, row 5, as in _edge_ties_second_layer) with en_b2
    raised to 6: exactly those two logits tie for the maximum at every row and step; the code must be the lower index,
    so every other code -- the higher partner among them -- is absent from the batch."""
    A, Cn, E, S, od = shape
    m, b = smz_model(*shape, seed=seed, device=d), smz_batch(B, L, A, od, seed)
    w = arrays(m)
    W2, b2 = w["en_w2"], w["en_b2"]
    keep = W2[5, cols[0]]
    W2[:, list(cols)] = 0.0
    W2[5, list(cols)] = keep
    b2[list(cols)] = 6.0
    set_arrays(m, en_w2=W2, en_b2=b2)

    def extra(cap):
        assert len(cap["enc"]) == L - 1
        for e in cap["enc"]:
            e = np.asarray(e)
            assert (e[:, cols[0]] == e[:, cols[1]]).all() and (e[:, cols[0]] == e.max(1)).all()
            assert ((e == e.max(1, keepdims=True)).sum(1) == 2).all() and (e.argmax(1) == min(cols)).all()
        c = edge_conditions(cap, b, S)
        assert (c["encoder_gap"] == 0).all() and c["runner_up_gap"].min() >= 1e-3
    return StochEdge(m, b, _verifier(b, S, encoder=False, extra=extra),
                     absent_codes=[c for c in range(Cn) if c != min(cols)])


def _edge_large_logits(shape, reach, seed, d, B=48, L=3):
    """The output layers of av, ac, cr, pv and pp scaled until their logits reach about +-reach (measured on the first
    transition in float64 on the CPU, so that the weights do not depend on the device); the encoder and the
    state-producing stacks (repr, ad, cn) are left alone, so the argmax and the normalisers are conditioned as before."""
    A, _, _, S, od = shape
    m, b = smz_model(*shape, seed=seed, device=d), smz_batch(B, L, A, od, seed)

    def outputs():
        m2 = copy_model(m)
        rep, pred, after_dy, after_pred, chance_dy, enc = m2.network
        with torch.no_grad():
            obs = torch.as_tensor(np.asarray(b.obs), dtype=torch.float64)
            s = rep(obs[:, 0])
            after = after_dy(s, torch.as_tensor(np.asarray(b.a)[:, 0]))
            av, ac = after_pred(after)
            r, _ = chance_dy(after, enc.code(obs[:, 1])[1])
            pv, pp = pred(s)
        return dict(av=av, ac=ac, cr=r, pv=pv, pp=pp)
    w = arrays(m)
    new = {}
    for h, out in outputs().items():
        f = F32(reach / float(out.abs().max()))
        new[h + "_w2"], new[h + "_b2"] = w[h + "_w2"] * f, w[h + "_b2"] * f
    set_arrays(m, **new)
    for h, out in outputs().items():
        assert 0.7 * reach <= float(out.abs().max()) <= 1.3 * reach, (h, float(out.abs().max()))
    return StochEdge(m, b, _verifier(b, S))


def _edge_policy_targets(seed, d, zero=False, B=40, L=3):
    """MID: one-hot rows, rows with two zeros, all-zero rows (padded steps: no loss, no gradient), rows summing to 0.5
    and to 3, in turn over rows and steps; `zero`: every row zero, and the policy head sees no data at all."""
    A, _, _, S, od = MID
    m, b = smz_model(*MID, seed=seed, device=d), smz_batch(B, L, A, od, seed)
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
    b.pi[:] = 0.0 if zero else pi.reshape(B, L, 1, A)

    def extra(cap):
        p = np.asarray(b.pi).reshape(B, L, A)
        if zero:
            assert not p.any()
            return
        sums = p.sum(-1)
        assert ((p == 1).sum(-1) == 1).any() and (sums == 0).any() and ((p == 0).sum(-1) == 2).any()
        assert np.isclose(sums, 0.5).any() and np.isclose(sums, 3.0).any()
    return StochEdge(m, b, _verifier(b, S, extra=extra), pi_zero=zero)


def _edge_support(shape, seed, d, B=32, L=3):
    """helpers.support_edge_scalars(support) -- 0, +-1, h(x) on an integer and one float32 ulp either side, the clip,
    far beyond it -- over the B L entries of r, and rolled and negated over those of Rn: r feeds the reward head, Rn
    both v_i and the afterstate value of transition i + 1.  At support 31 the clip puts the mass on bin 0 and on bin
    62, the last real lane of slot 3.  The target condition is the one given up here."""
    from helpers import support_edge_scalars
    A, _, _, S, od = shape
    x = support_edge_scalars(S)
    assert len(x) <= B * L
    m, b = smz_model(*shape, seed=seed, device=d), smz_batch(B, L, A, od, seed)
    b.r[:] = np.resize(x, B * L).reshape(B, L)
    b.Rn[:] = -np.resize(np.roll(x, 7), B * L)[::-1].reshape(B, L)

    def extra(cap):
        for f in (b.r, b.Rn):
            assert set(np.abs(x).tolist()) <= set(np.abs(np.asarray(f)).ravel().tolist())
        c = edge_conditions(cap, b, S)["target_distance"]
        assert (c[:, :L] == 0).any() and (c[:, L:] == 0).any()
    return StochEdge(m, b, _verifier(b, S, targets=False, extra=extra))


def _edge_absent_actions(shape, action, seed, d, B=40, L=3):
    """Every action the same: the ad_w1 rows of the actions not taken get exact zeros from the data."""
    A, _, _, S, od = shape
    m, b = smz_model(*shape, seed=seed, device=d), smz_batch(B, L, A, od, seed)
    b.a[:] = action

    def extra(cap):
        assert (np.asarray(b.a) == action).all()
    return StochEdge(m, b, _verifier(b, S, extra=extra), absent_actions=[k for k in range(A) if k != action])


def _edge_zero_weight_rows(seed, d, B=48, L=3):
    """MID with sample weights 1 but for exact zeros on rows 3, 40, 47 and the whole second workgroup (rows 16..31):
    the result is that of the batch without those rows at the same scale per row."""
    A, _, _, S, od = MID
    m, b = smz_model(*MID, seed=seed, device=d), smz_batch(B, L, A, od, seed)
    sw = np.ones(B, F32)
    sw[[3, 40, 47]] = 0.0
    sw[16:32] = 0.0
    return StochEdge(m, b, _verifier(b, S), kw=dict(sample_weight=sw), keep=[int(k) for k in np.flatnonzero(sw)])


def _edge_batch(B, seed, d, L=3):
    """PAD at a batch of B rows: one short of, exactly, and one past a 16-row workgroup, and the same around four."""
    A, _, _, S, od = PAD
    m, b = smz_model(*PAD, seed=seed, device=d), smz_batch(B, L, A, od, seed)
    return StochEdge(m, b, _verifier(b, S))


def _edge_large_reduction(seed, d, B=4096, L=2):
    """WIDE at B = 4096, L = 2: 256 workgroup partials per gradient entry.  No seeded batch of 4096 rows has every
    row clear of every condition (about one row in ten misses one), so the batch IS the first 4096 qualifying rows of
    a seeded 5120 -- the conditions are per row -- and verify() then asserts them on that whole batch."""
    A, _, _, S, od = WIDE
    m, pool = smz_model(*WIDE, seed=seed, device=d), smz_batch(5120, L, A, od, seed)
    c = conditions(m, pool)
    ok = (c["encoder_gap"].min(1) >= 2e-3) & (c["minmax_gap"].min(1) >= 2e-4) & (c["target_distance"].min(1) >= 2e-4)
    rows = np.flatnonzero(ok)[:B]
    assert len(rows) == B
    b = cut_rows(pool, rows)
    return StochEdge(m, b, _verifier(b, S))


STOCH_EDGE_CASES = {
    "ties_repr-E32": lambda d, s: _edge_ties_repr(WIDE, s, d),
    "ties_repr-E8": lambda d, s: _edge_ties_repr(PAD, s, d),
    "ties_after-E32": lambda d, s: _edge_ties_second_layer(WIDE, "ad", s, d),
    "ties_after-E8": lambda d, s: _edge_ties_second_layer(PAD, "ad", s, d),
    "ties_next-E32": lambda d, s: _edge_ties_second_layer(WIDE, "cn", s, d),
    "ties_next-E8": lambda d, s: _edge_ties_second_layer(PAD, "cn", s, d),
    "all_tied-E32": lambda d, s: _edge_all_tied(WIDE, s, d),
    "all_tied-E8": lambda d, s: _edge_all_tied(PAD, s, d),
    "near_degenerate-2^-18": lambda d, s: _edge_near_degenerate(-18, s, d),
    "near_degenerate-2^-16": lambda d, s: _edge_near_degenerate(-16, s, d),
    "encoder_tie_first-C32": lambda d, s: _edge_encoder_tie(WIDE, (3, 19), s, d),
    "encoder_tie_first-C17": lambda d, s: _edge_encoder_tie(PAD, (0, 16), s, d),
    **{f"large_logits-{n}-{int(reach)}": (lambda d, s, shape=shape, reach=reach: _edge_large_logits(shape, reach, s, d))
       for n, shape in (("F63", WIDE), ("C17", PAD)) for reach in (50.0, 300.0)},
    "policy_targets": lambda d, s: _edge_policy_targets(s, d),
    "policy_targets-all_zero": lambda d, s: _edge_policy_targets(s, d, zero=True),
    "support_edges-8": lambda d, s: _edge_support(PAD, s, d),
    "support_edges-31": lambda d, s: _edge_support(WIDE, s, d),
    "absent_actions-first": lambda d, s: _edge_absent_actions(PAD, 0, s, d),
    "absent_actions-last": lambda d, s: _edge_absent_actions(MID, 3, s, d),
    "zero_weight_rows": lambda d, s: _edge_zero_weight_rows(s, d),
    **{f"batch_edges-{B}": (lambda d, s, B=B: _edge_batch(B, s, d)) for B in (15, 16, 17, 63, 65)},
    "large_reduction": lambda d, s: _edge_large_reduction(s, d),
}


# the same inputs on an on-demand instance (tests/test_gpu_stochastic_train_jit.py builds it): E = 17 puts a partner of
# the three-way maximum in the one real lane of slot 1
JIT_SHAPE = (5, 32, 17, 10, 16)
STOCH_JIT_EDGE_CASES = {
    "ties_repr-E17": lambda d, s: _edge_ties_repr(JIT_SHAPE, s, d),
    "encoder_tie_first-E17": lambda d, s: _edge_encoder_tie(JIT_SHAPE, (3, 19), s, d),
}


def edge_case(name, device=None, seed=None):
    """The case `name` at its listed seed (`seed`: another, for picking one)."""
    build = STOCH_EDGE_CASES.get(name) or STOCH_JIT_EDGE_CASES[name]
    return build(device, EDGE_SEEDS[name] if seed is None else seed)
