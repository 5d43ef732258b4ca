"""Shared input builders for the parity tests (seeded, no reference import) and the training step's fp64 reference."""
import numpy as np

F32 = np.float32


def make_case(oracle, seed, B, obs_dim, E, A, S, support=10, bias_scale=0.1, invalid_frac=0.0):
    F = 2 * support + 1
    w = oracle.random_mlp_weights(seed, obs_dim, E, A, F, bias_scale=bias_scale)
    rng = np.random.default_rng(seed + 1000)
    obs = rng.uniform(-1, 1, (B, obs_dim)).astype(F32)
    noise = rng.dirichlet([0.3] * A, B).astype(F32)
    gum = rng.gumbel(size=(B, A)).astype(F32)
    invalid = None
    if invalid_frac > 0:
        invalid = (rng.uniform(size=(B, A)) < invalid_frac).astype(np.uint8)
        invalid[np.arange(B), rng.integers(0, A, B)] = 0  # keep one valid action per root
        invalid[0, :] = 1                                  # ... except one all-invalid root (mctx: argmax -> 0)
    return dict(w=w, obs=obs, noise=noise, gumbel=gum, invalid=invalid, B=B, obs_dim=obs_dim, E=E, A=A,
                F=F, S=S, support=support)


def assert_trees_equal(oracle_tree, gpu_tree, exact_floats=True):
    ref = oracle_tree.arrays()
    for name, a in ref.items():
        b = getattr(gpu_tree, name).cpu().numpy()
        assert a.shape == b.shape, name
        if a.dtype == np.int32 or exact_floats:
            bad = np.argwhere(a != b)
            assert bad.size == 0, f"{name}: {len(bad)} mismatches, first at {bad[0]}: {a[tuple(bad[0])]} vs {b[tuple(bad[0])]}"
        else:
            assert np.allclose(a, b, rtol=1e-5, atol=1e-5), name


# ---- the fused training step's fp64 reference (test_gpu_train.py, test_gpu_train_edges.py) ----
def train_model(A, E, obs_dim, seed, support=10, bias_noise=True, optimizer=("adam", 1e-2), device=None):
    """A default MLP trio with haiku's init; `bias_noise` adds N(0, 0.1) to every bias so that every gradient path is
    exercised (off: the zero biases of a freshly initialised net); `optimizer` is (name, learning rate); `device` None:
    MuZero's default (the GPU when there is one).  The weights do not depend on the device (CPU generator)."""
    import torch

    import muax_amd as mx
    g = torch.Generator().manual_seed(seed)
    F = 2 * support + 1
    net = mx.nn.MZNetwork(mx.nn.Representation(E, generator=g), mx.nn.Prediction(A, F, generator=g),
                          mx.nn.Dynamic(E, A, F, generator=g))
    m = mx.MuZero(net, optimizer=mx.optimizers.create_optimizer(*optimizer), support_size=support, device=device)
    m.init(0, np.zeros((1, obs_dim)))
    if bias_noise:
        with torch.no_grad():
            for p in [p for mod in m.network for p in mod.parameters()]:
                if p.dim() == 1:
                    p.add_(0.1 * torch.randn(p.shape, generator=g).to(p.device))
    return m


def train_batch(B, L, A, obs_dim, seed):
    import muax_amd as mx
    rng = np.random.default_rng(seed)
    return mx.Transition(obs=rng.uniform(-1, 1, (B, L, obs_dim)).astype(F32), a=rng.integers(0, A, (B, L)),
                         r=rng.uniform(-2, 3, (B, L)).astype(F32), Rn=rng.uniform(-30, 60, (B, L)).astype(F32),
                         pi=rng.dirichlet(np.ones(A), (B, L)).astype(F32).reshape(B, L, 1, A))


def train_autograd(m, b, dtype, device, capture=None, **kw):
    """(loss, [gradient of every MLP_WEIGHT_NAMES array]) of muax_amd/loss.py's formula by torch autograd: float32 runs
    default_loss_fn itself, float64 restates it without its float32 casts.  `capture`, a list, receives the input of
    every min_max_normalize of the forward pass (the representation's, then each dynamics step's), detached."""
    import copy

    import torch

    import muax_amd as mx
    mods = [copy.deepcopy(x).to(device=device, dtype=dtype) for x in m.network]
    m2 = mx.MuZero(mx.nn.MZNetwork(*mods), device=device)
    m2._params, m2._support_size = True, m._support_size
    bb = mx.Transition(**{k: (torch.as_tensor(v).to(dtype) if isinstance(v, np.ndarray) and v.dtype == F32 else v)
                          for k, v in b.__dict__.items()})
    orig = mx.loss.default_loss_fn

    def loss64(inst, batch, **k2):  # the restated loss casts to float32; redo it in `dtype`
        dev = inst.device
        t = lambda x, dt=dtype: torch.as_tensor(x, device=dev).to(dt)  # noqa: E731
        a = t(batch.a, torch.long)
        B, L = a.shape[:2]
        S = inst._support_size
        r_t = mx.utils.scalar_to_support(t(batch.r).reshape(B, L), S)
        Rn_t = mx.utils.scalar_to_support(t(batch.Rn).reshape(B, L), S)
        pi = t(batch.pi).reshape(B, L, -1)
        s = inst.repr_func(t(batch.obs)[:, 0])
        loss = 0
        for i in range(L):
            v, lg = inst.pred_func(s)
            s = mx.utils.scale_gradient(s, 0.5)
            r, ns = inst.dy_func(s, a[:, i])
            ce = mx.loss.softmax_cross_entropy
            loss = loss + ce(r, r_t[:, i]).mean() + ce(v, Rn_t[:, i]).mean() + ce(lg, pi[:, i]).mean()
            s = ns
        if k2.get("divide_by_length"):
            loss = loss / L
        return loss + 1e-4 * 0.5 * sum((p ** 2).sum() for mod in inst.network for p in mod.parameters())

    norm = mx.nn.min_max_normalize
    if capture is not None:
        def recording(s):
            capture.append(s.detach().cpu())
            return norm(s)
        mx.nn.min_max_normalize = recording
    try:
        loss = (loss64 if dtype == torch.float64 else orig)(m2, bb if dtype == torch.float64 else b, **kw)
    finally:
        mx.nn.min_max_normalize = norm
    loss.backward()
    w = mx.nn.mlp_trio_weights(m2.network)
    from muax_amd._lib import MLP_WEIGHT_NAMES
    return float(loss.detach()), [w[n].grad.detach().cpu().double().numpy() for n in MLP_WEIGHT_NAMES]


def support_edge_scalars(support, ks=(1, 2, 5, -3)):
    """float32 scalars at the edges of the value codec (muax/utils.py:65-91) with h(x) = sign(x) (sqrt(|x| + 1) - 1)
    + 1e-3 x: 0 and +-1; for each integer k of `ks` and for k = +-support (the clip), the float32 x nearest the fp64
    root of h(x) = k (bisection) and its four neighbours on either side, so that h(x) lands on k, or one float32 ulp
    either side of it, or just inside / outside the clip; and +-200, +-1e4, +-1e7 (far beyond it)."""
    def h(x):
        return np.sign(x) * (np.sqrt(abs(x) + 1.0) - 1.0) + 1e-3 * x
    out = [0.0, 1.0, -1.0]
    for k in tuple(ks) + (support, -support):
        lo, hi = (0.0, 1e6) if k > 0 else (-1e6, 0.0)
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if h(mid) < k else (lo, mid)
        c = [F32(hi)]
        for _ in range(4):
            c = [np.nextafter(c[0], F32(-np.inf)), *c, np.nextafter(c[-1], F32(np.inf))]
        out += c
    out += [200.0, -200.0, 1e4, -1e4, 1e7, -1e7]
    return np.array(out, F32)


# ---- the independent NumPy reference and the edge inputs at multi-slot shapes, shared by the CPU arbitration test
# (test_train_reference_cpu.py) and the GPU tests (test_gpu_wide_train_edges.py, test_gpu_train_lattice.py) ----
def trio_arrays(m):
    """The 18 arrays of the model as float32 NumPy copies, by name."""
    import muax_amd as mx
    return {n: t.detach().cpu().numpy().copy() for n, t in mx.nn.mlp_trio_weights(m.network).items()}


def set_trio(m, **arrays):
    import torch

    import muax_amd as mx
    w = mx.nn.mlp_trio_weights(m.network)
    with torch.no_grad():
        for n, v in arrays.items():
            w[n].copy_(torch.as_tensor(np.asarray(v), dtype=torch.float32))


def train_numpy(m, b, trace=None, **kw):
    """(loss, [gradient of every MLP_WEIGHT_NAMES array]) of oracle/mz_train_numpy.py -- float64, hand-derived
    backward, no torch and no muax_amd inside -- on the model's float32 weights and the batch."""
    from muax_amd._lib import MLP_WEIGHT_NAMES
    from oracle import mz_train_numpy as ref
    args = (trio_arrays(m), b.obs[:, 0], b.a, b.r, b.Rn, b.pi, m._support_size)
    if trace is not None:
        ref.forward(*args, trace=trace, **kw)
    loss, g = ref.loss_and_grads(*args, **kw)
    return loss, [g[n] for n in MLP_WEIGHT_NAMES]


def dyadic(rng, shape, step, lim):
    return (rng.integers(-int(lim / step), int(lim / step) + 1, shape) * step).astype(F32)


# The covering set of on-demand shapes, narrow and wide: (A, E, support, obs_dim).  Every E in {1, 15, 17, 33, 63}, every
# F = 2 support + 1 in {17, 33, 49, 63}, every A in {1, 15, 16, 17, 49, 64}, every X = E + A in {16, 17, 32, 33, 64, 65,
# 128} and every obs_dim in {1, 17, 128} appears at least once.
TRAIN_LATTICE = [(1, 15, 8, 1), (16, 1, 16, 17), (15, 17, 24, 128), (16, 17, 31, 4), (1, 63, 10, 4), (49, 15, 10, 17),
                 (64, 1, 10, 1), (32, 33, 16, 128), (64, 64, 31, 16), (17, 15, 10, 4), (17, 16, 10, 4), (17, 33, 8, 17)]


def lattice_case(A, E, support, obs_dim, device=None):
    seed = 1000 * A + 10 * E + support
    return train_model(A, E, obs_dim, seed=seed, support=support, device=device), train_batch(37, 3, A, obs_dim, seed=seed)


class EdgeCase:
    """One edge input: the model `m`, the batch `b`, `verify(cap)` asserting the construction on the captured
    normaliser inputs (the representation's, then one per dynamics step), `absent` the actions that occur nowhere in
    the batch (None: not that kind of case) and `pi_zero` (every policy target row zero)."""

    def __init__(self, m, b, verify=None, absent=None, pi_zero=False):
        self.m, self.b, self.verify, self.absent, self.pi_zero = m, b, verify, absent, pi_zero


def _tied(u, cols):
    return bool((u[:, cols] == u[:, cols[:1]]).all())


_TIE_COLS = {40: ((3, 35), (5, 21, 39)), 64: ((3, 35), (5, 21, 63))}  # (min partners, max partners): different slots


def _verify_ties(E, which):
    mins, maxs = _TIE_COLS[E]

    def verify(cap):
        caps = cap[:1] if which == "repr" else cap[1:]
        assert caps
        for u in caps:
            u = np.asarray(u)
            assert _tied(u, list(mins)) and _tied(u, list(maxs))
            assert (u[:, mins[0]] == u.min(1)).all() and (u[:, maxs[0]] == u.max(1)).all()
            assert ((u == u.min(1, keepdims=True)).sum(1) == len(mins)).all()
            assert ((u == u.max(1, keepdims=True)).sum(1) == len(maxs)).all()
    return verify


def _edge_ties_dn(A, E, device, shift=0.0):
    """dn_w2 columns (and biases) duplicated so that the next state's min ties between two columns of different slots
    and its max three ways across three slots, at every unroll step; `shift` is added to pp_b2.  Each tied column
    keeps ONE non-zero weight (row 2 for the min's partners, row 11 for the max's): elu(h) W2 + b2 is then
    round(round(a_k w) + b) there whatever the order a matrix product sums in, so the ties hold in every
    implementation and precision -- fully duplicated columns tie only where the product happens to treat columns
    3, 35 and 63 alike, which a float64 BLAS need not."""
    m, b = train_model(A, E, 4, seed=A + E, support=31, device=device), train_batch(36, 4, A, 4, seed=A + E)
    w = trio_arrays(m)
    (lo0, *lo), (hi0, *hi) = _TIE_COLS[E]
    W2, b2 = w["dn_w2"], w["dn_b2"]
    for cols, k in (([lo0, *lo], 2), ([hi0, *hi], 11)):
        keep = W2[k, cols[0]]
        W2[:, cols] = 0.0
        W2[k, cols] = keep
    b2[[lo0, *lo]], b2[[hi0, *hi]] = -20.0, 20.0
    set_trio(m, dn_w2=W2, dn_b2=b2, pp_b2=w["pp_b2"] + F32(shift))
    return EdgeCase(m, b, _verify_ties(E, "dn"))


def _edge_ties_repr(A, E, device):
    """The same ties in the representation: repr_w columns duplicated, weights and observations dyadic so that
    obs W + b is exact in fp32 and fp64 alike."""
    od = 4
    m, b = train_model(A, E, od, seed=A + E + 1, support=31, device=device), train_batch(40, 3, A, od, seed=A + E + 1)
    rng = np.random.default_rng(5)
    W, bias = dyadic(rng, (od, E), 1 / 16, 0.5), dyadic(rng, E, 1 / 16, 0.5)
    (lo0, *lo), (hi0, *hi) = _TIE_COLS[E]
    for c in lo:
        W[:, c] = W[:, lo0]
    for c in hi:
        W[:, c] = W[:, hi0]
    bias[[lo0, *lo]], bias[[hi0, *hi]] = -6.0, 6.0
    b.obs[:] = dyadic(rng, b.obs.shape, 1 / 8, 1.0)
    set_trio(m, repr_w=W, repr_b=bias)
    return EdgeCase(m, b, _verify_ties(E, "repr"))


def _edge_all_tied(A, E, device):
    """A fresh net (zero biases) on all-zero first observations: all E entries of obs W + b are both min and max."""
    m, b = train_model(A, E, 4, seed=A + E + 2, support=31, bias_noise=False, device=device), \
        train_batch(32, 4, A, 4, seed=A + E + 2)
    b.obs[:, 0] = 0.0

    def verify(cap):
        u = np.asarray(cap[0])
        assert u.shape[1] == E and float(np.abs(u).max()) == 0.0
    return EdgeCase(m, b, verify)


def _edge_near_degenerate(log2_range, device):
    """(A, E) = (33, 40): repr_w's columns equal and dyadic, the biases 0.25 + range * (eighths) with the single
    minimum in slot 1 (column 20), the single maximum in the partial last slot (column 39) and the grades in between
    over all three slots: every row's range is exactly 2^log2_range in fp32 and fp64."""
    A, E, od = 33, 40, 4
    m, b = train_model(A, E, od, seed=29, support=31, device=device), train_batch(32, 3, A, od, seed=29)
    rng = np.random.default_rng(7)
    W = np.repeat(dyadic(rng, od, 1 / 64, 0.5)[:, None], E, 1)
    c = 2.0 ** log2_range
    frac = np.array([(1 + k % 7) / 8 for k in range(E)])
    frac[20], frac[39] = 0.0, 1.0
    b.obs[:] = dyadic(rng, b.obs.shape, 1 / 8, 1.0)
    set_trio(m, repr_w=W, repr_b=(0.25 + c * frac).astype(F32))

    def verify(cap):
        u = np.asarray(cap[0])
        assert ((u.max(1) - u.min(1)) == c).all() and (c < 1e-5) == (log2_range == -18)
        assert (u.argmin(1) == 20).all() and (u.argmax(1) == 39).all()
    return EdgeCase(m, b, verify)


_PAD_SHAPES = {17: 8, 33: 16, 49: 24}  # A -> support: one real lane in the last slot of the policy AND support heads


def _pad_model(A, device, seed_off=0):
    S = _PAD_SHAPES[A]
    return train_model(A, 8, 4, seed=A + seed_off, support=S, device=device), train_batch(40, 3, A, 4, seed=A + seed_off)


def _edge_policy_shift(A, shift, device):
    """pp_b2 shifted by `shift`: at -300 every real logit is near -300 while a pad lane's raw value is 0."""
    m, b = _pad_model(A, device)
    set_trio(m, pp_b2=trio_arrays(m)["pp_b2"] + F32(shift))
    return EdgeCase(m, b)


def _edge_policy_equal(A, device):
    """pp_w2 = 0 and a constant pp_b2: all policy logits exactly equal (softmax 1 / A over the real lanes only)."""
    m, b = _pad_model(A, device, 1)
    w = trio_arrays(m)
    set_trio(m, pp_w2=0 * w["pp_w2"], pp_b2=0 * w["pp_b2"] + F32(0.75))
    return EdgeCase(m, b)


def _edge_large_logits(A, E, support, device, reach=300.0):
    """The output layers of all three heads scaled until their logits reach about +-reach (test_large_logits)."""
    import torch

    import muax_amd as mx
    m, b = train_model(A, E, 4, seed=A + E + 3, support=support, device=device), train_batch(48, 3, A, 4, seed=A + E + 3)
    w = mx.nn.mlp_trio_weights(m.network)
    with torch.no_grad():
        s = m.repr_func(torch.as_tensor(b.obs[:, 0], device=m.device))
        v, lg = m.pred_func(s)
        r, _ = m.dy_func(s, torch.as_tensor(b.a[:, 0], device=m.device))
        for (wn, bn), out in ((("pv_w2", "pv_b2"), v), (("pp_w2", "pp_b2"), lg), (("dr_w2", "dr_b2"), r)):
            f = reach / float(out.abs().max())
            w[wn].mul_(f)
            w[bn].mul_(f)
        v, lg = m.pred_func(s)
    assert 0.7 * reach <= float(v.abs().max()) <= 1.3 * reach and 0.7 * reach <= float(lg.abs().max()) <= 1.3 * reach
    return EdgeCase(m, b)


def _edge_support_clip(A, device):
    """Value targets at the codec's edges and far beyond the clip: the two-hot mass sits on bin 0 and on bin F - 1, the
    one real lane of the support heads' last slot."""
    S = _PAD_SHAPES[A]
    x = support_edge_scalars(S)
    m, b = train_model(A, 8, 4, seed=A + 2, support=S, device=device), train_batch(len(x), 2, A, 4, seed=A + 2)
    b.r[:] = np.stack([x, x[::-1]], 1)
    b.Rn[:] = np.stack([np.roll(x, 7), -x], 1)
    b.r[:6], b.Rn[:6] = F32(1e4), F32(-1e4)
    b.r[6:12, 0], b.Rn[6:12, 1] = F32(-1e7), F32(1e7)
    return EdgeCase(m, b)


def _edge_onehot(A, E, pattern, device, pi_zero=False):
    """Batches whose actions are all 0, all A - 1, or all drawn from one 16-lane slot, where E + a crosses a slot
    edge: the dr_w1 / dn_w1 rows of every absent action get exact zeros from the data."""
    B, L = 40, 3
    m, b = train_model(A, E, 4, seed=A + E + 4, device=device), train_batch(B, L, A, 4, seed=A + E + 4)
    rng = np.random.default_rng(A + E)
    if pattern == "first":
        b.a[:] = 0
    elif pattern == "last":
        b.a[:] = A - 1
    else:  # one slot: the third where there is one, else part of the first
        lo, hi = (32, 48) if A > 48 else (3, 13)
        b.a[:] = rng.integers(lo, hi, (B, L))
    if pi_zero:
        b.pi[:] = 0.0
    absent = sorted(set(range(A)) - set(np.unique(b.a).tolist()))
    assert absent
    return EdgeCase(m, b, absent=absent, pi_zero=pi_zero)


def _edge_large_reduction(device):
    """(64, 64, support 31) at B = 16384, L = 2: 4096 wavefront partials per gradient entry."""
    return EdgeCase(train_model(64, 64, 16, seed=9, support=31, device=device), train_batch(16384, 2, 64, 16, seed=9))


WIDE_EDGE_CASES = {
    "ties_dn-18-64": lambda d: _edge_ties_dn(18, 64, d),
    "ties_dn-33-40-policy_shift_m300": lambda d: _edge_ties_dn(33, 40, d, shift=-300.0),
    "ties_repr-18-64": lambda d: _edge_ties_repr(18, 64, d),
    "ties_repr-33-40": lambda d: _edge_ties_repr(33, 40, d),
    "all_tied-18-64": lambda d: _edge_all_tied(18, 64, d),
    "all_tied-64-64": lambda d: _edge_all_tied(64, 64, d),
    "near_degenerate-2^-18": lambda d: _edge_near_degenerate(-18, d),
    "near_degenerate-2^-16": lambda d: _edge_near_degenerate(-16, d),
    **{f"policy_shift-{A}-{int(s):+d}": (lambda d, A=A, s=s: _edge_policy_shift(A, s, d))
       for A in _PAD_SHAPES for s in (-300.0, 300.0)},
    **{f"policy_equal-{A}": (lambda d, A=A: _edge_policy_equal(A, d)) for A in _PAD_SHAPES},
    "large_logits-33-8": lambda d: _edge_large_logits(33, 8, 16, d),
    "large_logits-64-64": lambda d: _edge_large_logits(64, 64, 31, d),
    **{f"support_clip-{A}": (lambda d, A=A: _edge_support_clip(A, d)) for A in _PAD_SHAPES},
    **{f"onehot-{A}-{E}-{p}": (lambda d, A=A, E=E, p=p: _edge_onehot(A, E, p, d))
       for A, E in ((17, 15), (17, 16), (64, 63)) for p in ("first", "last", "slot")},
    "onehot-17-16-slot-pi_zero": lambda d: _edge_onehot(17, 16, "slot", d, pi_zero=True),
    "onehot-64-63-last-pi_zero": lambda d: _edge_onehot(64, 63, "last", d, pi_zero=True),
    "large_reduction-64-64": _edge_large_reduction,
}


# ---- the GPU check shared by test_gpu_wide_train_edges.py and test_gpu_train_lattice.py ----
def fused_loss_grad(m):
    """FusedLossGrad of the model, its on-demand instance registered first (update() does that itself)."""
    import muax_amd as mx
    from muax_amd import _jit
    f = mx.loss.FusedLossGrad(m)
    ensure = _jit.ensure_wide_train_instance if f.A > 16 else _jit.ensure_train_instance
    assert ensure(f.A, f.E, 2 * f.S + 1), _jit.build_log_tail()
    return f


def _rel_errors(views, ref):
    return [float(np.abs(g - d).max() / max(np.abs(d).max(), 1e-6)) for g, d in zip(views, ref)]


def check_train_step(m, b, verify=None, **kw):
    """The kernel's loss and gradients against fp64 autograd and against the NumPy reference, a second call
    bit-identical; `verify` runs on the normaliser inputs captured from the fp64 and from the torch fp32 route.
    Returns the kernel's gradients as float32 arrays by name."""
    import torch

    from muax_amd._lib import MLP_WEIGHT_NAMES
    fused = fused_loss_grad(m)
    loss, flat = fused(b, **kw)
    loss, views32 = float(loss.item()), [v.detach().cpu().numpy().copy() for v in fused.views]
    views = [v.astype(np.float64) for v in views32]
    flat = flat.clone()
    cap64, cap32 = [], []
    l64, g64 = train_autograd(m, b, torch.float64, "cpu", capture=cap64, **kw)
    l32, g32 = train_autograd(m, b, torch.float32, "cuda", capture=cap32, **kw)
    lnp, gnp = train_numpy(m, b, **kw)
    ek, et, en = _rel_errors(views, g64), _rel_errors(g32, g64), _rel_errors(views, gnp)
    lk, lt, ln = abs(loss - l64) / abs(l64), abs(l32 - l64) / abs(l64), abs(loss - lnp) / abs(lnp)
    print(f"[kernel loss {lk:.1e} grad {max(ek):.1e} | against NumPy loss {ln:.1e} grad {max(en):.1e} | "
          f"torch fp32 loss {lt:.1e} grad {max(et):.1e}]", end=" ")
    if verify is not None:
        verify([c.numpy() for c in cap64])
        verify([c.numpy() for c in cap32])
    assert all(np.isfinite(v).all() for v in views) and np.isfinite(loss)
    for n, gh, gd, e_k, e_n, e_t in zip(MLP_WEIGHT_NAMES, views, g64, ek, en, et):
        assert gh.shape == gd.shape
        assert e_k <= 2e-4, (n, e_k, e_t)
        assert e_n <= 2e-4, (n, e_n, e_t)
    assert lk <= 1e-5 and ln <= 1e-5, (loss, l64, lnp, l32)
    loss2, flat2 = fused(b, **kw)  # fixed-order reduction: bit-reproducible
    assert float(loss2.item()) == loss and torch.equal(flat2, flat)
    return dict(zip(MLP_WEIGHT_NAMES, views32))
