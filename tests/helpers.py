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
def train_model(A, E, obs_dim, seed, support=10, bias_noise=True, optimizer=("adam", 1e-2)):
    """A default MLP trio with haiku's init; `bias_noise` adds N(0, 0.1) to every bias so that every gradient path is
    exercised (off: the zero biases of a freshly initialised net); `optimizer` is (name, learning rate)."""
    import torch

    import muax_amd as mx
    g = torch.Generator().manual_seed(seed)
    F = 2 * support + 1
    net = mx.nn.MZNetwork(mx.nn.Representation(E, generator=g), mx.nn.Prediction(A, F, generator=g),
                          mx.nn.Dynamic(E, A, F, generator=g))
    m = mx.MuZero(net, optimizer=mx.optimizers.create_optimizer(*optimizer), support_size=support)
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
