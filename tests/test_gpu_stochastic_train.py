"""The fused training step of the default stochastic MLP family (muax_amd/csrc/mz_stoch_train.cuh through
mzs_stochastic_mlp_loss_grad and loss.StochasticFusedLossGrad) against float64 autograd on the CPU
(tests/stochastic_train_reference.py): the loss to 1e-5 relative, each of the 34 gradient arrays to 2e-4 of the array's
largest reference entry (floor 1e-6) -- the bound of tests/test_gpu_train.py for the same arithmetic (fp32 accumulation
over B L terms in another order).  The torch fp32 route on the GPU is measured against the same reference and printed.

The batches are conditioned, which is not a tolerance: the float64 reference's encoder top-two gap is at least 1e-3 and
no normaliser tie gap or target-to-integer distance is below 1e-4 for ANY row and step, so that float32 and float64
take the same argmax, min / max and floor everywhere.  The batch seeds below were picked on the CPU for that; every test
asserts it."""
import functools

import numpy as np
import pytest
import torch

import stochastic_train_reference as ref

pytestmark = pytest.mark.gpu
F32 = np.float32
SENTINEL = 0x5A5AA5A5
GUARD = 37
MODEL_SEED = 11
# batch seed per (index into ref.SHAPES, B, L): the first seed from 0 whose batch meets the conditions
BATCH_SEED = {
    (0, 1, 1): 0, (0, 1, 2): 0, (0, 1, 5): 0, (0, 16, 1): 0, (0, 16, 2): 0, (0, 16, 5): 0, (0, 17, 1): 0, (0, 17, 2): 0,
    (0, 17, 5): 0,
    (1, 1, 1): 0, (1, 1, 2): 0, (1, 1, 5): 0, (1, 16, 1): 0, (1, 16, 2): 1, (1, 16, 5): 4, (1, 17, 1): 0, (1, 17, 2): 1,
    (1, 17, 5): 1,
    (2, 1, 1): 0, (2, 1, 2): 0, (2, 1, 5): 0, (2, 16, 1): 0, (2, 16, 2): 0, (2, 16, 5): 0, (2, 17, 1): 0, (2, 17, 2): 0,
    (2, 17, 5): 1,
}
EQUAL_LOGITS_SEED = 0  # shape 1, B = 17, L = 5 with the encoder's w2 = 0: normaliser and target conditions only


@functools.lru_cache(maxsize=None)
def _model(si):
    return ref.smz_model(*ref.SHAPES[si], seed=MODEL_SEED + si)


@functools.lru_cache(maxsize=None)
def _case(si, B, L):
    """(model, batch, float64 loss, float64 gradients), computed once and shared; nothing below modifies them."""
    A, _, _, _, od = ref.SHAPES[si]
    m, b = _model(si), ref.smz_batch(B, L, A, od, BATCH_SEED[si, B, L])
    assert ref.well_conditioned(ref.conditions(m, b)), "pick another batch seed"
    return (m, b) + ref.autograd(m, b)


def _fused(m):
    import muax_amd as mx
    return mx.loss.StochasticFusedLossGrad(m)


def _run(f, b, **kw):
    loss, flat = f(b, **kw)
    return float(loss.item()), flat.clone(), [v.detach().cpu().numpy().copy() for v in f.views]


def _check(loss, views, l64, g64, note=""):
    from muax_amd._lib import STOCHASTIC_TRAIN_WEIGHT_NAMES as NAMES
    ek = ref.rel_errors(views, g64)
    lk = abs(loss - l64) / abs(l64)
    print(f"[{note} kernel loss {lk:.1e} grad {max(ek):.1e} ({NAMES[int(np.argmax(ek))]})]", end=" ")
    assert np.isfinite(loss) and all(np.isfinite(v).all() for v in views)
    assert lk <= 1e-5, (loss, l64)
    for n, v, d, e in zip(NAMES, views, g64, ek):
        assert v.shape == d.shape and e <= 2e-4, (n, e)


@pytest.mark.parametrize("L", [1, 2, 5])
@pytest.mark.parametrize("B", [1, 16, 17])
@pytest.mark.parametrize("si", [0, 1, 2])
def test_loss_and_gradients_against_float64(si, B, L):
    """Loss and all 34 arrays against float64, the torch fp32 route printed beside it; a second call on the same handle
    is bit-identical; at L = 1 there is no transition, and the gradients of everything but the representation and the
    prediction net are exactly l2 * w."""
    from muax_amd._lib import STOCHASTIC_TRAIN_WEIGHT_NAMES as NAMES
    m, b, l64, g64 = _case(si, B, L)
    f = _fused(m)
    loss, flat, views = _run(f, b)
    l32, g32 = ref.autograd(m, b, torch.float32, "cuda")
    print(f"[torch fp32 loss {abs(l32 - l64) / abs(l64):.1e} grad {max(ref.rel_errors(g32, g64)):.1e}]", end=" ")
    _check(loss, views, l64, g64)
    loss2, flat2, _ = _run(f, b)
    assert loss2 == loss and torch.equal(flat2, flat)
    if L == 1:
        for n, v, p in zip(NAMES, views, f.params):
            if n[:2] in ("ad", "av", "ac", "cr", "cn", "en"):
                assert np.array_equal(v, (F32(1e-4) * p.detach().cpu().numpy()).astype(F32)), n


def test_the_examples_shape_against_float64():
    """(A, C, E, F) = (4, 32, 32, 63), examples/fit_2048_stochastic.py's: the listed instance with the most accumulator
    tiles (two slots for E and C, four for F and E + C), at B = 17, L = 5 under the same conditions and bound."""
    A, Cn, E, S, od = 4, 32, 32, 31, 16
    m, b = ref.smz_model(A, Cn, E, S, od, seed=14), ref.smz_batch(17, 5, A, od, 1)
    assert ref.well_conditioned(ref.conditions(m, b)), "pick another batch seed"
    l64, g64 = ref.autograd(m, b)
    loss, _, views = _run(_fused(m), b)
    _check(loss, views, l64, g64)


@pytest.mark.parametrize("si", [0, 1, 2])
def test_guard_words_behind_every_output(si):
    m, b, l64, g64 = _case(si, 17, 5)
    f = _fused(m)
    f(b)  # sizes the workspace
    n, nws = f.grads.numel(), f._ws.numel()
    bufs = [torch.full((k + GUARD,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32) for k in (n, 1, nws)]
    f.grads, f.loss, f._ws = bufs[0][:n], bufs[1][:1], bufs[2][:nws]
    loss, flat = f(b)
    views, off = [], 0
    for p in f.params:
        views.append(flat[off:off + p.numel()].view_as(p).cpu().numpy())
        off += p.numel()
    _check(float(loss.item()), views, l64, g64)
    for buf, k in zip(bufs, (n, 1, nws)):
        assert (buf.view(torch.int32)[k:] == SENTINEL).all()
    assert (bufs[0].view(torch.int32)[:n] != SENTINEL).all()


def test_equal_encoder_logits_pick_code_zero():
    """w2 = 0 and equal b2: all C logits are bit-equal in fp32 and fp64; torch.argmax on the CPU returns index 0 and so
    must the kernel, or the chance dynamics' inputs -- and with them most gradients -- would differ."""
    si, B, L = 1, 17, 5
    A, _, _, _, od = ref.SHAPES[si]
    m = ref.smz_model(*ref.SHAPES[si], seed=MODEL_SEED + si)
    with torch.no_grad():
        m.enc_func.enc_func[1].w.zero_()
        m.enc_func.enc_func[1].b.fill_(0.375)
    b = ref.smz_batch(B, L, A, od, EQUAL_LOGITS_SEED)
    cond = ref.conditions(m, b)
    assert (cond["encoder_gap"] == 0).all() and cond["minmax_gap"].min() >= 1e-4 and cond["target_distance"].min() >= 1e-4
    l64, g64 = ref.autograd(m, b)
    loss, _, views = _run(_fused(m), b)
    _check(loss, views, l64, g64)


def test_gradient_does_not_depend_on_the_split():
    """B = 17 in one call against rows 0..15 and row 16 in calls of their own at the same scale per row (the wrapper's
    1/B times a constant sample weight), summed, the L2 term counted once."""
    for si in (0, 1, 2):
        m, b, l64, g64 = _case(si, 17, 5)
        f = _fused(m)
        parts = []
        for rows in (slice(0, 16), slice(16, 17)):
            nb = 16 if rows.start == 0 else 1
            sw = torch.full((nb,), nb / 17.0, device="cuda")
            parts.append(_run(f, ref.cut_rows(b, rows), sample_weight=sw))
        l2w = [1e-4 * p.detach().cpu().double().numpy() for p in f.params]
        l2 = 0.5 * sum(float((w * w).sum()) for w in l2w) / 1e-4
        views = [x.astype(np.float64) + y - w for x, y, w in zip(parts[0][2], parts[1][2], l2w)]
        _check(parts[0][0] + parts[1][0] - l2, views, l64, g64, note=f"shape {si} split")


def test_sample_weight_vqvae_beta_and_divide_by_length():
    si, B, L = 2, 17, 5
    m, b, l64, g64 = _case(si, B, L)
    f = _fused(m)
    loss, flat, _ = _run(f, b)
    loss1, flat1, _ = _run(f, b, sample_weight=torch.ones(B, device="cuda"))
    assert loss1 == loss and torch.equal(flat1, flat)  # weights of 1 give the unweighted bits
    # a zero weight on row 5 == the batch without that row at the same scale per row (1/17)
    sw = torch.ones(B, device="cuda")
    sw[5] = 0.0
    _, _, vz = _run(f, b, sample_weight=sw)
    keep = [k for k in range(B) if k != 5]
    lr, gr = ref.autograd(m, ref.cut_rows(b, keep), sample_weight=np.full(B - 1, (B - 1) / B))
    lz, _, _ = _run(f, b, sample_weight=sw)
    _check(lz, vz, lr, gr, note="zero weight")
    _, _, vw = _run(f, ref.cut_rows(b, keep), sample_weight=torch.full((B - 1,), (B - 1) / B, device="cuda"))
    for n, x, y, d in zip(range(34), vz, vw, gr):
        assert np.abs(x.astype(np.float64) - y).max() <= 2e-4 * max(np.abs(d).max(), 1e-6), n
    # random weights, another beta, the coax division
    w = np.random.default_rng(1).uniform(0.2, 3.0, B).astype(F32)
    for kw in (dict(sample_weight=w), dict(vqvae_beta=0.7), dict(divide_by_length=True),
               dict(sample_weight=w, vqvae_beta=1.5, divide_by_length=True)):
        lref, gref = ref.autograd(m, b, **kw)
        kk = dict(kw, sample_weight=torch.from_numpy(w).cuda()) if "sample_weight" in kw else kw
        lk, _, vk = _run(f, b, **kk)
        _check(lk, vk, lref, gref, note=",".join(kw))


def test_refusals_happen_before_any_launch():
    """By class and message; the output buffers keep their sentinel."""
    from muax_amd import _lib

    def refused(m, b, exc, match, **kw):
        f = _fused(m)
        f.grads.view(torch.int32).fill_(SENTINEL)
        f.loss.view(torch.int32).fill_(SENTINEL)
        with pytest.raises(exc, match=match) as e:
            f(b, **kw)
        torch.cuda.synchronize()
        assert (f.grads.view(torch.int32) == SENTINEL).all() and (f.loss.view(torch.int32) == SENTINEL).all()
        return e.value
    A, Cn, E, S, od = ref.SHAPES[0]
    b = ref.smz_batch(4, 3, A, od, 0)
    assert type(refused(ref.smz_model(A, Cn, E + 1, S, od, seed=1), b, _lib.NoKernelInstance, "no kernel instance")) \
        is _lib.NoKernelInstance
    for support in (7, 32):
        refused(ref.smz_model(A, Cn, E, support, od, seed=1), b, _lib.NoKernelInstance, r"support_size must be 8\.\.31")
    e = refused(ref.smz_model(A, Cn, E, S, 33, seed=1), ref.smz_batch(4, 3, A, 33, 0), _lib.Unsupported,
                r"obs_dim must be 1\.\.32")
    assert not isinstance(e, (_lib.NoKernelInstance, _lib.TooLargeForLds))
    m = _model(0)
    refused(m, ref.smz_batch(1, 80, A, od, 0), _lib.TooLargeForLds, r"unroll_steps 80 too large for the LDS \(at most \d+")
    short = ref.cut_rows(b, slice(0, 4))
    short.obs = short.obs[:, :1]
    refused(m, short, ValueError, "needs every step's observation")
    refused(m, b, ValueError, "sample_weight must be", sample_weight=torch.ones(3, device="cuda"))


def test_model_update_takes_the_fused_route():
    """With the flag: "auto" and "hip" take the kernel; one SGD step of learning rate 1 from equal weights (the step is
    minus the gradient) matches the step of "torch" at the tolerances of
    test_gpu_train.py::test_update_hip_and_torch_routes_take_the_same_step; the next act() searches with the new weights.
    Without the flag the torch route runs and "hip" is refused."""
    import muax_amd as mx
    si, B, L, S = 1, 17, 5, 10
    A, Cn, E, support, od = ref.SHAPES[si]
    b = _case(si, B, L)[1]
    sw = torch.from_numpy(np.random.default_rng(2).uniform(0.5, 2.0, B).astype(F32)).cuda()
    steps = {}
    for backend in ("auto", "hip", "torch"):
        m = ref.smz_model(A, Cn, E, support, od, seed=MODEL_SEED + si, optimizer=("sgd", 1.0), stochastic_fused_update=True)
        before = torch.cat([p.detach().reshape(-1).clone() for p in _fused(m).params])
        out = m.update(b, backend=backend, sample_weight=sw, vqvae_beta=0.5, divide_by_length=True)
        assert m._last_update_route == ("torch" if backend == "torch" else "hip_stochastic_fused")
        steps[backend] = (out["loss"], torch.cat([p.detach().reshape(-1) for p in _fused(m).params]) - before)
    assert torch.equal(steps["auto"][1], steps["hip"][1]) and steps["auto"][0] == steps["hip"][0]
    assert np.isclose(steps["hip"][0], steps["torch"][0], rtol=2e-4)
    assert steps["torch"][1].abs().max() > 1e-2
    assert torch.allclose(steps["hip"][1], steps["torch"][1], rtol=5e-3, atol=5e-4)
    # the next act() binds the stepped weights (_weights_version)
    obs = torch.from_numpy(np.random.default_rng(3).uniform(0, 1, (5, od)).astype(F32)).cuda()
    kw = dict(with_pi=True, obs_from_batch=True, num_simulations=S, dirichlet_fraction=0.0, device_outputs=True)
    m.act([1, 2], obs, **kw)
    v = m._weights_version
    m.update(b, backend="hip")
    assert m._weights_version == v + 1 and m._last_update_route == "hip_stochastic_fused"
    a, w = m.act([1, 2], obs, **kw)
    s = mx.MuZeroSearch(5, mx.SearchConfig(A, S, E, policy="stochastic", num_chance_outcomes=Cn))
    s.set_stochastic_mlp_weights({k: t.detach() for k, t in mx.nn.stochastic_mlp_weights(m.network).items()}, support,
                                 m._discount)
    out = s.search_stochastic_mlp(m._root_inference_eager(obs), key=[1, 2], dirichlet_fraction=0.0)
    assert torch.equal(out.action, a) and torch.equal(out.action_weights.view(torch.int32), w.view(torch.int32))
    s.close()
    # "auto" falls to torch where the kernel refuses on the host, "hip" re-raises
    long = ref.smz_batch(2, 80, A, od, 0)
    with pytest.raises(mx._lib.TooLargeForLds):
        m.update(long, backend="hip")
    assert np.isfinite(m.update(long)["loss"]) and m._last_update_route == "torch"
    off = ref.smz_model(A, Cn, E, support, od, seed=MODEL_SEED + si)
    off.update(b)
    assert off._last_update_route == "torch"
    with pytest.raises(ValueError, match="torch autograd only"):
        off.update(b, backend="hip")
