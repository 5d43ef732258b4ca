"""On-demand instances of the stochastic family's fused training step (muax_amd/csrc/mz_stoch_train_jit.hip through
_jit.ensure_stochastic_train_instance and mzs_register_stochastic_train_dispatch) against float64 autograd of
loss.stochastic_loss_fn on the CPU.  The comparison (`_check`), the conditioning filter (`well_conditioned`) and the bars
are those of test_gpu_stochastic_train.py::test_loss_and_gradients_against_float64: loss to 1e-5 relative, each of the 34
arrays to 2e-4 of its largest reference entry (floor 1e-6).

The batch seeds were picked on the CPU (float64 autograd alone, no GPU) as the first seed from 0 whose WHOLE batch meets
the conditions: the filter drops nothing, the kept share of (row, step) cases is 17 x 3 of 17 x 3 = 100 %, so every step
index and both workgroups (16 rows + 1 live row) stay covered; every test asserts it.

The lattice is six instances at B = 17, L = 3, each on a 16-lane slot edge the listed instances miss.  Three are the
nearest neighbours of the shapes first proposed, whose builds report scratch (profiles/stochastic_train.txt: the kernel
is register-bound, the plan's tile budget is necessary but not sufficient), so _jit never registers them:
  (5, 33, 17, 21, obs 16) -> (5, 32, 17, 21, obs 16)   E = 17 and XC = 49 cross a slot edge; C = 33 spills 72 bytes
  (2, 62, 64, 17, obs 65) -> (2, 62, 16, 17, obs 65)   A + C = 64, XC = 78, cap 96; E = 64 is beyond the plan's tile budget
  (7, 20, 33, 35, obs 32) -> (7, 20, 32, 35, obs 32)   obs_dim = cap = 32, F = 35 in three slots; E = 33 spills / fails to build
A fourth, (1, 1, 1, 17, obs 1), became (1, 2, 3, 17, obs 1): the reference's conditioning measure (top-two encoder gap,
two-smallest / two-largest normaliser gap) needs two entries per vector, and with E <= 2 every normalised state is the
constant (0, 1), so the gradient in front of a normaliser is zero in exact arithmetic and the comparison would measure
fp32 cancellation noise against the L2 term (2.9e-3 of repr_b's largest entry at E = 2, on either fp32 route).
No test here registers (3, 2, 5, 17) or (3, 2, 4, 17), which test_gpu_stochastic_train.py expects refused."""
import functools

import numpy as np
import pytest
import torch

import stochastic_train_reference as ref
from test_gpu_stochastic_train import GUARD, SENTINEL, _check, _fused, _run

pytestmark = pytest.mark.gpu
F32 = np.float32
B, L = 17, 3
# (A, C, E, support, obs_dim) -> (model seed, batch seed at (B, L) = (17, 3))
LATTICE = {
    (1, 2, 3, 8, 1): (21, 0),
    (16, 17, 15, 31, 33): (22, 1),
    (5, 32, 17, 10, 16): (23, 0),
    (4, 48, 16, 20, 128): (24, 0),
    (2, 62, 16, 8, 65): (25, 0),
    (7, 20, 32, 17, 32): (26, 0),
}
LONG_SHAPE, LONG_L, LONG_SEED = (5, 32, 17, 10, 16), 12, 0  # the longest unroll its plan admits, capped at 12
CAP32_SHAPE = (3, 4, 5, 8, 20)     # an instance at cap 32 of a shape no other test uses: 33 observations are refused
MODEL_SHAPE = (6, 20, 8, 10, 40)   # the model-level test's own shape (cap 64): registered by that test only


def _ensure(shape):
    from muax_amd import _jit
    A, Cn, E, S, od = shape
    assert _jit.ensure_stochastic_train_instance(A, Cn, E, 2 * S + 1, od), _jit.build_log_tail()
    info = _jit.stochastic_train_instance_info(A, Cn, E, 2 * S + 1, od)
    assert info["scratch_bytes"] == 0
    return info


@functools.lru_cache(maxsize=None)
def _case(shape, Bn=B, Ln=L, batch_seed=None):
    """(model, batch, float64 loss, float64 gradients), computed once and shared; nothing below modifies them."""
    A, _, _, _, od = shape
    mseed, bseed = LATTICE[shape]
    m = ref.smz_model(*shape, seed=mseed)
    b = ref.smz_batch(Bn, Ln, A, od, bseed if batch_seed is None else batch_seed)
    assert ref.well_conditioned(ref.conditions(m, b)), "pick another batch seed"
    return (m, b) + ref.autograd(m, b)


@pytest.mark.parametrize("shape", list(LATTICE))
def test_lattice_against_float64(shape):
    """Loss and all 34 arrays against float64 on an on-demand instance; a second call is bit-identical."""
    _ensure(shape)
    m, b, l64, g64 = _case(shape)
    f = _fused(m)
    loss, flat, views = _run(f, b)
    _check(loss, views, l64, g64)
    loss2, flat2, _ = _run(f, b)
    assert loss2 == loss and torch.equal(flat2, flat)


def test_longest_unroll_and_the_refusal_beyond_it():
    from muax_amd import _lib
    info = _ensure(LONG_SHAPE)
    assert info["max_unroll"] >= LONG_L  # (the cap of 12 is what binds)
    m, b, l64, g64 = _case(LONG_SHAPE, B, LONG_L, LONG_SEED)
    loss, _, views = _run(_fused(m), b)
    _check(loss, views, l64, g64)
    f = _fused(m)
    f.grads.view(torch.int32).fill_(SENTINEL)
    f.loss.view(torch.int32).fill_(SENTINEL)
    too_long = info["max_unroll"] + 1
    with pytest.raises(_lib.TooLargeForLds, match=rf"unroll_steps {too_long} too large for the LDS \(at most {info['max_unroll']} "):
        f(ref.smz_batch(1, too_long, LONG_SHAPE[0], LONG_SHAPE[4], 0))
    torch.cuda.synchronize()
    assert (f.grads.view(torch.int32) == SENTINEL).all() and (f.loss.view(torch.int32) == SENTINEL).all()


@pytest.mark.parametrize("shape", [(16, 17, 15, 31, 33), (4, 48, 16, 20, 128)])
def test_guard_words_behind_every_output(shape):
    _ensure(shape)
    m, b, l64, g64 = _case(shape)
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


@pytest.mark.parametrize("shape", [(2, 62, 16, 8, 65), (5, 32, 17, 10, 16)])
def test_gradient_does_not_depend_on_the_split(shape):
    """B = 17 in one call against rows 0..8 and 9..16 in calls of their own at the same scale per row, summed, the L2
    term counted once."""
    _ensure(shape)
    m, b, l64, g64 = _case(shape)
    f = _fused(m)
    parts = []
    for rows, nb in ((slice(0, 9), 9), (slice(9, 17), 8)):
        sw = torch.full((nb,), nb / 17.0, device="cuda")
        parts.append(_run(f, ref.cut_rows(b, rows), sample_weight=sw))
    l2w = [1e-4 * p.detach().cpu().double().numpy() for p in f.params]
    l2 = 0.5 * sum(float((w * w).sum()) for w in l2w) / 1e-4
    views = [x.astype(np.float64) + y - w for x, y, w in zip(parts[0][2], parts[1][2], l2w)]
    _check(parts[0][0] + parts[1][0] - l2, views, l64, g64, note="split 9 + 8")


def test_observations_wider_than_a_registered_cap_are_still_refused():
    from muax_amd import _jit, _lib
    A, Cn, E, S, od = CAP32_SHAPE
    assert _jit.stochastic_train_plan(A, Cn, E, 2 * S + 1, od)[0] == 32
    _ensure(CAP32_SHAPE)
    m = ref.smz_model(*CAP32_SHAPE, seed=31)
    assert np.isfinite(_run(_fused(m), ref.smz_batch(4, 3, A, od, 0))[0])
    wide = ref.smz_model(A, Cn, E, S, 33, seed=31)
    f = _fused(wide)
    f.grads.view(torch.int32).fill_(SENTINEL)
    with pytest.raises(_lib.Unsupported, match=r"obs_dim must be 1\.\.32") as e:
        f(ref.smz_batch(4, 3, A, 33, 0))
    assert not isinstance(e.value, (_lib.NoKernelInstance, _lib.TooLargeForLds))
    torch.cuda.synchronize()
    assert (f.grads.view(torch.int32) == SENTINEL).all()


def test_model_update_builds_an_instance_on_demand():
    """Without the new flag an unlisted shape takes "torch" under "auto" and raises under "hip" (checked first: the
    registration below is process-wide).  With it "auto" and "hip" take the kernel, and one SGD step of learning rate 1
    matches the step of "torch" at the tolerances of test_gpu_stochastic_train.py::test_model_update_takes_the_fused_route."""
    from muax_amd import _lib
    A, Cn, E, support, od = MODEL_SHAPE
    b = ref.smz_batch(B, L, A, od, 0)
    sw = torch.from_numpy(np.random.default_rng(2).uniform(0.5, 2.0, B).astype(F32)).cuda()
    make = functools.partial(ref.smz_model, A, Cn, E, support, od, seed=41, optimizer=("sgd", 1.0), stochastic_fused_update=True)
    off = make()
    off.update(b)
    assert off._last_update_route == "torch"
    with pytest.raises(ValueError):  # (33 to 128 observations are not admitted without the flag)
        off.update(b, backend="hip")
    narrow = ref.smz_model(A, Cn, E, support, 20, seed=41, stochastic_fused_update=True)
    nb = ref.smz_batch(B, L, A, 20, 0)
    narrow.update(nb)
    assert narrow._last_update_route == "torch"
    with pytest.raises(_lib.NoKernelInstance):
        narrow.update(nb, backend="hip")
    steps = {}
    for backend in ("auto", "hip", "torch"):
        m = make(stochastic_train_on_demand=True)
        before = torch.cat([p.detach().reshape(-1).clone() for p in _fused(m).params])
        out = m.update(b, backend=backend, sample_weight=sw, vqvae_beta=0.5, divide_by_length=True)
        assert m._last_update_route == ("torch" if backend == "torch" else "hip_stochastic_fused")
        steps[backend] = (out["loss"], torch.cat([p.detach().reshape(-1) for p in _fused(m).params]) - before)
    assert torch.equal(steps["auto"][1], steps["hip"][1]) and steps["auto"][0] == steps["hip"][0]
    assert np.isclose(steps["hip"][0], steps["torch"][0], rtol=2e-4)
    assert steps["torch"][1].abs().max() > 1e-2
    assert torch.allclose(steps["hip"][1], steps["torch"][1], rtol=5e-3, atol=5e-4)
