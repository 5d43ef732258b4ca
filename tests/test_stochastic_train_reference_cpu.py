"""The stochastic training step's independent float64 reference (oracle/mz_stoch_train_numpy.py: NumPy, hand-derived
backward, neither torch nor muax_amd inside) used to arbitrate the reference the GPU tests lean on
(stochastic_train_reference.autograd: muax_amd's own nn / utils / loss code under torch autograd in float64), on the
batches of tests/test_gpu_stochastic_train.py and on every edge input of tests/test_gpu_stochastic_train_edges.py
(stochastic_train_reference.STOCH_EDGE_CASES and STOCH_JIT_EDGE_CASES).  Needs no GPU.

For every edge input, three things:
  * fp64 autograd and the NumPy reference agree: loss to 1e-9 relative, every array to 1e-9 of its largest entry (the
    bar of tests/test_train_reference_cpu.py for the plain trio);
  * the case's verify() passes on the captures of the fp64 route, of the NumPy reference and of the fp32 route on the
    CPU: the tie or edge exists in both precisions, and the remaining conditions of well_conditioned hold for the
    WHOLE batch -- the seeds (EDGE_SEEDS) were picked on the CPU as the first from 0 for which they do, so nothing is
    filtered out: the kept share of (row, step) cases is 100 % everywhere;
  * fp32 autograd on the CPU stays within HALF of each GPU bar (loss 5e-6 relative, gradients 1e-4 of the array's
    largest fp64 entry): the input is not ill-conditioned for an fp32 route, which is what makes the GPU bars fair.

Measured fp32-CPU errors, loss (relative) and worst gradient array (of its largest fp64 entry) -- every one at least a
hundred times inside its half bar:
  ties_repr-E32                1.0e-08  5.2e-07 (repr_w)      large_logits-C17-300         7.3e-08  4.2e-07 (en_w1)
  ties_repr-E8                 6.8e-08  5.1e-07 (en_w2)       policy_targets               1.1e-07  2.3e-07 (en_w2)
  ties_after-E32               2.4e-08  4.4e-07 (repr_w)      policy_targets-all_zero      1.2e-07  3.4e-07 (repr_w)
  ties_after-E8                8.7e-08  3.6e-07 (repr_w)      support_edges-8              6.3e-08  3.7e-07 (en_w1)
  ties_next-E32                2.9e-08  3.9e-07 (repr_w)      support_edges-31             7.0e-08  7.5e-07 (en_w2)
  ties_next-E8                 9.0e-08  5.0e-07 (repr_w)      absent_actions-first         2.7e-08  4.8e-07 (ad_w1)
  all_tied-E32                 4.3e-08  3.1e-07 (en_w2)       absent_actions-last          4.3e-08  3.7e-07 (repr_w)
  all_tied-E8                  8.9e-08  3.2e-07 (en_w1)       zero_weight_rows             1.5e-07  3.2e-07 (repr_w)
  near_degenerate-2^-18        1.2e-07  3.7e-07 (en_w1)       batch_edges-15               1.6e-08  5.3e-07 (cn_w1)
  near_degenerate-2^-16        7.0e-09  4.7e-07 (en_w1)       batch_edges-16               5.2e-08  3.1e-07 (en_w1)
  encoder_tie_first-C32        2.7e-08  4.2e-07 (repr_w)      batch_edges-17               1.4e-07  4.7e-07 (repr_w)
  encoder_tie_first-C17        1.0e-08  2.8e-07 (en_w1)       batch_edges-63               6.9e-08  4.3e-07 (repr_w)
  large_logits-F63-50          3.2e-08  3.6e-07 (pv_w2)       batch_edges-65               1.6e-07  4.1e-07 (repr_w)
  large_logits-F63-300         2.6e-08  9.1e-07 (repr_w)      large_reduction (B = 4096)   1.9e-09  2.2e-07 (repr_w)
  large_logits-C17-50          3.0e-08  2.5e-07 (en_w1)       ties_repr-E17                1.6e-07  5.2e-07 (repr_w)
                                                              encoder_tie_first-E17        4.9e-08  4.3e-07 (en_w2)
large_reduction runs here at its full B = 4096: its fp64 autograd takes well under a second.
"""
import numpy as np
import pytest
import torch

import stochastic_train_reference as ref
from muax_amd._lib import STOCHASTIC_TRAIN_WEIGHT_NAMES as NAMES
from test_gpu_stochastic_train import BATCH_SEED, MODEL_SEED

HALF_LOSS_BAR, HALF_GRAD_BAR = 5e-6, 1e-4
EDGE_NAMES = list(ref.STOCH_EDGE_CASES) + list(ref.STOCH_JIT_EDGE_CASES)


def _arbitrate(m, b, **kw):
    l_t, g_t = ref.autograd(m, b, **kw)
    l_n, g_n = ref.numpy_reference(m, b, **kw)
    errs = ref.rel_errors(g_t, g_n)
    print(f"[autograd fp64 against NumPy: loss {abs(l_t - l_n) / abs(l_n):.1e} grad {max(errs):.1e}]", end=" ")
    assert abs(l_t - l_n) <= 1e-9 * abs(l_n), (l_t, l_n)
    for n, x, y, e in zip(NAMES, g_t, g_n, errs):
        assert x.shape == y.shape and e <= 1e-9, (n, e)
    return l_t, g_t


def test_numpy_reference_names_the_34_arrays_in_order():
    from oracle import mz_stoch_train_numpy as oracle
    assert list(oracle.WEIGHT_NAMES) == list(NAMES) and len(NAMES) == 34


@pytest.mark.parametrize("kw", [{}, dict(vqvae_beta=0.7), dict(divide_by_length=True),
                                dict(sample_weight=True, vqvae_beta=1.5, divide_by_length=True)],
                         ids=["default", "beta", "divide", "all"])
@pytest.mark.parametrize("si,B,L", [(0, 17, 5), (1, 17, 5), (2, 17, 5), (1, 1, 1), (2, 16, 2)])
def test_autograd_reference_agrees_with_numpy_on_the_existing_batches(si, B, L, kw):
    """The batches of tests/test_gpu_stochastic_train.py (its model and batch seeds), with the loss's three options."""
    A, _, _, _, od = ref.SHAPES[si]
    m = ref.smz_model(*ref.SHAPES[si], seed=MODEL_SEED + si, device="cpu")
    b = ref.smz_batch(B, L, A, od, BATCH_SEED[si, B, L])
    if kw.get("sample_weight"):
        kw = dict(kw, sample_weight=np.random.default_rng(1).uniform(0.2, 3.0, B).astype(np.float32))
    _arbitrate(m, b, **kw)


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_edge_input_on_the_cpu(name):
    case = ref.edge_case(name, "cpu")
    m, b, kw = case.m, case.b, case.kw
    trace = {}
    ref.numpy_reference(m, b, trace=trace, **kw)
    for cap in (ref.captures(m, b), trace, ref.captures(m, b, torch.float32)):
        case.verify(cap)
    l64, g64 = _arbitrate(m, b, **kw)
    l32, g32 = ref.autograd(m, b, torch.float32, "cpu", **kw)
    el, eg = abs(l32 - l64) / abs(l64), ref.rel_errors(g32, g64)
    print(f"[fp32 on the CPU: loss {el:.1e} grad {max(eg):.1e} ({NAMES[int(np.argmax(eg))]})]", end=" ")
    assert el <= HALF_LOSS_BAR, (l32, l64)
    for n, e in zip(NAMES, eg):
        assert e <= HALF_GRAD_BAR, (n, e)
    if case.absent_codes is not None:  # the reference's code is the lower index of the tied pair, everywhere
        codes = set(np.unique(trace["codes"]).tolist())
        assert codes and not codes & set(case.absent_codes)
    if case.keep is not None:  # zero weights == the batch without those rows at the same scale per row
        nk, B = len(case.keep), len(kw["sample_weight"])
        lc, gc = ref.numpy_reference(m, ref.cut_rows(b, case.keep), sample_weight=np.full(nk, nk / B))
        assert 0 < nk < B and abs(lc - l64) <= 1e-9 * abs(l64)
        assert max(ref.rel_errors(gc, g64)) <= 1e-9
