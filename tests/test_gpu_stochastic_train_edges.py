"""GPU tests of the stochastic family's fused training step (muax_amd/csrc/mz_stoch_train.cuh through
mzs_stochastic_mlp_loss_grad and loss.StochasticFusedLossGrad) at the edges of its inputs, which the conditioning filter
of test_gpu_stochastic_train.py and test_gpu_stochastic_train_jit.py keeps those files away from on purpose: ties in
each of the three normalisers (also across 16-lane slots, also all E entries, also a range below 1e-5), a tie for the
encoder's argmax between two columns of different slots, logits of +-50 and +-300 on heads with a partial last slot,
targets on the codec's integers and at its clip, policy targets that are one-hot, partly or wholly zero or do not sum
to 1, actions and codes that never occur, zero sample weights, batches around one and four workgroups, and a batch of
4096 rows.

The inputs are stochastic_train_reference.STOCH_EDGE_CASES (each builder's docstring says what it is), shared with
tests/test_stochastic_train_reference_cpu.py, which shows on the CPU that the two float64 references used here agree on
every one of them to 1e-9, that the edge exists in fp32 and fp64 alike, that every OTHER condition of well_conditioned
holds for the whole batch (the seeds were picked on the CPU as the first from 0 for which it does: the filter drops
nothing, the kept share of (row, step) cases is 100 %), and that fp32 autograd on the CPU meets half of each bar below.

Bars (those of test_gpu_stochastic_train.py, through its `_check`; they do not move): loss within 1e-5 relative, each of
the 34 gradient arrays within 2e-4 of its largest reference entry (floor 1e-6), a second call bit-identical -- against
fp64 autograd of loss.stochastic_loss_fn AND against the independent NumPy reference
(oracle/mz_stoch_train_numpy.py), so that the result does not rest on product code.  Where the data contribute exact
zeros the gradient is fp32(1e-4 w) EXACTLY: the ad_w1 rows of actions absent from the batch, the cr_w1 / cn_w1 rows of
codes that never occur (the higher partner of the tied encoder pair among them), and the policy head's four arrays
when every policy target row is zero.

Measured on an MI355X, loss (relative) and worst gradient array against fp64 autograd, the kernel's and, beside it, the
torch fp32 route's on the GPU:
  case                         kernel: loss  grad                torch fp32: loss  grad
  ties_repr-E32                1.0e-08  3.8e-07 (repr_w)        1.0e-08  4.4e-07 (cn_w2)
  ties_repr-E8                 7.3e-09  3.0e-07 (en_w1)         6.9e-08  4.6e-07 (en_w1)
  ties_after-E32               7.7e-08  4.6e-07 (repr_w)        2.4e-08  4.8e-07 (pp_w1)
  ties_after-E8                4.8e-08  4.1e-07 (en_w2)         8.7e-08  3.1e-07 (en_w1)
  ties_next-E32                2.9e-08  3.7e-07 (repr_w)        2.9e-08  4.3e-07 (repr_w)
  ties_next-E8                 4.7e-08  4.1e-07 (repr_w)        9.0e-08  4.2e-07 (repr_w)
  all_tied-E32                 2.2e-08  2.6e-07 (en_w1)         4.3e-08  3.0e-07 (ad_w1)
  all_tied-E8                  1.5e-09  4.3e-07 (en_w1)         8.9e-08  4.0e-07 (en_w1)
  near_degenerate-2^-18        2.3e-08  4.5e-07 (repr_b)        2.3e-08  6.5e-07 (repr_b)
  near_degenerate-2^-16        7.1e-09  5.3e-07 (ad_w2)         8.7e-08  5.6e-07 (en_w1)
  encoder_tie_first-C32        6.3e-08  3.1e-07 (repr_w)        6.3e-08  3.2e-07 (en_w1)
  encoder_tie_first-C17        9.9e-09  3.5e-07 (repr_w)        9.9e-09  3.4e-07 (repr_w)
  large_logits-F63-50          3.1e-08  4.2e-07 (repr_w)        1.1e-07  3.7e-07 (pv_w2)
  large_logits-F63-300         2.7e-08  9.0e-07 (repr_w)        2.7e-08  6.8e-07 (repr_w)
  large_logits-C17-50          3.0e-08  2.9e-07 (en_w1)         3.0e-08  2.9e-07 (repr_w)
  large_logits-C17-300         1.2e-08  4.3e-07 (en_w1)         1.2e-08  1.4e-06 (repr_w)
  policy_targets               1.1e-07  2.8e-07 (en_w2)         1.1e-07  3.5e-07 (repr_b)
  policy_targets-all_zero      7.4e-08  3.5e-07 (repr_w)        9.3e-09  4.1e-07 (repr_w)
  support_edges-8              6.0e-08  3.2e-07 (en_w1)         2.1e-09  3.9e-07 (ad_w1)
  support_edges-31             7.0e-08  6.3e-07 (en_w2)         7.0e-08  7.9e-07 (en_w2)
  absent_actions-first         3.6e-08  4.2e-07 (en_w1)         2.8e-08  3.3e-07 (en_w1)
  absent_actions-last          6.9e-08  3.6e-07 (repr_w)        4.3e-08  3.0e-07 (repr_b)
  zero_weight_rows             5.5e-08  2.4e-07 (en_w1)         1.5e-07  2.8e-07 (ad_w2)
  batch_edges-15               1.4e-07  5.8e-07 (cn_b2)         1.4e-07  4.6e-07 (cn_b1)
  batch_edges-16               8.8e-09  3.0e-07 (en_w1)         5.3e-08  3.1e-07 (en_w1)
  batch_edges-17               3.9e-08  5.3e-07 (en_w2)         8.3e-08  9.6e-07 (repr_w)
  batch_edges-63               5.8e-08  3.9e-07 (repr_w)        5.7e-09  3.8e-07 (en_w1)
  batch_edges-65               3.2e-08  3.6e-07 (en_w1)         9.5e-08  4.2e-07 (en_w1)
  large_reduction              2.0e-09  2.9e-07 (cr_b1)         2.0e-09  1.9e-06 (repr_w)
  ties_repr-E17                4.7e-08  4.3e-07 (repr_w)        4.7e-08  3.8e-07 (repr_w)
  encoder_tie_first-E17        4.9e-08  4.7e-07 (en_w2)         6.3e-08  4.4e-07 (cn_w2)
The errors against the NumPy reference are the same to the digits shown (the two references agree to 1e-15).
"""
import numpy as np
import pytest
import torch

import stochastic_train_reference as ref
from test_gpu_stochastic_train import _check, _fused, _run

pytestmark = pytest.mark.gpu
F32 = np.float32


def _edge(case):
    from muax_amd._lib import STOCHASTIC_TRAIN_WEIGHT_NAMES as NAMES
    m, b, kw = case.m, case.b, case.kw
    kk = dict(kw, sample_weight=torch.from_numpy(kw["sample_weight"]).cuda()) if "sample_weight" in kw else kw
    f = _fused(m)
    loss, flat, views = _run(f, b, **kk)
    l64, g64 = ref.autograd(m, b, **kw)
    trace = {}
    lnp, gnp = ref.numpy_reference(m, b, trace=trace, **kw)
    case.verify(ref.captures(m, b))
    case.verify(trace)
    l32, g32 = ref.autograd(m, b, torch.float32, "cuda", **kw)
    et = ref.rel_errors(g32, g64)
    print(f"[torch fp32 loss {abs(l32 - l64) / abs(l64):.1e} grad {max(et):.1e} ({NAMES[int(np.argmax(et))]})]", end=" ")
    _check(loss, views, l64, g64, note="fp64:")
    _check(loss, views, lnp, gnp, note="NumPy:")
    loss2, flat2, _ = _run(f, b, **kk)  # fixed-order reduction: bit-reproducible
    assert loss2 == loss and torch.equal(flat2, flat)
    g = dict(zip(NAMES, views))
    w = ref.arrays(m)
    l2w = lambda n: (F32(1e-4) * w[n]).astype(F32)  # noqa: E731
    E = w["repr_b"].shape[0]
    if case.absent_actions is not None:
        rows = [E + a for a in case.absent_actions]
        assert np.array_equal(g["ad_w1"][rows], l2w("ad_w1")[rows])
        assert not np.array_equal(g["ad_w1"][:E], l2w("ad_w1")[:E])  # (the state rows do get data)
    if case.absent_codes is not None:
        rows = [E + c for c in case.absent_codes]
        taken = sorted(set(range(E, E + w["en_b2"].shape[0])) - set(rows))
        for n in ("cr_w1", "cn_w1"):
            assert np.array_equal(g[n][rows], l2w(n)[rows]), n
            assert taken and not np.array_equal(g[n][taken], l2w(n)[taken]), n  # (the code taken does get data)
    if case.pi_zero:
        for n in ("pp_w1", "pp_b1", "pp_w2", "pp_b2"):
            assert np.array_equal(g[n], l2w(n)), n
    if case.keep is not None:  # zero weights == the batch without those rows at the same scale per row
        nk, B = len(case.keep), len(kw["sample_weight"])
        lc, gc = ref.numpy_reference(m, ref.cut_rows(b, case.keep), sample_weight=np.full(nk, nk / B))
        _check(loss, views, lc, gc, note="without the rows:")
        _, _, vc = _run(f, ref.cut_rows(b, case.keep), sample_weight=torch.full((nk,), nk / B, device="cuda"))
        for n, x, y, d in zip(NAMES, views, vc, gc):
            assert np.abs(x.astype(np.float64) - y).max() <= 2e-4 * max(np.abs(d).max(), 1e-6), n


@pytest.mark.parametrize("name", list(ref.STOCH_EDGE_CASES))
def test_stochastic_edge_case(name):
    """One input of STOCH_EDGE_CASES on a listed instance:
      ties_repr / _after / _next  min tied two ways, max three ways, in the representation's, the afterstate's or the
                              next state's normaliser (every transition of L = 5); E = 32: the min's partners in
                              columns 3 and 19, the max's two in slot 0 and one in slot 1; E = 8: one slot
      all_tied                fresh net, zero first observations: every entry of s_0 is both min and max, c = 0
      near_degenerate         representation ranges of 2^-18 / 2^-16 at E = 32, graded biases over both slots
      encoder_tie_first       two encoder logits tie for the maximum at every row and step (C = 32: columns 3 and 19;
                              C = 17: 0 and 16, the last slot's one real lane): the code is the lower index, every
                              other code's cr_w1 / cn_w1 row is exact
      large_logits            av, ac, cr, pv, pp scaled to about +-50 / +-300, F = 63 with C = 32 and F = 17 with C = 17
      policy_targets          one-hot, partly zero, all-zero, sum 0.5 and sum 3 rows; every row zero: pp_* exact
      support_edges           support 8 and 31: targets on integers, one ulp beside them, at and far beyond the clip
      absent_actions          all actions 0, all A - 1: the other actions' ad_w1 rows exact
      zero_weight_rows        sample weights 0 on three rows and on a whole 16-row workgroup
      batch_edges             B = 15, 16, 17, 63, 65 at L = 3
      large_reduction         (4, 32, 32, 31, 16), B = 4096, L = 2."""
    _edge(ref.edge_case(name))


@pytest.mark.parametrize("name", list(ref.STOCH_JIT_EDGE_CASES))
def test_edge_case_on_an_on_demand_instance(name):
    """ties_repr and encoder_tie_first on (5, 32, 17, 10, 16), the instance test_gpu_stochastic_train_jit.py builds (the
    compile is shared through the jit cache): E = 17 puts a partner of the three-way maximum in the one real lane of
    slot 1."""
    from test_gpu_stochastic_train_jit import _ensure
    _ensure(ref.JIT_SHAPE)
    _edge(ref.edge_case(name))
