"""GPU tests of the fused training step (mzs_mlp_loss_grad, muax_amd/csrc/mz_train.cuh) at the edges of its inputs on
MULTI-SLOT shapes: embeddings of 40 and 64 (three and four 16-lane slots), 17 to 64 actions, support heads of 17, 33
and 49 bins -- where minmax_fwd / minmax_bwd combine per-slot partial minima, maxima and tie counts, softmax_lse and
ce_and_grad mask the pad lanes of a partial last slot, make_x places the action one-hot across a slot boundary, and
store_bias / store_tiles write slots t > 0.  tests/test_gpu_train_edges.py has the same edges at one-slot shapes.

The inputs are helpers.WIDE_EDGE_CASES, shared with tests/test_train_reference_cpu.py, which shows on the CPU that the
two float64 references used here agree on every one of them to 1e-9.

Bars (those of test_gpu_train.py; they do not move): loss within 1e-5 relative, each of the 18 gradient arrays within
2e-4 of its largest reference entry, a second call bit-identical -- against fp64 autograd of muax_amd/loss.py
(helpers.train_autograd) AND against the independent NumPy reference (oracle/mz_train_numpy.py), so that the result
does not rest on product code.  Where the data contribute exact zeros the gradient is fp32(1e-4 w) EXACTLY: the
dr_w1 / dn_w1 rows of every action absent from the batch, and the policy head's four arrays when every policy target
row is zero.  helpers.check_train_step prints the kernel's and the torch fp32 route's errors."""
import numpy as np
import pytest

from helpers import WIDE_EDGE_CASES, check_train_step, trio_arrays

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.mark.parametrize("name", list(WIDE_EDGE_CASES))
def test_wide_edge_case(name):
    """One input of helpers.WIDE_EDGE_CASES (its builder's docstring says what it is):
      ties_dn / ties_repr     min tied between columns 3 and 35, max three ways over three slots (E = 40: one partner
                              in the partial last slot, column 39), asserted on the captured normaliser inputs of
                              every step in fp64 and fp32; once with pp_b2 - 300 on top
      all_tied                fresh net, zero first observations: all 64 entries are both min and max
      near_degenerate         ranges of 2^-18 / 2^-16 at E = 40, graded biases over all three slots
      policy_shift / _equal   A = 17, 33, 49 (one real lane in the last slot): pp_b2 -+ 300 -- a pad lane's raw value
                              is 0 while every real logit is near -300 -- and all logits exactly equal
      large_logits            all three heads scaled to about +-300, at (33, 8) and (64, 64)
      support_clip            F = 17, 33, 49: two-hot mass on bin 0 and on bin F - 1, the last slot's one real lane
      onehot                  actions all 0, all A - 1, all from one slot, at (E, A) = (15, 17), (16, 17), (63, 64);
                              absent actions' dr_w1 / dn_w1 rows exact; all-zero pi: the policy head's arrays exact
      large_reduction         (64, 64, support 31), B = 16384, L = 2."""
    case = WIDE_EDGE_CASES[name](None)
    g = check_train_step(case.m, case.b, verify=case.verify)
    w = trio_arrays(case.m)
    l2 = F32(1e-4)
    if case.absent is not None:
        E = w["repr_b"].shape[0]
        rows = [E + a for a in case.absent]
        for n in ("dr_w1", "dn_w1"):
            assert np.array_equal(g[n][rows], l2 * w[n][rows]), n
            assert not np.array_equal(g[n][:E], l2 * w[n][:E]), n  # (the state rows do get data)
    if case.pi_zero:
        for n in ("pp_w1", "pp_b1", "pp_w2", "pp_b2"):
            assert np.array_equal(g[n], l2 * w[n]), n
