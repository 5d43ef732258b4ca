"""GPU test of the fused training step (mzs_mlp_loss_grad, muax_amd/csrc/mz_train.cuh) over a covering set of
on-demand instances, narrow (muax_amd/_jit.py::ensure_train_instance) and wide (ensure_wide_train_instance), and of the
support sizes it refuses.  helpers.TRAIN_LATTICE: twelve shapes in which every

    E in {1, 15, 17, 33, 63}          (one lane, one short of a slot, one real lane in the last slot, one short of 64)
    F = 2 support + 1 in {17, 33, 49, 63}                 (the same one-lane situation in the support heads)
    A in {1, 15, 16, 17, 49, 64}
    X = E + A in {16, 17, 32, 33, 64, 65, 128}            (the dynamics' input on and one past a slot edge)
    obs_dim in {1, 17, 128}

appears at least once (tests/test_train_reference_cpu.py asserts that without a GPU; the host model takes A = 1: it is in the set).  Bars: those of test_gpu_wide_train_edges.py,
against fp64 autograd and against the NumPy reference.  Every shape compiles one translation unit on first use."""
import numpy as np
import pytest

import muax_amd as mx
from helpers import TRAIN_LATTICE, check_train_step, lattice_case, train_batch, train_model

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("A,E,support,obs_dim", TRAIN_LATTICE)
def test_shape_lattice_matches_both_references(A, E, support, obs_dim):
    """One on-demand instance per case, with the loss summed over the steps and divided by their number."""
    m, b = lattice_case(A, E, support, obs_dim)
    check_train_step(m, b)
    check_train_step(m, b, divide_by_length=True)


@pytest.mark.parametrize("support", [7, 32])
def test_support_sizes_outside_8_to_31_are_refused_with_the_limit_named(support):
    """F = 15 and F = 65: refused on the host, before any launch, with the limit in the message; update() raises under
    backend="hip" and takes the torch route under backend="auto"."""
    m, b = train_model(2, 8, 4, seed=support, support=support), train_batch(20, 2, 2, 4, seed=support)
    with pytest.raises(ValueError, match=r"no kernel instance .*support_size must be 8\.\.31"):
        mx.loss.FusedLossGrad(m)(b)
    with pytest.raises(ValueError, match=r"support_size must be 8\.\.31"):
        train_model(2, 8, 4, seed=support, support=support).update(b, backend="hip")
    mt = train_model(2, 8, 4, seed=support, support=support)
    la, lt = m.update(b)["loss"], mt.update(b, backend="torch")["loss"]
    assert np.isclose(la, lt, rtol=1e-6)
