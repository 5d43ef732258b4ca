"""The training step's independent float64 reference (oracle/mz_train_numpy.py: NumPy, hand-derived backward, neither
torch nor muax_amd inside) -- checked against itself by finite differences, then used to arbitrate the reference the
GPU tests lean on (helpers.train_autograd: muax_amd's own nn / utils / loss code under torch autograd in float64).
Needs no GPU."""
import numpy as np
import pytest
import torch

from helpers import TRAIN_LATTICE, WIDE_EDGE_CASES, lattice_case, train_autograd, train_batch, train_model, train_numpy, trio_arrays
from muax_amd._lib import MLP_WEIGHT_NAMES
from oracle import mz_train_numpy as ref

EPS = np.finfo(np.float64).eps
FD_WORST_MEASURED = 2.6e-7  # the worst finite-difference disagreement over every case below (see the docstring)
FD_BAR = 10 * FD_WORST_MEASURED
GRAD_FLOOR = 1e-2           # an array whose gradient is smaller all over is measured against this instead


def _args(m, b):
    return (trio_arrays(m), b.obs[:, 0], b.a, b.r, b.Rn, b.pi, m._support_size)


def _smooth(trace):
    """No kink of the loss within reach of a finite-difference step: every normaliser input has one minimum and one
    maximum, clear of the runner-up by 1e-4, and a range clear of the 1e-5 branch; no h(x) within 1e-3 of an integer
    (nor beyond the clip); no ELU input within 1e-3 of 0."""
    for u in trace["normalizer_inputs"]:
        if u.shape[1] < 2:
            return False
        srt = np.sort(u, 1)
        if (srt[:, 1] - srt[:, 0]).min() < 1e-4 or (srt[:, -1] - srt[:, -2]).min() < 1e-4:
            return False
        if np.abs((srt[:, -1] - srt[:, 0]) - 1e-5).min() < 1e-4:
            return False
    h = trace["scaled_targets"]
    if np.abs(h - np.round(h)).min() < 1e-3:
        return False
    return all(np.abs(x).min() >= 1e-3 for x in trace["elu_inputs"])


def _smooth_case(A, E, support, L):
    """The first seeded (model, batch) of the shape that is a smooth point; B = 3 keeps the ELU inputs few enough for
    one to exist among a few seeds.  The conditions are about the inputs alone, not about any gradient."""
    for seed in range(60):
        m = train_model(A, E, 5, seed=seed, support=support, device="cpu")
        b = train_batch(3, L, A, 5, seed=seed)
        trace = {}
        ref.forward(*_args(m, b), trace=trace)
        if np.abs(trace["scaled_targets"]).max() < support and _smooth(trace):
            return m, b, trace
    raise AssertionError("no smooth point among 60 seeds")


@pytest.mark.parametrize("divide_by_length", [False, True])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("A,E,support", [(2, 8, 10), (18, 8, 10), (33, 40, 31)])
def test_analytic_gradient_matches_central_differences(A, E, support, L, divide_by_length):
    """The hand-derived backward of oracle/mz_train_numpy.py against central differences of the same file's forward,
    at smooth points (asserted first).  Every entry at (2, 8, F 21); a seeded sample of 200 entries per array (all of
    an array that has no more) otherwise.  Step: the cube-root-of-epsilon rule, h = eps^(1/3) max(|x|, 0.1) for an
    entry x (0.1: the size of a typical weight, so that an entry near zero does not get a step lost in rounding).
    Error: |fd - g| over the array's largest |g|, as every other bar of the training tests -- or over GRAD_FLOOR = 1e-2
    where the whole array is smaller (dn_* at L = 1 carry the L2 term alone, about 1e-5: the difference quotient's own
    rounding, eps loss / h, about 3e-9 absolute, would be all that is measured there).  The two sides differentiate
    the same function only when the stop_gradient half of scale_gradient(s, 0.5) is held at the base point: see
    forward()'s frozen_states.

    Measured over the twelve cases: worst 2.6e-7 at (33, 40, F 63), L = 3 (FD_WORST_MEASURED), 1.9e-8 to 1.0e-7 at
    the two smaller shapes; it is the quotient's rounding on the arrays with the smallest gradients, not truncation
    (h^2 f''' / 6 with h about 6e-7 is below 1e-11).  The bar is ten times the measured worst, since the error varies
    by about that much from entry to entry, and stays below 1e-5."""
    assert FD_BAR < 1e-5
    m, b, trace = _smooth_case(A, E, support, L)
    assert _smooth(trace)
    args = _args(m, b)
    w = {n: v.astype(np.float64) for n, v in args[0].items()}
    loss, g = ref.loss_and_grads(*args, divide_by_length=divide_by_length)
    kw = dict(divide_by_length=divide_by_length, frozen_states=trace["states"])  # (see forward() on frozen_states)
    assert abs(loss - ref.forward(*args, **kw)) <= 4 * EPS * loss
    rng = np.random.default_rng(A + E + L)
    worst = 0.0
    for n in MLP_WEIGHT_NAMES:
        size = w[n].size
        idx = np.arange(size) if (A, E) == (2, 8) or size <= 200 else rng.choice(size, 200, replace=False)
        gmax = max(np.abs(g[n]).max(), GRAD_FLOOR)
        for k in idx:
            x = w[n].flat[k]
            h = EPS ** (1 / 3) * max(abs(x), 0.1)
            hi, lo = x + h, x - h
            w[n].flat[k] = hi
            fp = ref.forward(w, *args[1:], **kw)
            w[n].flat[k] = lo
            fm = ref.forward(w, *args[1:], **kw)
            w[n].flat[k] = x
            err = abs((fp - fm) / (hi - lo) - g[n].flat[k]) / gmax
            worst = max(worst, err)
            assert err <= FD_BAR, (n, int(k), err)
    print(f"[finite differences: worst {worst:.1e} of the array's largest entry]", end=" ")


def _arbitrate(m, b, **kw):
    l_t, g_t = train_autograd(m, b, torch.float64, "cpu", **kw)
    l_n, g_n = train_numpy(m, b, **kw)
    errs = [float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-6)) for x, y in zip(g_t, g_n)]
    print(f"[autograd fp64 against NumPy: loss {abs(l_t - l_n) / abs(l_n):.1e} grad {max(errs):.1e}]", end=" ")
    assert abs(l_t - l_n) <= 1e-12 * abs(l_n), (l_t, l_n)
    for n, x, y, e in zip(MLP_WEIGHT_NAMES, g_t, g_n, errs):
        assert x.shape == y.shape and e <= 1e-9, (n, e)


def test_lattice_covers_every_listed_value():
    """helpers.TRAIN_LATTICE, the shapes of tests/test_gpu_train_lattice.py, is a covering set of at most 14."""
    cover = lambda f: {f(*s) for s in TRAIN_LATTICE}  # noqa: E731
    assert len(TRAIN_LATTICE) <= 14
    assert cover(lambda A, E, S, od: E) >= {1, 15, 17, 33, 63}
    assert cover(lambda A, E, S, od: 2 * S + 1) >= {17, 33, 49, 63}
    assert cover(lambda A, E, S, od: A) >= {1, 15, 16, 17, 49, 64}
    assert cover(lambda A, E, S, od: E + A) >= {16, 17, 32, 33, 64, 65, 128}
    assert cover(lambda A, E, S, od: od) >= {1, 17, 128}


@pytest.mark.parametrize("divide_by_length", [False, True])
@pytest.mark.parametrize("A,E,support,obs_dim", TRAIN_LATTICE)
def test_autograd_reference_agrees_with_numpy_on_the_lattice(A, E, support, obs_dim, divide_by_length):
    """Both are float64 evaluations of about 1e4 operations per entry: 1e-9 of the array's largest entry on every
    gradient, 1e-12 relative on the loss.  A disagreement is a finding about muax_amd's nn / utils / loss."""
    m, b = lattice_case(A, E, support, obs_dim, device="cpu")
    _arbitrate(m, b, divide_by_length=divide_by_length)


@pytest.mark.parametrize("name", list(WIDE_EDGE_CASES))
def test_autograd_reference_agrees_with_numpy_on_the_edge_inputs(name):
    """The edge inputs of tests/test_gpu_wide_train_edges.py: ties across slots (asserted on the normaliser inputs of
    BOTH references), degenerate ranges, logits of +-300, targets at the clip, absent actions, all-zero policy rows."""
    case = WIDE_EDGE_CASES[name]("cpu")
    if case.verify is not None:
        cap, trace = [], {}
        train_autograd(case.m, case.b, torch.float64, "cpu", capture=cap)
        train_numpy(case.m, case.b, trace=trace)
        case.verify([c.numpy() for c in cap])
        case.verify(trace["normalizer_inputs"])
        cap32 = []
        train_autograd(case.m, case.b, torch.float32, "cpu", capture=cap32)
        case.verify([c.numpy() for c in cap32])
    _arbitrate(case.m, case.b)
