"""CPU tests of tests/nstep_reference.py, the plain-loop float64 reference test_gpu_replay_kernels.py compares the
replay kernels with.

Against the package's array code (`vector.nstep_returns`, `vector.episode_trajectory`) and the older NumPy restatement
(`reanalyse_reference.targets`), which state the same operations in the same order, nothing may differ: Rn, done, and
with them the operand |v - Rn| of the priority weight, are compared bit for bit over the whole grid; so are w and cw
wherever the power is exact (no alpha, alpha = 1).  With a fractional alpha w is NOT bit-comparable between the two
sides, and that is no matter of operation order: `x ** alpha` on a Python float is the C library's pow, on a NumPy array
it is NumPy's own loop (sqrt for 0.5, a vectorised pow otherwise), and the two round differently on the same operand
(measured on 2e6 uniform operands in (0, 100): 1 697 differ in the last bit at alpha 0.5, 111 362 at 0.6, none at 1).
There w is held to 1e-12 relative -- the project's bar for two pow implementations (test_gpu_replay.py) --
and to exactly 0 where either is 0, and cw to the bit-exact sequential sum of the reference's own w, which must also
be what np.cumsum makes of it.  Against the step-by-step tracers `NStep` / `PNStep`, which take the reward sum with
`np.sum` (another order), Rn may differ by the rounding of a sum of at most n + 1 addends: each of its at most n
additions rounds a partial sum no larger than S = sum |addend| by at most 2^-53 S, in either order, so
|Rn_loop - Rn_tracer| <= (n + 1) 2^-53 S covers both with room for the bootstrap's addition."""
import functools

import numpy as np
import pytest

import nstep_reference as loop
import reanalyse_reference as rref
from muax_amd import vector
from muax_amd.episode_tracer import NStep, PNStep

LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 200)
N_STEPS = (1, 5, 64, 300)
ALPHAS = (None, 0.5, 0.6, 1.0)


@functools.lru_cache(maxsize=None)
def _episodes(kind):
    """[(r [T] f64, v [T] f64)] over LENGTHS and the discount: general values, or dyadic ones (every return exact)."""
    rng = np.random.default_rng(31 if kind == "random" else 32)
    out = []
    for T in LENGTHS:
        if kind == "dyadic":
            out.append((rng.integers(-16, 17, T) / 8.0, rng.integers(-64, 65, T) / 8.0))
        else:
            out.append((rng.uniform(-2, 3, T), rng.uniform(-30, 60, T)))
    return out, (0.5 if kind == "dyadic" else 0.997)


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def _assert_w(w, cw, a_w, alpha, where):
    """The loop reference's w, cw against an array-computed w of the same operands (see the module's docstring)."""
    w, a_w = np.asarray(w), np.asarray(a_w, np.float64).reshape(-1)
    if alpha is None or alpha == 1.0:
        assert np.array_equal(_bits(w), _bits(a_w)), where
        assert np.array_equal(_bits(cw), _bits(np.cumsum(a_w))), where
    else:
        zero = (w == 0) | (a_w == 0)
        assert np.array_equal(_bits(w[zero]), _bits(a_w[zero])), where
        err = np.abs(w[~zero] - a_w[~zero]) / a_w[~zero]
        assert (err <= 1e-12).all(), (where, err.max())
    assert np.array_equal(_bits(cw), _bits(np.cumsum(w))), where
    carry, seq = 0.0, []
    for x in w.tolist():
        carry += x
        seq.append(carry)
    assert np.array_equal(_bits(cw), _bits(seq)), where


@pytest.mark.parametrize("kind", ["random", "dyadic"])
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("n", N_STEPS)
def test_loop_reference_equals_the_array_code_bit_for_bit(n, alpha, kind):
    eps, gamma = _episodes(kind)
    for r, v in eps:
        T = len(r)
        Rn, done, w, cw, weight = loop.episode(r, v, n, gamma, alpha, "mean")
        a_Rn, a_done = vector.nstep_returns(r, v, n, gamma)
        assert np.array_equal(_bits(Rn), _bits(a_Rn)), (T, n)
        assert np.array_equal(np.array(done), a_done), (T, n)
        tr = vector.episode_trajectory(np.zeros((T, 1)), np.zeros(T, int), r, v, np.ones((T, 1)), n, gamma, alpha)
        assert np.array_equal(_bits([abs(float(v[t]) - Rn[t]) for t in range(T)]), _bits(np.abs(v - a_Rn))), (T, n)
        _assert_w(w, cw, tr._rows[7], alpha, (T, n, alpha))
        # the float32 inputs of reanalysis: stored rewards and searched values, widened
        r32, v32 = r.astype(np.float32), v.astype(np.float32)
        for mode in ("mean", "sum"):
            Rn, done, w, cw, weight = loop.episode(r32, v32, n, gamma, alpha, mode)
            t_Rn, t_done, t_w, t_cw, t_weight = rref.targets(r32, np.ones((T, 1), np.float32), v32, n, gamma, alpha, mode)
            assert np.array_equal(np.array(Rn).astype(np.float32).view(np.uint32), t_Rn.view(np.uint32)), (T, n)
            assert np.array_equal(np.array(done), t_done), (T, n)
            _assert_w(w, cw, t_w, alpha, (T, n, alpha, mode))
            assert np.array_equal(_bits(t_cw), _bits(np.cumsum(t_w)))
            assert weight == (cw[-1] if mode == "sum" else cw[-1] / T)
            if alpha is None or alpha == 1.0:  # (np.mean and np.sum add pairwise: another order, so to rounding only)
                assert abs(weight - t_weight) <= T * 2.0 ** -53 * abs(t_weight)


def _traced(tracer, r, v):
    out = []
    for t in range(len(r)):
        tracer.add(0, 0, float(r[t]), t == len(r) - 1, v=float(v[t]))
        while tracer:
            out.append(tracer.pop())
    return out


@pytest.mark.parametrize("kind", ["random", "dyadic"])
@pytest.mark.parametrize("n", N_STEPS)
def test_loop_reference_within_the_rounding_of_the_tracers_sum(n, kind):
    eps, gamma = _episodes(kind)
    worst = 0.0
    for r, v in eps:
        T = len(r)
        Rn, done, w, _, _ = loop.episode(r, v, n, gamma, 0.5)
        for tracer, with_w in ((NStep(n, gamma), False), (PNStep(n, gamma, 0.5), True)):
            got = _traced(tracer, r, v)
            assert len(got) == T
            for t, tr in enumerate(got):
                S = sum(abs(x) for x in loop.terms(r, v, t, n, gamma))
                bound = (n + 1) * 2.0 ** -53 * S
                err = abs(float(tr.Rn) - Rn[t])
                worst = max(worst, err / bound if bound else (0.0 if err == 0 else np.inf))
                assert err <= bound, (T, t, err, bound)
                assert bool(tr.done) == done[t], (T, t)
                if kind == "dyadic" and n <= 5:  # multiples of 2^-8 below 2^4: every partial sum exact in any order
                    assert float(tr.Rn) == Rn[t]
                    if with_w:
                        assert float(tr.w) == w[t]
    print(f"[n {n} {kind}: largest |Rn_loop - Rn_tracer| / bound = {worst:.3f}]", end=" ")


def test_transition_by_hand():
    """Three steps, n = 2, gamma = 0.5: the numbers worked out on paper."""
    r, v = [1.0, 2.0, 4.0], [8.0, 16.0, 32.0]
    assert loop.transition(r, v, 0, 2, 0.5) == (1.0 + 0.5 * 2.0 + 0.25 * 32.0, False, 1.0)
    assert loop.transition(r, v, 1, 2, 0.5, 1.0) == (2.0 + 0.5 * 4.0, True, 12.0)
    assert loop.transition(r, v, 2, 2, 0.5, 0.5) == (4.0, True, 28.0 ** 0.5)
    Rn, done, w, cw, weight = loop.episode(r, v, 2, 0.5, 1.0, "sum")
    assert (Rn, done, w, cw, weight) == ([10.0, 4.0, 4.0], [False, True, True], [2.0, 12.0, 28.0], [2.0, 14.0, 42.0], 42.0)
    assert loop.episode(r, v, 2, 0.5, 1.0, "mean")[4] == 14.0
    assert loop.terms(r, v, 0, 2, 0.5) == [1.0, 1.0, 8.0] and loop.terms(r, v, 2, 2, 0.5) == [4.0]
