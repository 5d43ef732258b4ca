"""Plain-loop restatement of the device MountainCar (include/mzsearch.h, mzs_env_classic_* with MZS_ENV_MOUNTAINCAR;
DESIGN.md 4.7 "Device environments") in Python floats, one environment and one step at a time, written from the
equations of Gym's MountainCar-v0 and the draw rule.  math.cos and prng.threefry2x32; it shares nothing with
muax_amd/envs.py or the kernels.  Every expression is evaluated left to right as written; the kernel follows this file
operation by operation.

Generic in the number type as tests/acrobot_reference.py is (np.longdouble state, `cos=np.cos`), for the measurement of
D64 = max |fp64 - longdouble| over `uploaded_states()` in tests/test_env_classic_reference_cpu.py, which asserts
8 * D64 <= STEP_BAR.

STEP_BAR: D64 measured 1.1e-16 (x86-64 glibc, 80-bit long double): one cos of an argument below 3.6, scaled by 0.0025,
then two additions of quantities below 1.2 -- half an ulp of x.  8 * D64 = 8.7e-16, rounded up to one digit."""
import math

import numpy as np

from muax_amd import prng

MIN_X, MAX_X, MAX_V, GOAL_X, GOAL_V, FORCE, GRAVITY = -1.2, 0.6, 0.07, 0.5, 0.0, 0.001, 0.0025
OBS_DIM, NUM_ACTIONS, DRAWN = 2, 3, 1
STEP_BAR = 9e-16


def u53(key, x0, x1):
    """((y0 << 32 | y1) >> 11) * 2^-53 of threefry2x32(key, x0, x1): exact integer arithmetic, then one exact scaling."""
    y0, y1 = prng.threefry2x32(key, x0 & 0xFFFFFFFF, x1 & 0xFFFFFFFF)
    return float(((int(y0) << 32) | int(y1)) >> 11) * 2.0 ** -53


def draw(key, e, d):
    """The d-th start state of environment e: x drawn (one component, so the counter is d itself), v = 0."""
    return [-0.6 + 0.2 * u53(key, e, DRAWN * d + 0), 0.0]


def reset(draws, key, e):
    """-> (state, t, draws')"""
    return draw(key, e, draws), 0, draws + 1


def bound(x, lo, hi):
    return lo if x < lo else (hi if x > hi else x)


def raw_step(state, a, cos=math.cos):
    """(v before its clamp, x before its clamp, the stepped state)."""
    x, v = state
    a = 0 if a <= 0 else (2 if a >= 2 else a)
    v_raw = v + ((a - 1) * FORCE + cos(3.0 * x) * (-GRAVITY))
    v = bound(v_raw, -MAX_V, MAX_V)
    x_raw = x + v
    x = bound(x_raw, MIN_X, MAX_X)
    if x == MIN_X and v < 0.0:
        v = 0.0
    return v_raw, x_raw, [x, v]


def physics(state, a, cos=math.cos):
    """The stepped state; actions are clamped to 0..2."""
    return raw_step(state, a, cos)[2]


def terminated(new_state):
    return new_state[0] >= GOAL_X and new_state[1] >= GOAL_V


def margin(state, a):
    """How far the step from `state` stays from every branch a last bit could flip: v from its clamps, x from its
    clamps and from the goal, and -- only where x is at the goal, and v was not zeroed by the wall -- v from 0."""
    v_raw, x_raw, (x, v) = raw_step(state, a)
    m = min(abs(abs(v_raw) - MAX_V), abs(x_raw - MIN_X), abs(x_raw - MAX_X), abs(x - GOAL_X))
    if x >= GOAL_X - 1e-6:
        m = min(m, abs(v - GOAL_V))
    return m


def step(state, t, draws, a, key, e, max_steps):
    """-> (state', t', draws', r, done): a finished environment already holds its next start state, with t' = 0."""
    new = physics(state, a)
    t = t + 1
    done = terminated(new) or t >= max_steps
    if done:
        new, t, draws = draw(key, e, draws), 0, draws + 1
    return new, t, draws, -1.0, done


def obs(state):
    return list(state)


# ---- the states the GPU test uploads (tests/test_gpu_env_classic.py), shared so that D64 is measured on exactly them
N_RANDOM = 257
ACTIONS = (1, 0, -1, 2, 7)


def random_states(n=N_RANDOM, seed=1):
    """x over the whole track, v over its whole range; the action of state e is ACTIONS[e % 5]."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(MIN_X, MAX_X, n), rng.uniform(-MAX_V, MAX_V, n)], 1)


def _v_for_zero():
    """The v from which a step at x = 0.5 under action 0 ends with v = 0 exactly: minus the step's increment."""
    return -((0 - 1) * FORCE + math.cos(3.0 * 0.5) * (-GRAVITY))


def edge_rows():
    """(state, action, the stepped state, terminated, what the row is for).  The expected states are exact whatever the
    libm's last bits: a clamp or the wall decides every component (the margins are asserted on this reference by
    tests/test_env_classic_reference_cpu.py), and x + v is one exact-input addition.  The one row that leans on cos is
    "x = 0.5, v = 0": there the increment -0.001 - 0.0025 cos(1.5) must be the same double on the device, which it is
    for any cos(1.5) within 3 ulp of the host's (asserted there too: 0.0025 ulp(cos) is an eighth of the sum's ulp)."""
    return [([-1.19, -0.05], 0, [MIN_X, 0.0], False, "left wall: x clamped, v zeroed"),
            ([-1.0, 0.0695], 2, [-1.0 + MAX_V, MAX_V], False, "v clamped at +0.07"),
            ([0.0, -0.0695], 0, [0.0 - MAX_V, -MAX_V], False, "v clamped at -0.07"),
            ([0.58, 0.0699], 2, [MAX_X, MAX_V], True, "x clamped at 0.6 (done)"),
            ([0.5 - MAX_V, 0.0699], 2, [0.5, MAX_V], True, "x = 0.5 exactly, v > 0 (done)"),
            ([0.5, _v_for_zero()], 0, [0.5, 0.0], True, "x = 0.5 exactly, v = 0 (done)"),
            ([0.5 + MAX_V, -0.0699], 0, [0.5, -MAX_V], False, "x = 0.5 exactly, v < 0 (not done)")]


def uploaded_states():
    """[(state, action)] of every state the GPU test steps from an upload: the random ones, then the edge rows."""
    rs = random_states()
    return [(rs[e].tolist(), ACTIONS[e % 5]) for e in range(len(rs))] + [(r[0], r[1]) for r in edge_rows()]
