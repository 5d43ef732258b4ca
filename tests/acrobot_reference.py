"""Plain-loop restatement of the device Acrobot (include/mzsearch.h, mzs_env_classic_* with MZS_ENV_ACROBOT; DESIGN.md
4.7 "Device environments") in Python floats, one environment and one step at a time, written from the equations (Sutton
& Barto's "book" form, as Gym's Acrobot-v1 states them) and the draw rule.  math.sin / math.cos and prng.threefry2x32; it
shares nothing with muax_amd/envs.py or the kernels.  Every expression is evaluated left to right as written; the kernel
follows this file operation by operation.

The arithmetic is generic in the number type: with np.longdouble state components and `cos=np.cos, sin=np.sin` every
operation that involves the state runs in extended precision, while the sub-expressions of constants alone stay the
fp64 values they are in the fp64 run (the same real constants).  tests/test_env_classic_reference_cpu.py measures D64 =
max |fp64 - longdouble| over `uploaded_states()` that way and asserts 8 * D64 <= STEP_BAR.

STEP_BAR: D64 measured 1.2e-12 (x86-64 glibc, 80-bit long double).  The largest differences are raw velocities of order
100 before their clamp, where one ulp is 1.4e-14, after four derivative evaluations each of which divides by
m2 lc2^2 + I2 - d2^2 / d1 and multiplies the early roundings by velocities squared.  8 * D64 = 8.95e-12, rounded up to
one digit."""
import math

import numpy as np

from muax_amd import prng

M1, M2, L1, LC1, LC2, I1, I2, G = 1.0, 1.0, 1.0, 0.5, 0.5, 1.0, 1.0, 9.8
DT, PI = 0.2, math.pi
MAX_VEL_1, MAX_VEL_2 = 4 * PI, 9 * PI
WRAP_MAX = 64  # -+2 pi at most this often each way (the ABI's bound; never reached from a wrapped state)
OBS_DIM, NUM_ACTIONS, DRAWN = 6, 3, 4
STEP_BAR = 9e-12


def u53(key, x0, x1):
    """((y0 << 32 | y1) >> 11) * 2^-53 of threefry2x32(key, x0, x1): exact integer arithmetic, then one exact scaling."""
    y0, y1 = prng.threefry2x32(key, x0 & 0xFFFFFFFF, x1 & 0xFFFFFFFF)
    return float(((int(y0) << 32) | int(y1)) >> 11) * 2.0 ** -53


def draw(key, e, d):
    """The d-th start state of environment e: all four components drawn."""
    return [-0.1 + 0.2 * u53(key, e, DRAWN * d + c) for c in range(DRAWN)]


def reset(draws, key, e):
    """-> (state, t, draws')"""
    return draw(key, e, draws), 0, draws + 1


def torque(a):
    return -1.0 if a <= 0 else (1.0 if a >= 2 else 0.0)


def dsdt(s, a, cos=math.cos, sin=math.sin):
    """d/dt of (th1, th2, dth1, dth2) under torque a."""
    th1, th2, dth1, dth2 = s
    c2, s2 = cos(th2), sin(th2)
    d1 = M1 * LC1 * LC1 + M2 * (L1 * L1 + LC2 * LC2 + 2.0 * L1 * LC2 * c2) + I1 + I2
    d2 = M2 * (LC2 * LC2 + L1 * LC2 * c2) + I2
    phi2 = M2 * LC2 * G * cos(th1 + th2 - PI / 2.0)
    phi1 = -M2 * L1 * LC2 * dth2 * dth2 * s2 - 2.0 * M2 * L1 * LC2 * dth2 * dth1 * s2 \
        + (M1 * LC1 + M2 * L1) * G * cos(th1 - PI / 2.0) + phi2
    ddth2 = (a + d2 / d1 * phi1 - M2 * L1 * LC2 * dth1 * dth1 * s2 - phi2) / (M2 * LC2 * LC2 + I2 - d2 * d2 / d1)
    ddth1 = -(d2 * ddth2 + phi1) / d1
    return [dth1, dth2, ddth1, ddth2]


def rk4(s, a, dt=DT, cos=math.cos, sin=math.sin):
    """One classical Runge-Kutta step of (state, torque a): the raw new state, before wrap and clamp."""
    dt2, dt6 = dt / 2.0, dt / 6.0
    k1 = dsdt(s, a, cos, sin)
    k2 = dsdt([s[i] + dt2 * k1[i] for i in range(4)], a, cos, sin)
    k3 = dsdt([s[i] + dt2 * k2[i] for i in range(4)], a, cos, sin)
    k4 = dsdt([s[i] + dt * k3[i] for i in range(4)], a, cos, sin)
    return [s[i] + dt6 * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]) for i in range(4)]


def wrap(x):
    """Into [-pi, pi] by repeated -+2 pi."""
    two_pi = PI - (-PI)
    for _ in range(WRAP_MAX):
        if not x > PI:
            break
        x = x - two_pi
    for _ in range(WRAP_MAX):
        if not x < -PI:
            break
        x = x + two_pi
    return x


def bound(x, lo, hi):
    return lo if x < lo else (hi if x > hi else x)


def finish(raw):
    return [wrap(raw[0]), wrap(raw[1]), bound(raw[2], -MAX_VEL_1, MAX_VEL_1), bound(raw[3], -MAX_VEL_2, MAX_VEL_2)]


def physics(state, a, cos=math.cos, sin=math.sin):
    """The stepped state: RK4, angles wrapped, velocities clamped.  `a` is the ACTION (0, 1, 2; others clamped)."""
    return finish(rk4(state, torque(a), DT, cos, sin))


def height(new_state, cos=math.cos):
    """terminated = height > 1"""
    return -cos(new_state[0]) - cos(new_state[0] + new_state[1])


def margin(state, a):
    """How far the step from `state` stays from every branch a last bit could flip: the raw angles from the odd
    multiples of pi (the wrap's comparisons), the raw velocities from their clamps, the new state's height from 1."""
    raw = rk4(state, torque(a))

    def odd_pi(x):  # distance from the nearest odd multiple of pi
        k = 2 * math.floor(x / (2 * PI)) + 1
        return min(abs(x - k * PI), abs(x - (k - 2) * PI), abs(x - (k + 2) * PI))
    return min(odd_pi(raw[0]), odd_pi(raw[1]), abs(abs(raw[2]) - MAX_VEL_1), abs(abs(raw[3]) - MAX_VEL_2),
               abs(height(finish(raw)) - 1.0))


def step(state, t, draws, a, key, e, max_steps):
    """-> (state', t', draws', r, done): a finished environment already holds its next start state, with t' = 0."""
    new = physics(state, a)
    t = t + 1
    terminated = height(new) > 1.0
    done = terminated or t >= max_steps
    if done:
        new, t, draws = draw(key, e, draws), 0, draws + 1
    return new, t, draws, (0.0 if terminated else -1.0), done


def obs(state):
    """The observation in fp64 (the device stores its float32 cast)."""
    return [math.cos(state[0]), math.sin(state[0]), math.cos(state[1]), math.sin(state[1]), state[2], state[3]]


def energy(s):
    """Mechanical energy of the double pendulum the equations describe: 1/2 q'^T M(q) q' + V(q) with the mass matrix
    [[d1, d2], [d2, m2 lc2^2 + I2]] and V = -(m1 lc1 + m2 l1) g cos th1 - m2 lc2 g cos(th1 + th2) (angles from the
    downward vertical).  Written from the Lagrangian, not from dsdt."""
    th1, th2, w1, w2 = s
    m11 = M1 * LC1 ** 2 + M2 * (L1 ** 2 + LC2 ** 2 + 2 * L1 * LC2 * math.cos(th2)) + I1 + I2
    m12 = M2 * (LC2 ** 2 + L1 * LC2 * math.cos(th2)) + I2
    m22 = M2 * LC2 ** 2 + I2
    kinetic = 0.5 * (m11 * w1 * w1 + 2.0 * m12 * w1 * w2 + m22 * w2 * w2)
    return kinetic - (M1 * LC1 + M2 * L1) * G * math.cos(th1) - M2 * LC2 * G * math.cos(th1 + th2)


# ---- the states the GPU test uploads (tests/test_gpu_env_classic.py), shared so that D64 is measured on exactly them
N_RANDOM = 257
ACTIONS = (1, 0, -1, 2, 7)


def random_states(n=N_RANDOM, seed=1):
    """Angles over the whole circle, velocities up to their clamps; the action of state e is ACTIONS[e % 5]."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-PI, PI, n), rng.uniform(-PI, PI, n), rng.uniform(-MAX_VEL_1, MAX_VEL_1, n),
                     rng.uniform(-MAX_VEL_2, MAX_VEL_2, n)], 1)


def edge_rows():
    """(state, action, what the row is for, expectation): the expectation is ("wrap", component, -1 or +1: the raw angle
    lies beyond pi / -pi and comes back by -+2 pi, the step does not terminate), ("clamp", sign: both raw velocities lie
    beyond their clamps, the new ones are exactly +-4 pi and +-9 pi), ("terminates",) or ("plain",).
    tests/test_env_classic_reference_cpu.py asserts each on this reference."""
    return [([3.0, -3.0, 2.0, 0.0], 1, "th1 wraps down", ("wrap", 0, -1)),
            ([-3.0, 3.0, -2.0, 0.0], 1, "th1 wraps up", ("wrap", 0, 1)),
            ([0.0, 3.0, 0.0, 3.0], 1, "th2 wraps down", ("wrap", 1, -1)),
            ([0.0, -3.0, 0.0, -3.0], 1, "th2 wraps up", ("wrap", 1, 1)),
            ([0.5, 0.2, 12.5, 28.0], 2, "both velocities clamped above", ("clamp", 1)),
            ([-0.5, -0.2, -12.5, -28.0], 0, "both velocities clamped below", ("clamp", -1)),
            ([3.0, 0.1, 0.0, 0.0], 1, "terminates: reward 0", ("terminates",)),
            ([0.0, 0.0, 0.0, 0.0], 1, "hangs still", ("plain",))]


def uploaded_states():
    """[(state, action)] of every state the GPU test steps from an upload: the random ones, then the edge rows."""
    rs = random_states()
    return [(rs[e].tolist(), ACTIONS[e % 5]) for e in range(len(rs))] + [(r[0], r[1]) for r in edge_rows()]
