"""Plain-loop restatement of the device cart-pole (include/mzsearch.h, mzs_env_cartpole_*; DESIGN.md 4.7 "Device
environments") in Python floats, one environment and one step at a time, written from the equations and the draw rule.
math.sin / math.cos and prng.threefry2x32; it shares nothing with muax_amd/envs.py or the kernels."""
import math

from muax_amd import prng

GRAVITY, M_CART, M_POLE, HALF_LEN, FORCE, DT = 9.8, 1.0, 0.1, 0.5, 10.0, 0.02
X_LIMIT, THETA_LIMIT = 2.4, 12 * 2 * math.pi / 360


def u53(key, x0, x1):
    """((y0 << 32 | y1) >> 11) * 2^-53 of threefry2x32(key, x0, x1): exact integer arithmetic, then one exact scaling."""
    y0, y1 = prng.threefry2x32(key, x0 & 0xFFFFFFFF, x1 & 0xFFFFFFFF)
    return float(((int(y0) << 32) | int(y1)) >> 11) * 2.0 ** -53


def draw(key, e, d):
    """The d-th start state of environment e."""
    return [-0.05 + 0.1 * u53(key, e, 4 * d + c) for c in range(4)]


def reset(draws, key, e):
    """-> (state, t, draws')"""
    return draw(key, e, draws), 0, draws + 1


def physics(state, a):
    """One explicit Euler step of the Barto-Sutton-Anderson cart-pole; any action other than 1 pushes left."""
    x, x_dot, th, th_dot = state
    f = FORCE if a == 1 else -FORCE
    m_total, pm_l = M_CART + M_POLE, M_POLE * HALF_LEN
    c, s = math.cos(th), math.sin(th)
    tmp = (f + pm_l * th_dot * th_dot * s) / m_total
    th_acc = (GRAVITY * s - c * tmp) / (HALF_LEN * (4.0 / 3.0 - M_POLE * c * c / m_total))
    x_acc = tmp - pm_l * th_acc * c / m_total
    return [x + DT * x_dot, x_dot + DT * x_acc, th + DT * th_dot, th_dot + DT * th_acc]


def margin(new_state):
    """Distance of the stepped state from the nearer of the two termination thresholds."""
    return min(abs(abs(new_state[0]) - X_LIMIT), abs(abs(new_state[2]) - THETA_LIMIT))


def step(state, t, draws, a, key, e, max_steps):
    """-> (state', t', draws', r, done): a finished environment already holds its next start state, with t' = 0."""
    new = physics(state, a)
    t = t + 1
    done = abs(new[0]) > X_LIMIT or abs(new[2]) > THETA_LIMIT or t >= max_steps
    if done:
        new, t, draws = draw(key, e, draws), 0, draws + 1
    return new, t, draws, 1.0, done
