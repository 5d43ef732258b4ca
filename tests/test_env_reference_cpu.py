"""The loop reference of the device cart-pole (tests/cartpole_reference.py) against the host environment it restates
(examples/cartpole_env.VectorCartPole), its draw rule, and fit_vector's refusals of a device environment that would be
stepped through host copies.  No GPU."""
import os
import sys

import numpy as np
import pytest

import cartpole_reference as cp
import muax_amd as mx
from muax_amd import prng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
from cartpole_env import CartPole, VectorCartPole  # noqa: E402


def test_constants_are_the_host_environments():
    c = CartPole
    assert (cp.GRAVITY, cp.M_CART, cp.M_POLE, cp.HALF_LEN, cp.FORCE, cp.DT) == \
        (c.GRAVITY, c.M_CART, c.M_POLE, c.HALF_LEN, c.FORCE, c.DT)
    assert (cp.X_LIMIT, cp.THETA_LIMIT) == (c.X_LIMIT, c.THETA_LIMIT)


def test_reference_step_equals_vector_cartpole():
    """200 random in-range states.  NumPy's vectorised sin / cos and the C library's may differ in the last bit, so the
    new state is compared to 1e-12 absolute (quantities are O(10)); `done` must be equal, which the states' margin of
    1e-6 from both thresholds guarantees."""
    rng = np.random.default_rng(0)
    n = 200
    states = np.stack([rng.uniform(-2.39, 2.39, n), rng.uniform(-3, 3, n), rng.uniform(-0.2, 0.2, n),
                       rng.uniform(-3, 3, n)], 1)
    actions = rng.integers(0, 2, n)
    env = VectorCartPole(n, max_episode_steps=500, seed=0)
    env._state = states.copy()
    env._t[:] = 7
    # the host environment's step, before its auto-reset: the same arithmetic on its own arrays
    _, r, done = env.step(actions)
    worst, dones = 0.0, 0
    for e in range(n):
        new = cp.physics(states[e].tolist(), int(actions[e]))
        assert cp.margin(new) >= 1e-6, e
        _, t, d, r_ref, done_ref = cp.step(states[e].tolist(), 7, 3, int(actions[e]), prng.PRNGKey(0), e, 500)
        assert done_ref == bool(done[e]) and r_ref == r[e] == 1.0
        dones += done_ref
        if done_ref:
            assert (t, d) == (0, 4)
        else:
            assert (t, d) == (8, 3)
            err = float(np.max(np.abs(np.array(new) - env._state[e])))
            worst = max(worst, err)
            assert err <= 1e-12, (e, err)
    assert 0 < dones < n  # both outcomes were compared
    print(f"[reference against VectorCartPole: worst absolute difference {worst:.1e}]", end=" ")


def test_reference_truncates_at_max_steps():
    s = [0.0, 0.0, 0.0, 0.0]
    assert cp.step(s, 1, 0, 1, prng.PRNGKey(0), 0, 3)[4] is False
    new, t, d, r, done = cp.step(s, 2, 0, 1, prng.PRNGKey(0), 0, 3)
    assert done and (t, d, r) == (0, 1, 1.0) and new == cp.draw(prng.PRNGKey(0), 0, 0)


def test_draw_rule():
    key = prng.PRNGKey(5)
    vals = {}
    for e in range(6):
        for d in range(5):
            s = cp.draw(key, e, d)
            assert all(-0.05 <= x < 0.05 for x in s)
            for c in range(4):
                vals[(e, d, c)] = s[c]
    assert len(set(vals.values())) == len(vals)  # distinct across e, d and c
    # known answer for (seed 5, e 3, d 2), from prng's words: counters (3, 8 + c)
    for c in range(4):
        y0, y1 = prng._threefry_int(int(key[0]), int(key[1]), 3, 4 * 2 + c)
        bits = ((y0 << 32) | y1) >> 11
        assert 0 <= bits < 1 << 53
        assert vals[(3, 2, c)] == -0.05 + 0.1 * (bits / float(1 << 53))
    # the extremes of the rule itself
    assert -0.05 + 0.1 * 0.0 == -0.05 and -0.05 + 0.1 * ((2 ** 53 - 1) * 2.0 ** -53) < 0.05
    # a different seed is a different stream
    assert cp.draw(prng.PRNGKey(6), 3, 2) != cp.draw(key, 3, 2)


class _StubDeviceEnv:
    """Has the device protocol's attribute and nothing that could run: the refusals come before any use."""
    n = 2
    step_device = None

    def reset(self):
        raise AssertionError("the environment must not be touched")


def test_fit_vector_refuses_a_device_environment_without_device_collect():
    with pytest.raises(ValueError, match="device_collect"):
        mx.fit_vector(None, _StubDeviceEnv(), None, device_collect=False)


def test_fit_vector_refuses_a_device_environment_with_a_host_buffer():
    with pytest.raises(ValueError, match="add_steps"):
        mx.fit_vector(None, _StubDeviceEnv(), None, buffer=mx.TrajectoryReplayBuffer(10), device_collect=True)
