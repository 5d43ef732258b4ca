"""The loop references of the device Acrobot and MountainCar (tests/acrobot_reference.py, tests/mountaincar_reference.py)
checked without a GPU: the draw rule, hand-computed MountainCar steps and clamps, the Acrobot Runge-Kutta step against
the same derivative integrated finely and against the double pendulum's energy, the edge rows the GPU test uploads, and
the tolerance of the GPU comparison.

The tolerance (STEP_BAR of each reference module) is fixed here: D64 is the largest absolute difference, over exactly
the states tests/test_gpu_env_classic.py uploads (`uploaded_states()`), between the reference in fp64 and the same
reference in np.longdouble; STEP_BAR must be at least 8 * D64 -- a factor of 4 for a device libm at about 2 ulp where the
host's is near 0.5, a factor of 2 of headroom -- and is that rounded up to one digit.  Measured (x86-64, glibc, 80-bit
long double): Acrobot D64 1.12e-12 -> STEP_BAR 9e-12; MountainCar D64 1.09e-16 -> STEP_BAR 9e-16."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import acrobot_reference as ac
import mountaincar_reference as mc
import muax_amd as mx
from muax_amd import _lib, prng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONG = np.longdouble


# ---------------------------------------------------------------- the draw rule
@pytest.mark.parametrize("ref,lo,width,zeros", [(ac, -0.1, 0.2, 0), (mc, -0.6, 0.2, 1)])
def test_draws_follow_the_u53_rule(ref, lo, width, zeros):
    key = prng.PRNGKey(5)
    C_, seen = ref.DRAWN, {}
    for e in range(6):
        for d in range(5):
            s = ref.draw(key, e, d)
            assert len(s) == C_ + zeros and all(x == 0.0 for x in s[C_:])
            for c in range(C_):
                y0, y1 = prng._threefry_int(int(key[0]), int(key[1]), e, C_ * d + c)
                bits = ((y0 << 32) | y1) >> 11
                assert 0 <= bits < 1 << 53
                assert s[c] == lo + width * (bits / float(1 << 53)) and lo <= s[c] < lo + width
                seen[(e, d, c)] = s[c]
    assert len(set(seen.values())) == len(seen)  # distinct across e, d and c
    assert ref.draw(prng.PRNGKey(6), 3, 2) != ref.draw(key, 3, 2)
    assert ref.reset(2, key, 3) == (ref.draw(key, 3, 2), 0, 3)


def test_acrobot_and_mountaincar_counters_differ():
    """C = 4 against C = 1: the same (key, e) gives Acrobot's component c of draw d the uniform MountainCar uses for
    its draw 4 d + c."""
    key = prng.PRNGKey(9)
    for d in range(3):
        for c in range(4):
            u = (ac.draw(key, 2, d)[c] + 0.1) / 0.2
            assert abs(u - (mc.draw(key, 2, 4 * d + c)[0] + 0.6) / 0.2) < 1e-15


# ---------------------------------------------------------------- MountainCar by hand
def test_mountaincar_step_by_hand():
    x, v = -0.5, 0.01
    for a, push in ((0, -0.001), (1, 0.0), (2, 0.001), (-1, -0.001), (7, 0.001)):
        v1 = v + (push + math.cos(3.0 * x) * -0.0025)
        assert mc.physics([x, v], a) == [x + v1, v1]
    # the numbers themselves: cos(-1.5) = 0.0707372016677029
    got = mc.physics([x, v], 2)
    assert abs(got[1] - (0.01 + 0.001 - 0.0025 * 0.0707372016677029)) < 1e-17 and abs(got[0] - (-0.5 + got[1])) < 1e-16
    assert mc.step([x, v], 3, 1, 2, prng.PRNGKey(0), 0, 200) == (got, 4, 1, -1.0, False)


def test_mountaincar_clamps_and_goal():
    for state, a, want, term, what in mc.edge_rows():
        assert mc.physics(state, a) == want, what
        assert mc.terminated(want) is term, what
        new, t, d, r, done = mc.step(state, 0, 0, a, prng.PRNGKey(1), 0, 200)
        assert r == -1.0 and done is term and (new == mc.draw(prng.PRNGKey(1), 0, 0)) is term, what
    rows = {what: (state, a) for state, a, _, _, what in mc.edge_rows()}
    # the clamps are hit with room to spare, so the device's last bits cannot miss them
    for what in ("left wall: x clamped, v zeroed", "v clamped at +0.07", "v clamped at -0.07", "x clamped at 0.6 (done)"):
        assert mc.margin(*rows[what]) >= 1e-6, what
    for what in ("x = 0.5 exactly, v > 0 (done)", "x = 0.5 exactly, v < 0 (not done)"):
        v_raw = mc.raw_step(*rows[what])[0]
        assert abs(v_raw) - mc.MAX_V >= 1e-6, what  # v is the clamp's, and x = x0 +- 0.07 is one exact-input addition
    # "x = 0.5, v = 0": the increment is the same double for any cos(1.5) within 3 ulp of this libm's
    (x, v), a = rows["x = 0.5 exactly, v = 0 (done)"]
    c = math.cos(3.0 * x)
    for k in range(-3, 4):
        ck = c
        for _ in range(abs(k)):
            ck = float(np.nextafter(ck, math.inf if k > 0 else -math.inf))
        assert mc.physics([x, v], a, cos=lambda _: ck) == [0.5, 0.0], k
    # truncation and the left wall without a negative v
    assert mc.step([0.0, 0.0], 2, 0, 1, prng.PRNGKey(0), 0, 3)[3:] == (-1.0, True)
    assert mc.step([0.0, 0.0], 1, 0, 1, prng.PRNGKey(0), 0, 3)[3:] == (-1.0, False)


# ---------------------------------------------------------------- Acrobot against finer integration and against physics
def _fine(state, a, T=ac.DT, n=1000):
    s = list(state)
    for _ in range(n):
        s = ac.rk4(s, a, T / n)
    return s


MILD = [[0.3, -0.2, 0.5, -0.4], [1.0, 0.5, -1.0, 1.5], [-2.0, 1.2, 0.8, -2.0], [0.05, -0.08, 0.02, 0.09]]


@pytest.mark.parametrize("torque", [-1.0, 0.0, 1.0])
def test_acrobot_rk4_step_agrees_with_fine_integration_to_fourth_order(torque):
    """One step of 0.2 against 1000 substeps (whose own error is 1000^-4 of it): the difference is the step's
    truncation error.  Two half steps must cut it by about 2^4 (between 8 and 32: order 3 to 5), which is what "to the
    order an RK4 step allows" means without a constant taken from the code under test.  In absolute terms the error
    is h^5 = 3.2e-4 times a constant of the solution's fifth derivatives; on these mild states (rates up to 2 rad/s,
    accelerations up to 7 rad/s^2) that constant is of order 1 to 10, so the bar is 1e-2 -- a wrong stage weight or
    stage point leaves an O(h^2) or O(h^3) error (0.04 x, 0.008 x the accelerations) and, more sharply, breaks the
    ratio.  Measured: errors 1.1e-4 to 1.9e-3, ratios 13.0 to 19.2."""
    for s in MILD:
        exact = _fine(s, torque)
        one = ac.rk4(s, torque)
        two = ac.rk4(ac.rk4(s, torque, ac.DT / 2), torque, ac.DT / 2)
        e1 = max(abs(x - y) for x, y in zip(one, exact))
        e2 = max(abs(x - y) for x, y in zip(two, exact))
        assert e1 < 1e-2, (s, e1)
        assert 8.0 <= e1 / e2 <= 32.0, (s, e1, e2)


def test_acrobot_energy_is_conserved_without_torque():
    """The equations against physics: with zero torque the finely integrated trajectory (10 steps of 0.2 s, each 1000
    RK4 substeps) keeps 1/2 q'^T M q' + V of the double pendulum, written from the Lagrangian in
    acrobot_reference.energy, not from dsdt.  Measured drift over the 2 s: 6.8e-14 relative to max(1, |E|), energies up
    to 20 (rounding; the substeps' truncation error, 1000^-4 of a step's, is below it); the bar is 1e-10.  A wrong
    sign or coefficient in dsdt drifts by order 1 or more (checked once by flipping the sign of the first Coriolis term:
    15).  With torque the energy
    changes (checked: it must, or the test would pass on a reference that ignores the action)."""
    worst = 0.0
    for s in MILD + [[2.5, -1.0, 3.0, -5.0]]:
        e0, cur = ac.energy(s), list(s)
        for _ in range(10):
            cur = _fine(cur, 0.0)
            worst = max(worst, abs(ac.energy(cur) - e0) / max(1.0, abs(e0)))
    print(f"[energy drift over 2 s of fine integration: {worst:.1e} relative]", end=" ")
    assert worst <= 1e-10
    s = MILD[1]
    assert abs(ac.energy(_fine(s, 1.0)) - ac.energy(s)) > 1e-3
    # and a single RK4 step of 0.2 keeps it to the step's own error
    assert abs(ac.energy(ac.rk4(s, 0.0)) - ac.energy(s)) < 5e-3


def test_acrobot_edge_rows_do_what_they_are_for():
    key, terminating = prng.PRNGKey(1), 0
    for state, a, what, expect in ac.edge_rows():
        raw = ac.rk4(state, ac.torque(a))
        new = ac.physics(state, a)
        assert ac.margin(state, a) >= 1e-6, what
        got, t, d, r, done = ac.step(state, 0, 0, a, key, 0, 500)
        if expect[0] == "wrap":
            _, i, direction = expect
            assert (raw[i] > ac.PI) if direction < 0 else (raw[i] < -ac.PI), what
            assert new[i] == raw[i] + direction * 2 * ac.PI and -ac.PI <= new[i] <= ac.PI, what
            assert not done and r == -1.0 and got == new, what
        elif expect[0] == "clamp":
            sign = expect[1]
            assert sign * raw[2] > ac.MAX_VEL_1 and sign * raw[3] > ac.MAX_VEL_2, what
            assert new[2:] == [sign * 4 * math.pi, sign * 9 * math.pi] and not done, what
        elif expect[0] == "terminates":
            assert ac.height(new) > 1.0 and done and r == 0.0 and got == ac.draw(key, 0, 0) and (t, d) == (0, 1), what
            terminating += 1
        else:
            assert not done and r == -1.0 and got == new == raw, what
    assert terminating == 1


def test_acrobot_actions_rewards_and_truncation():
    s = MILD[0]
    assert ac.physics(s, -1) == ac.physics(s, 0) != ac.physics(s, 1) != ac.physics(s, 2) == ac.physics(s, 7)
    key = prng.PRNGKey(0)
    assert ac.step(s, 1, 0, 1, key, 0, 3)[3:] == (-1.0, False)
    new, t, d, r, done = ac.step(s, 2, 0, 1, key, 0, 3)  # truncated, not terminated: the reward stays -1
    assert done and (t, d, r) == (0, 1, -1.0) and new == ac.draw(key, 0, 0)
    o = ac.obs([0.5, -0.25, 1.0, 2.0])
    assert o == [math.cos(0.5), math.sin(0.5), math.cos(-0.25), math.sin(-0.25), 1.0, 2.0] and len(o) == ac.OBS_DIM
    assert ac.wrap(4.0) == 4.0 - 2 * math.pi and ac.wrap(-10.0) == -10.0 + 2 * math.pi + 2 * math.pi
    assert ac.wrap(math.pi) == math.pi and ac.wrap(-math.pi) == -math.pi and ac.wrap(math.inf) == math.inf


# ---------------------------------------------------------------- the uploaded states and the tolerance
@pytest.mark.parametrize("ref", [ac, mc])
def test_no_uploaded_random_state_is_near_a_branch(ref):
    """No case is skipped: every one of the 257 random states keeps 1e-6 from every threshold, and both outcomes
    (episode ends / goes on) occur among them."""
    states = ref.uploaded_states()[:ref.N_RANDOM]
    assert len(states) == 257
    for e, (s, a) in enumerate(states):
        assert ref.margin(s, a) >= 1e-6, e
        assert a == ref.ACTIONS[e % 5]
    ends = sum(ref.step(s, 7, 0, a, prng.PRNGKey(0), 0, 500)[4] for s, a in states)
    assert 0 < ends < len(states)
    for e in range(2, 257, 5):  # -1 is action 0 and 7 is action 2
        s = states[e][0]
        assert ref.physics(s, -1) == ref.physics(s, 0)
        assert ref.physics(states[e + 2][0], 7) == ref.physics(states[e + 2][0], 2)


def _d64(ref, trig):
    worst = 0.0
    for s, a in ref.uploaded_states():
        f64 = ref.physics(s, a)
        ext = ref.physics([LONG(x) for x in s], a, **trig)
        worst = max(worst, max(abs(float(LONG(x) - y)) for x, y in zip(f64, ext)))
    return worst


@pytest.mark.parametrize("ref,trig", [(ac, dict(cos=np.cos, sin=np.sin)), (mc, dict(cos=np.cos))])
def test_step_bar_is_eight_times_the_fp64_error_of_the_reference(ref, trig):
    if np.finfo(LONG).eps >= np.finfo(np.float64).eps:
        pytest.fail("np.longdouble is no wider than float64 here: D64 cannot be measured on this platform")
    d64 = _d64(ref, trig)
    print(f"[{ref.__name__}: D64 {d64:.3e}, 8 x D64 {8 * d64:.3e}, STEP_BAR {ref.STEP_BAR:.0e}]", end=" ")
    assert d64 > 0.0
    assert 8 * d64 <= ref.STEP_BAR
    digit = float(f"{ref.STEP_BAR:.0e}")
    assert digit == ref.STEP_BAR  # one digit


# ---------------------------------------------------------------- the ABI's Python side and the public names
def test_abi_declares_the_classic_environments():
    """(EXPORTED_SYMBOLS and the field lists against the header: tests/test_abi_cpu.py, for the whole ABI.)"""
    header = open(os.path.join(ROOT, "include", "mzsearch.h")).read()
    assert {"mzs_env_classic_reset", "mzs_env_classic_step"} <= set(_lib.EXPORTED_SYMBOLS)
    fields = [n for n, _ in _lib.MzsEnvClassic._fields_]
    assert fields == ["struct_size", "device", "kind", "num_envs", "max_episode_steps", "key", "state", "t", "draws"]
    assert C.sizeof(_lib.MzsEnvClassic) == 56 and _lib.MzsEnvClassic.state.offset == 32
    for name in ("MZS_ENV_ACROBOT", "MZS_ENV_MOUNTAINCAR"):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == getattr(_lib, name)
    # the cart-pole's descriptor and entries are as they were
    assert C.sizeof(_lib.MzsEnvCartPole) == 48 and {"mzs_env_cartpole_reset", "mzs_env_cartpole_step"} <= set(_lib.EXPORTED_SYMBOLS)


def test_public_names_and_refusals_without_a_gpu():
    for cls, steps, obs_dim in ((mx.DeviceAcrobot, 500, 6), (mx.DeviceMountainCar, 200, 2)):
        assert cls.obs_dim == obs_dim and cls.num_actions == 3
        import inspect
        p = inspect.signature(cls.__init__).parameters
        assert list(p)[1:] == ["n", "max_episode_steps", "seed", "device"]
        assert (p["max_episode_steps"].default, p["seed"].default, p["device"].default) == (steps, 0, None)
        for name in ("reset_device", "step_device", "reset", "step"):
            assert callable(getattr(cls, name))
        with pytest.raises(ValueError, match="at least 1"):
            cls(0)
        with pytest.raises(ValueError, match="GPU"):
            cls(2, device="cpu")
    assert (ac.OBS_DIM, ac.NUM_ACTIONS, mc.OBS_DIM, mc.NUM_ACTIONS) == (6, 3, 2, 3)
    assert callable(mx.test_vector_device)

    class HostEnv:
        n = 2
    with pytest.raises(ValueError, match="step_device"):
        mx.test_vector_device(None, HostEnv(), prng.PRNGKey(0), 4)
