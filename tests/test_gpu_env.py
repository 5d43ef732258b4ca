"""The two device-environment entry points of the C ABI (mzs_env_cartpole_reset / mzs_env_cartpole_step;
muax_amd/csrc/mz_env.cuh) called directly through muax_amd._lib against the loop reference tests/cartpole_reference.py,
and `DeviceCartPole`'s two protocols against each other.

Every tensor a kernel sees lies between guards (tests/replay_abi.Guarded).  `r_out` and `done_out` are the MIDDLE row of
a [3, N] array, so a wrong row stride shows.  After each call everything outside state, t, draws, obs_out, r_out[0:N]
and done_out[0:N] must be bit-identical to what it was.

Tolerances: start states (no libm call) are compared bit for bit.  A stepped state goes through the device's fp64
sin / cos where the reference has the C library's: quantities are O(10) and the error a few ulps of sin / cos, so the
bar is 1e-12 absolute, the one the project uses for pow.  Random test states are asserted (on the reference, no case
skipped) to end at least 1e-6 away from both thresholds, so a last-bit difference cannot flip `done`; the threshold
cases have a zero velocity, for which the new x / theta is the old one bit for bit whatever the libm."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import cartpole_reference as cp
import env_abi
import muax_amd as mx
from env_abi import _bits32
from muax_amd import _lib, prng

pytestmark = pytest.mark.gpu
F32 = np.float32
MAX_DIFF = {"step": 0.0, "n": 0}  # the largest |device - reference| of a stepped state component, and how many states
CARTPOLE = env_abi.EnvAbi(_lib.MzsEnvCartPole, "mzs_env_cartpole_reset", "mzs_env_cartpole_step", 4, 4)


def Env(N, max_steps, seed, **buffers):
    """Guarded buffers of one mzs_env_cartpole and the two calls (tests/env_abi.Env)."""
    return env_abi.Env(CARTPOLE, N, max_steps, seed, **buffers)


def _check_step(env, prev, a):
    """The device's step from `prev` = (state, t, draws) against the reference, environment by environment: done, r,
    t and draws exact; a start state exact; a stepped state within 1e-12; obs = (float)state of the device's own."""
    state, t, draws, obs, r, done = env.host()
    p_state, p_t, p_draws = prev
    ends = 0
    for e in range(env.N):
        want, wt, wd, wr, wdone = cp.step(p_state[e].tolist(), int(p_t[e]), int(p_draws[e]), int(a[e]), env.key, e,
                                          env.max_steps)
        assert (int(done[e]), r[e], int(t[e]), int(draws[e])) == (int(wdone), wr, wt, wd), e
        if wdone:
            assert state[e].tolist() == want, e
            ends += 1
        else:
            err = float(np.max(np.abs(state[e] - np.array(want))))
            MAX_DIFF["step"], MAX_DIFF["n"] = max(MAX_DIFF["step"], err), MAX_DIFF["n"] + 1
            assert err <= 1e-12, (e, err)
    assert np.array_equal(_bits32(obs), _bits32(state.astype(F32)))
    return ends


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_reset_is_the_references_bit_for_bit(N):
    env = Env(N, 500, seed=11, t=np.full(N, 9))
    for d in (0, 1):  # the second reset gives draw 1
        assert env.reset() == _lib.MZS_OK
        state, t, draws, obs, _, _ = env.host()
        want = np.array([cp.reset(d, env.key, e)[0] for e in range(N)])
        assert np.array_equal(state.view(np.uint64), want.view(np.uint64))
        assert np.array_equal(_bits32(obs), _bits32(want.astype(F32)))
        assert (t == 0).all() and (draws == d + 1).all()


def random_states(n, seed=1):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-2.39, 2.39, n), rng.uniform(-3, 3, n), rng.uniform(-0.2, 0.2, n),
                     rng.uniform(-3, 3, n)], 1)


def test_single_steps_from_uploaded_states():
    """257 states (two workgroups), both actions and -1, 2, 7 (all -FORCE), some of them ending their episode."""
    N = 257
    states = random_states(N)
    a = np.array([1, 0, -1, 2, 7], np.int32)[np.arange(N) % 5]
    for e in range(N):  # no case is skipped: every stepped state keeps its distance from both thresholds
        assert cp.margin(cp.physics(states[e].tolist(), int(a[e]))) >= 1e-6, e
    for e in range(2, N, 5):  # -1 (and 2, 7) are the reference's -FORCE too
        assert cp.physics(states[e].tolist(), int(a[e])) == cp.physics(states[e].tolist(), 0)
    t, draws = np.full(N, 7), np.arange(N) % 3
    env = Env(N, 500, seed=4, state=states, t=t, draws=draws)
    assert env.step(a) == _lib.MZS_OK
    ends = _check_step(env, (states, t, draws), a)
    assert 0 < ends < N
    print(f"[stepped state against the reference: largest absolute difference {MAX_DIFF['step']:.1e} over "
          f"{MAX_DIFF['n']} stepped states]", end=" ")


def test_thresholds_exactly():
    up = math.inf
    X, TH = cp.X_LIMIT, cp.THETA_LIMIT
    rows = [([X, 0, 0, 0], 0), ([np.nextafter(X, up), 0, 0, 0], 1), ([-X, 0, 0, 0], 0),
            ([np.nextafter(-X, -up), 0, 0, 0], 1), ([0, 0, TH, 0], 0), ([0, 0, np.nextafter(TH, up), 0], 1),
            ([0, 0, -TH, 0], 0), ([0, 0, np.nextafter(-TH, -up), 0], 1),
            ([np.nextafter(X, 0), 1.0, 0, 0], 1), ([0, 0, 0, 0], 0)]
    states = np.array([s for s, _ in rows], np.float64)
    want_done = np.array([d for _, d in rows])
    N = len(rows)
    for a in (0, 1):
        t = np.zeros(N, np.int32)
        env = Env(N, 3, seed=2, state=states, t=t)
        assert env.step(np.full(N, a)) == _lib.MZS_OK
        assert np.array_equal(env.host()[5], want_done)
        _check_step(env, (states, t, np.zeros(N, np.int32)), np.full(N, a))


@pytest.mark.parametrize("max_steps,t,want", [(1, [0, 0, 0], [1, 1, 1]), (3, [0, 1, 2], [0, 0, 1])])
def test_truncation(max_steps, t, want):
    states = np.zeros((3, 4))
    env = Env(3, max_steps, seed=2, state=states, t=t)
    assert env.step([1, 0, 1]) == _lib.MZS_OK
    assert env.host()[5].tolist() == want
    _check_step(env, (states, np.array(t), np.zeros(3, np.int32)), [1, 0, 1])


def test_auto_reset_over_time():
    """max_episode_steps 3, 65 environments, 10 steps, every step against the reference stepped from the device's
    previous state (no accumulation along the chaotic trajectory)."""
    N, rng = 65, np.random.default_rng(3)
    env = Env(N, 3, seed=8)
    assert env.reset() == _lib.MZS_OK
    finished = np.zeros(N, np.int64)
    for _ in range(10):
        prev = env.host()[:3]
        a = rng.integers(0, 2, N)
        assert env.step(a) == _lib.MZS_OK
        _check_step(env, prev, a)
        finished += env.host()[5]
        assert np.array_equal(env.host()[2], 1 + finished)
    assert (finished == 3).all()
    print(f"[largest absolute difference so far {MAX_DIFF['step']:.1e} over {MAX_DIFF['n']} stepped states]", end=" ")


def test_refusals_write_nothing():
    env = Env(5, 3, seed=0)
    E, S = env.descriptor, env.step_args
    bad_envs = [E(struct_size=C.sizeof(_lib.MzsEnvCartPole) - 8), E(state=None), E(t=None), E(draws=None),
                E(num_envs=0), E(num_envs=-1), E(max_episode_steps=0)]
    for d in bad_envs:
        assert env.reset(env=d) == _lib.MZS_E_INVALID
        assert env.step([1] * 5, env=d) == _lib.MZS_E_INVALID
    assert env.reset(obs=None) == _lib.MZS_E_INVALID
    for s in (S(struct_size=C.sizeof(_lib.MzsEnvStepArgs) + 8), S(a=None), S(obs_out=None), S(r_out=None),
              S(done_out=None)):
        assert env.step([1] * 5, args=s) == _lib.MZS_E_INVALID
    assert b"mzs_env_cartpole_step" in env.L.mzs_last_error(None)
    # state and obs_out are read and written 16 bytes at a time: a pointer off that alignment is refused too
    off_obs, off_state = env.g["obs"].ptr + 4, env.g["state"].ptr + 8
    assert env.reset(obs=off_obs) == _lib.MZS_E_INVALID
    assert env.step([1] * 5, args=S(obs_out=off_obs)) == _lib.MZS_E_INVALID
    assert b"16-byte aligned" in env.L.mzs_last_error(None)
    assert env.reset(env=E(state=off_state)) == _lib.MZS_E_INVALID
    assert env.step([1] * 5, env=E(state=off_state)) == _lib.MZS_E_INVALID
    assert env.reset() == _lib.MZS_OK  # the buffers are still usable


def test_device_cartpole_host_and_device_protocols_give_one_stream():
    N, rng = 5, np.random.default_rng(0)
    host, dev, mixed = (mx.DeviceCartPole(N, max_episode_steps=4, seed=21) for _ in range(3))
    assert (dev.n, dev.spec.max_episode_steps, dev.device.type) == (N, 4, "cuda")
    r_out = torch.zeros(N, dtype=torch.float64, device=dev.device)
    done_out = torch.zeros(N, dtype=torch.uint8, device=dev.device)
    obs_h, obs_d = host.reset(), dev.reset_device()
    assert obs_d.dtype == torch.float32 and tuple(obs_d.shape) == (N, 4) and obs_d.is_cuda
    assert np.array_equal(obs_h, obs_d.cpu().numpy()) and np.array_equal(obs_h, mixed.reset())
    want = np.array([cp.draw(prng.PRNGKey(21), e, 0) for e in range(N)]).astype(F32)
    assert obs_h.dtype == F32 and np.array_equal(_bits32(obs_h), _bits32(want))
    ends = 0
    for i in range(9):
        a = rng.integers(0, 2, N)
        oh, rh, dh = host.step(a)
        od = dev.step_device(torch.as_tensor(a, dtype=torch.int32, device=dev.device), r_out, done_out)
        if i % 2:
            om = mixed.step_device(torch.as_tensor(a, dtype=torch.int32, device=dev.device), r_out, done_out)
            om = om.cpu().numpy()
        else:
            om = mixed.step(a)[0]
        assert np.array_equal(oh, od.cpu().numpy()) and np.array_equal(oh, om)
        assert rh.dtype == np.float64 and np.array_equal(rh, r_out.cpu().numpy()) and (rh == 1.0).all()
        assert dh.dtype == bool and np.array_equal(dh, done_out.cpu().numpy().astype(bool))
        assert torch.equal(host._state, dev._state) and torch.equal(host._state, mixed._state)
        ends += int(dh.sum())
    assert ends == 2 * N and (dev._draws == 3).all()
    with pytest.raises(ValueError, match="r_out"):
        dev.step_device(torch.zeros(N, dtype=torch.int32, device=dev.device), r_out.float(), done_out)
