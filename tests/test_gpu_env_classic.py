"""The two entry points of the device Acrobot and MountainCar (mzs_env_classic_reset / mzs_env_classic_step;
muax_amd/csrc/mz_env.cuh) called directly through muax_amd._lib against the loop references tests/acrobot_reference.py
and tests/mountaincar_reference.py, and the two protocols of `DeviceAcrobot` / `DeviceMountainCar` against each other.

Every tensor a kernel sees lies between guards (tests/replay_abi.Guarded).  `r_out` and `done_out` are the MIDDLE row of
a [3, N] array, so a wrong row stride shows.  After each call everything outside state, t, draws, obs_out, r_out[0:N]
and done_out[0:N] must be bit-identical to what it was.

Tolerances.  Exact: start states (no libm call), t, draws, r, done, a clamped velocity / position, and the casts of the
device's own state in obs.  A stepped state goes through the device's fp64 sin / cos where the reference has the C
library's and is held to the reference module's STEP_BAR (Acrobot 9e-12, MountainCar 9e-16), which
tests/test_env_classic_reference_cpu.py fixes as 8 x the fp64 error of the reference itself on exactly the uploaded
states -- CartPole's 1e-12 is not assumed to carry over.  Acrobot's four trigonometric observations are held to one
float32 ulp of float32(cos / sin(the device's own angle)).  The uploaded random states are asserted on the reference (no
case skipped, tests/test_env_classic_reference_cpu.py and again here) to stay 1e-6 away from every termination
threshold, wrap and clamp, so a last bit cannot flip a branch.  The largest difference seen is printed."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import acrobot_reference as ac
import env_abi
import mountaincar_reference as mc
import muax_amd as mx
from env_abi import _bits32, _stream
from muax_amd import _lib, prng
from replay_abi import Guarded

pytestmark = pytest.mark.gpu
F32 = np.float32
STATE_DIM = {ac: 4, mc: 2}
ABI = {ref: env_abi.EnvAbi(_lib.MzsEnvClassic, "mzs_env_classic_reset", "mzs_env_classic_step", STATE_DIM[ref],
                           ref.OBS_DIM, kind)
       for ref, kind in ((ac, _lib.MZS_ENV_ACROBOT), (mc, _lib.MZS_ENV_MOUNTAINCAR))}
CLS = {ac: "DeviceAcrobot", mc: "DeviceMountainCar"}
MAX_DIFF = {ac: [0.0, 0], mc: [0.0, 0]}  # the largest |device - reference| of a stepped state component, how many states
BOTH = pytest.mark.parametrize("ref", [ac, mc], ids=["acrobot", "mountaincar"])


def Env(ref, N, max_steps, seed, **buffers):
    """Guarded buffers of one mzs_env_classic of `ref`'s kind and the two calls (tests/env_abi.Env)."""
    env = env_abi.Env(ABI[ref], N, max_steps, seed, **buffers)
    env.ref = ref
    return env


def _check_obs(ref, state, obs):
    """obs against the DEVICE's own state: casts exact; Acrobot's cos / sin within one float32 ulp of the float32 of
    the host's fp64 cos / sin of the device's angle."""
    if ref is mc:
        assert np.array_equal(_bits32(obs), _bits32(state.astype(F32)))
        return
    assert np.array_equal(_bits32(obs[:, 4:]), _bits32(state[:, 2:].astype(F32)))
    want = np.stack([np.cos(state[:, 0]), np.sin(state[:, 0]), np.cos(state[:, 1]), np.sin(state[:, 1])], 1).astype(F32)
    assert (np.abs(obs[:, :4] - want) <= np.spacing(np.abs(want))).all()


def _check_step(env, prev, a):
    """The device's step from `prev` = (state, t, draws) against the reference, environment by environment: done, r,
    t and draws exact; a start state exact; a stepped state within STEP_BAR, a component the reference clamped (or the
    wall zeroed) exact; obs from the device's own state.  Returns the number of episodes that ended."""
    ref = env.ref
    state, t, draws, obs, r, done = env.host()
    p_state, p_t, p_draws = prev
    ends = 0
    for e in range(env.N):
        want, wt, wd, wr, wdone = ref.step(p_state[e].tolist(), int(p_t[e]), int(p_draws[e]), int(a[e]), env.key, e,
                                           env.max_steps)
        assert (int(done[e]), r[e], int(t[e]), int(draws[e])) == (int(wdone), wr, wt, wd), e
        if wdone:
            assert state[e].tolist() == want, e
            ends += 1
        else:
            err = float(np.max(np.abs(state[e] - np.array(want))))
            MAX_DIFF[ref][0], MAX_DIFF[ref][1] = max(MAX_DIFF[ref][0], err), MAX_DIFF[ref][1] + 1
            assert err <= ref.STEP_BAR, (e, err)
            for c, limit in _CLAMPS[ref]:
                if abs(want[c]) == limit or (ref is mc and want == [mc.MIN_X, 0.0]):
                    assert state[e][c] == want[c], (e, c)
    _check_obs(ref, state, obs)
    return ends


_CLAMPS = {ac: ((2, ac.MAX_VEL_1), (3, ac.MAX_VEL_2)), mc: ((1, mc.MAX_V), (0, -mc.MIN_X), (0, mc.MAX_X))}


def _report(ref):
    return (f"[{ref.__name__}: largest |device - reference| of a stepped state {MAX_DIFF[ref][0]:.2e} over "
            f"{MAX_DIFF[ref][1]} stepped states; STEP_BAR {ref.STEP_BAR:.0e}]")


@BOTH
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_reset_is_the_references_bit_for_bit(ref, N):
    env = Env(ref, N, 500, seed=11, t=np.full(N, 9))
    for d in (0, 1):  # the second reset gives draw 1
        assert env.reset() == _lib.MZS_OK
        state, t, draws, obs, _, _ = env.host()
        want = np.array([ref.reset(d, env.key, e)[0] for e in range(N)])
        assert np.array_equal(state.view(np.uint64), want.view(np.uint64))
        _check_obs(ref, state, obs)
        assert (t == 0).all() and (draws == d + 1).all()


@BOTH
def test_single_steps_from_uploaded_states(ref):
    """257 states (two workgroups), actions 1, 0, -1, 2, 7, some of them ending their episode."""
    N = ref.N_RANDOM
    states = ref.random_states()
    a = np.array(ref.ACTIONS, np.int32)[np.arange(N) % 5]
    for e in range(N):  # no case is skipped: every step keeps its distance from every branch
        assert ref.margin(states[e].tolist(), int(a[e])) >= 1e-6, e
    t, draws = np.full(N, 7), np.arange(N) % 3
    env = Env(ref, N, 500, seed=4, state=states, t=t, draws=draws)
    assert env.step(a) == _lib.MZS_OK
    ends = _check_step(env, (states, t, draws), a)
    assert 0 < ends < N
    print(_report(ref), end=" ")


def test_acrobot_edge_rows():
    rows = ac.edge_rows()
    states, a = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    N = len(rows)
    env = Env(ac, N, 500, seed=2, state=states)
    assert env.step(a) == _lib.MZS_OK
    z = np.zeros(N, np.int32)
    assert _check_step(env, (states, z, z), a) == 1
    state, _, _, _, r, done = env.host()
    for e, (s0, _, what, expect) in enumerate(rows):
        if expect[0] == "wrap":
            i, direction = expect[1:]
            assert abs(state[e][i]) <= math.pi and np.sign(state[e][i]) == direction and not done[e], what
            assert np.sign(s0[i]) == -direction, what  # it did go round
        elif expect[0] == "clamp":
            assert state[e][2:].tolist() == [expect[1] * 4 * math.pi, expect[1] * 9 * math.pi] and not done[e], what
        elif expect[0] == "terminates":
            assert done[e] == 1 and r[e] == 0.0 and state[e].tolist() == ac.draw(env.key, e, 0), what
        else:
            assert not done[e] and r[e] == -1.0, what
    assert sorted(set(r.tolist())) == [-1.0, 0.0]


def test_mountaincar_edge_rows():
    rows = mc.edge_rows()
    states, a = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    N = len(rows)
    env = Env(mc, N, 200, seed=2, state=states)
    assert env.step(a) == _lib.MZS_OK
    z = np.zeros(N, np.int32)
    ends = _check_step(env, (states, z, z), a)
    state, _, _, obs, r, done = env.host()
    assert ends == sum(term for _, _, _, term, _ in rows) == 3
    for e, (_, _, want, term, what) in enumerate(rows):
        assert int(done[e]) == int(term) and r[e] == -1.0, what
        if not term:  # a finished environment already holds its next start state
            assert state[e].tolist() == want, what
    # the finished ones: the step's own state is gone, so their outcome is checked through done alone, which needs
    # x >= 0.5 and v >= 0 on the device too; "x = 0.5, v < 0" went on with exactly (0.5, -0.07)


@BOTH
@pytest.mark.parametrize("max_steps,t,want", [(1, [0, 0, 0], [1, 1, 1]), (3, [0, 1, 2], [0, 0, 1])])
def test_truncation(ref, max_steps, t, want):
    states = np.zeros((3, STATE_DIM[ref]))  # Acrobot hanging still, the car at rest at x = 0: neither terminates
    env = Env(ref, 3, max_steps, seed=2, state=states, t=t)
    assert env.step([1, 0, 2]) == _lib.MZS_OK
    assert env.host()[5].tolist() == want and (env.host()[4] == -1.0).all()  # truncated, not terminated: reward -1
    _check_step(env, (states, np.array(t), np.zeros(3, np.int32)), [1, 0, 2])


@BOTH
def test_auto_reset_over_time(ref):
    """max_episode_steps 3, 65 environments, 10 steps, every step against the reference stepped from the device's
    previous state (no accumulation along the trajectory)."""
    N, rng = 65, np.random.default_rng(3)
    env = Env(ref, N, 3, seed=8)
    assert env.reset() == _lib.MZS_OK
    finished = np.zeros(N, np.int64)
    for _ in range(10):
        prev = env.host()[:3]
        a = rng.integers(0, 3, N)
        for e in range(N):
            assert ref.margin(prev[0][e].tolist(), int(a[e])) >= 1e-6, e
        assert env.step(a) == _lib.MZS_OK
        _check_step(env, prev, a)
        finished += env.host()[5]
        assert np.array_equal(env.host()[2], 1 + finished)
    assert (finished == 3).all()
    print(_report(ref), end=" ")


@BOTH
def test_refusals_write_nothing(ref):
    env = Env(ref, 5, 3, seed=0)
    E, S = env.descriptor, env.step_args
    bad_envs = [E(struct_size=C.sizeof(_lib.MzsEnvClassic) - 8), E(state=None), E(t=None), E(draws=None),
                E(num_envs=0), E(num_envs=-1), E(max_episode_steps=0), E(kind=0), E(kind=3), E(kind=-1)]
    for d in bad_envs:
        assert env.reset(env=d) == _lib.MZS_E_INVALID
        assert env.step([1] * 5, env=d) == _lib.MZS_E_INVALID
    assert b"unknown kind" in env.L.mzs_last_error(None)
    assert env.L.mzs_env_classic_reset(None, C.c_void_p(env.g["obs"].ptr), _stream()) == _lib.MZS_E_INVALID
    assert env.L.mzs_env_classic_step(C.byref(env.env), None, _stream()) == _lib.MZS_E_INVALID
    assert env.reset(obs=None) == _lib.MZS_E_INVALID
    for s in (S(struct_size=C.sizeof(_lib.MzsEnvStepArgs) + 8), S(a=None), S(obs_out=None), S(r_out=None),
              S(done_out=None)):
        assert env.step([1] * 5, args=s) == _lib.MZS_E_INVALID
    assert b"mzs_env_classic_step" in env.L.mzs_last_error(None)
    # obs_out is written 8 bytes at a time (both kinds), state 16 bytes at a time: a pointer off that is refused
    off_obs, off_state = env.g["obs"].ptr + 4, env.g["state"].ptr + 8
    assert env.reset(obs=off_obs) == _lib.MZS_E_INVALID
    assert env.step([1] * 5, args=S(obs_out=off_obs)) == _lib.MZS_E_INVALID
    assert b"8-byte aligned" in env.L.mzs_last_error(None)
    assert env.reset(env=E(state=off_state)) == _lib.MZS_E_INVALID
    assert env.step([1] * 5, env=E(state=off_state)) == _lib.MZS_E_INVALID
    assert b"16-byte aligned" in env.L.mzs_last_error(None)
    assert env.reset() == _lib.MZS_OK  # the buffers are still usable


@BOTH
def test_obs_out_on_an_eight_byte_boundary_is_accepted(ref):
    """8 bytes is what the entries demand, not 16: an obs_out 8 bytes into the guarded buffer (one row fewer) works and
    writes nothing outside its rows."""
    N = 5
    env = Env(ref, N, 3, seed=6)
    wide = Guarded(N + 1, ref.OBS_DIM, torch.float32, flat=False)
    if (wide.ptr + 8) % 16 == 0:
        pytest.fail("the guarded buffer is not 16-byte aligned itself: the case cannot be built")
    before = wide.bits.clone()
    assert env.L.mzs_env_classic_reset(C.byref(env.env), C.c_void_p(wide.ptr + 8), _stream()) == _lib.MZS_OK
    torch.cuda.synchronize()
    flat = wide.t.reshape(-1).cpu().numpy()
    state = env.g["state"].host()
    _check_obs(ref, state, flat[2:2 + N * ref.OBS_DIM].reshape(N, ref.OBS_DIM))
    changed = (wide.bits != before).cpu().numpy()
    from replay_abi import GUARD
    assert not changed[:GUARD + 2].any() and not changed[GUARD + 2 + N * ref.OBS_DIM:].any() and wide.guards_intact()


@BOTH
def test_host_and_device_protocols_give_one_stream(ref):
    N, rng = 5, np.random.default_rng(0)
    cls = getattr(mx, CLS[ref])
    host, dev, mixed = (cls(N, max_episode_steps=4, seed=21) for _ in range(3))
    assert (dev.n, dev.spec.max_episode_steps, dev.device.type) == (N, 4, "cuda")
    assert (dev.obs_dim, dev.num_actions) == (ref.OBS_DIM, ref.NUM_ACTIONS)
    assert dev.spec.id == {ac: "Acrobot-v1", mc: "MountainCar-v0"}[ref]
    assert cls(2).spec.max_episode_steps == {ac: 500, mc: 200}[ref]
    r_out = torch.zeros(N, dtype=torch.float64, device=dev.device)
    done_out = torch.zeros(N, dtype=torch.uint8, device=dev.device)
    obs_h, obs_d = host.reset(), dev.reset_device()
    assert obs_d.dtype == torch.float32 and tuple(obs_d.shape) == (N, ref.OBS_DIM) and obs_d.is_cuda
    assert np.array_equal(obs_h, obs_d.cpu().numpy()) and np.array_equal(obs_h, mixed.reset())
    want = np.array([ref.draw(prng.PRNGKey(21), e, 0) for e in range(N)])
    assert np.array_equal(dev._state.cpu().numpy().view(np.uint64), want.view(np.uint64)) and obs_h.dtype == F32
    _check_obs(ref, want, obs_h)
    ends = 0
    for i in range(9):
        a = rng.integers(0, 3, N)
        oh, rh, dh = host.step(a)
        od = dev.step_device(torch.as_tensor(a, dtype=torch.int32, device=dev.device), r_out, done_out)
        if i % 2:
            om = mixed.step_device(torch.as_tensor(a, dtype=torch.int32, device=dev.device), r_out, done_out)
            om = om.cpu().numpy()
        else:
            om = mixed.step(a)[0]
        assert np.array_equal(oh, od.cpu().numpy()) and np.array_equal(oh, om)
        assert rh.dtype == np.float64 and np.array_equal(rh, r_out.cpu().numpy()) and (rh == -1.0).all()
        assert dh.dtype == bool and np.array_equal(dh, done_out.cpu().numpy().astype(bool))
        assert torch.equal(host._state, dev._state) and torch.equal(host._state, mixed._state)
        ends += int(dh.sum())
    assert ends == 2 * N and (dev._draws == 3).all()
    with pytest.raises(ValueError, match="r_out"):
        dev.step_device(torch.zeros(N, dtype=torch.int32, device=dev.device), r_out.float(), done_out)
