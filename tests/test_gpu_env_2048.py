"""The three entry points of the device 2048 (mzs_env_2048_reset / mzs_env_2048_step / mzs_env_2048_mask;
muax_amd/csrc/mz_env2048.cuh) called directly through muax_amd._lib against the plain-Python restatement
tests/game2048_reference.py, and the protocols of `Device2048` against each other.

Every tensor a kernel sees lies between guards (tests/replay_abi.Guarded).  `r_out` and `done_out` are the MIDDLE row of
a [3, N] array, so a wrong row stride shows.  After each call everything outside board, t, draws, invalid, obs_out,
r_out[0:N] and done_out[0:N] must be bit-identical to what it was; a refused call must have changed nothing at all.

The environment is integer arithmetic (rewards are integers times a power of two, observations sixteenths): every
comparison is ==."""
import ctypes as C

import numpy as np
import pytest
import torch

import game2048_reference as g
import muax_amd as mx
from env_abi import MIDDLE, _bits32, _stream
from muax_amd import _lib, prng
from replay_abi import Guarded

pytestmark = pytest.mark.gpu
ODD_ACTIONS = [-1, 4, 7, -2 ** 31, 2 ** 31 - 1]


def _u64(grids):
    return np.array([g.pack(x) for x in grids], np.uint64)


class Env:
    """Guarded buffers of one mzs_env_2048 and the three calls."""

    def __init__(self, N, max_steps, seed, shift=0, boards=None, t=None, draws=None):
        self.N, self.max_steps, self.shift, self.seed, self.key = int(N), int(max_steps), shift, seed, prng.PRNGKey(seed)
        z = np.zeros
        boards = z(N, np.uint64) if boards is None else np.asarray(boards, np.uint64)
        self.g = dict(board=Guarded.of(boards.view(np.int64)),
                      t=Guarded.of(np.asarray(z(N) if t is None else t, np.int32)),
                      draws=Guarded.of(np.asarray(z(N) if draws is None else draws, np.int32)),
                      invalid=Guarded(N, 4, torch.uint8, flat=False), obs=Guarded(N, 16, torch.float32, flat=False),
                      a=Guarded(N, 1, torch.int32), r=Guarded(3, N, torch.float64, flat=False),
                      done=Guarded(3, N, torch.uint8, flat=False), witness=Guarded(N, 4, torch.uint8, flat=False))
        self.L = _lib.load()
        self.env = self.descriptor()

    def descriptor(self, **over):
        d = _lib.MzsEnv2048()
        d.struct_size = C.sizeof(_lib.MzsEnv2048)
        d.device, d.num_envs, d.max_episode_steps = torch.cuda.current_device(), self.N, self.max_steps
        d.key[0], d.key[1] = int(self.key[0]), int(self.key[1])
        d.reward_shift = self.shift
        d.board, d.t, d.draws, d.invalid = (self.g[k].ptr for k in ("board", "t", "draws", "invalid"))
        for k, v in over.items():
            setattr(d, k, v)
        return d

    def step_args(self, **over):
        s = _lib.MzsEnvStepArgs()
        s.struct_size = C.sizeof(_lib.MzsEnvStepArgs)
        s.a, s.obs_out = self.g["a"].ptr, self.g["obs"].ptr
        s.r_out, s.done_out = self.g["r"].t[1].data_ptr(), self.g["done"].t[1].data_ptr()
        for k, v in over.items():
            setattr(s, k, v)
        return s

    def _call(self, fn, args, writes):
        """`writes`: the buffers the call may write (r and done: their middle row only)."""
        torch.cuda.synchronize()
        before = {n: x.bits.clone() for n, x in self.g.items()}
        rc = fn(*args, _stream())
        torch.cuda.synchronize()
        for n, x in self.g.items():
            assert x.guards_intact(), f"{fn.__name__}: a guard of {n} was overwritten"
            same = x.bits == before[n]
            if rc == _lib.MZS_OK and n in writes:
                same |= x.row_mask(MIDDLE if n in ("r", "done") else np.ones(x.rows, bool))
            assert bool(same.all()), f"{fn.__name__}: {n} changed where it must not"
        return rc

    def reset(self, env=None, obs="own"):
        obs = self.g["obs"].ptr if obs == "own" else obs
        return self._call(self.L.mzs_env_2048_reset, (C.byref(env or self.env), C.c_void_p(obs)),
                          ("board", "t", "draws", "invalid", "obs"))

    def step(self, a=None, env=None, args=None):
        if a is not None:
            self.g["a"].t.copy_(torch.as_tensor(np.asarray(a, np.int64).astype(np.int32)))
        return self._call(self.L.mzs_env_2048_step, (C.byref(env or self.env), C.byref(args or self.step_args())),
                          ("board", "t", "draws", "invalid", "obs", "r", "done"))

    def mask(self, obs="own", out="own", B=None, device=None):
        obs = self.g["obs"].ptr if obs == "own" else obs
        out = self.g["witness"].ptr if out == "own" else out
        device = torch.cuda.current_device() if device is None else device
        return self._call(self.L.mzs_env_2048_mask,
                          (device, C.c_void_p(obs), C.c_void_p(out), self.N if B is None else B), ("witness",))

    def host(self):
        x = self.g
        return dict(board=x["board"].host().view(np.uint64), t=x["t"].host(), draws=x["draws"].host(),
                    invalid=x["invalid"].host(), obs=x["obs"].host(), r=x["r"].host()[1], done=x["done"].host()[1],
                    witness=x["witness"].host())

    def check(self, ref, r=None, done=None):
        """Everything the device holds against the reference, and the mask kernel on obs as the second witness."""
        assert self.mask() == _lib.MZS_OK
        h = self.host()
        assert np.array_equal(h["board"], ref.boards())
        assert h["t"].tolist() == ref.t and h["draws"].tolist() == ref.draws
        assert np.array_equal(_bits32(h["obs"]), _bits32(ref.obs()))
        assert np.array_equal(h["invalid"], ref.invalid_actions())
        assert np.array_equal(h["witness"], h["invalid"])
        if r is not None:
            assert np.array_equal(h["r"].view(np.uint64), np.asarray(r, np.float64).view(np.uint64))
            assert h["done"].tolist() == [int(x) for x in done]
        return h


def _reference(env):
    return g.Vector2048(env.N, env.max_steps, seed=env.seed, reward_shift=env.shift)


@pytest.mark.parametrize("N", [1, 257])
def test_three_hundred_scripted_steps_equal_the_reference(N):
    """Random actions 0..3 (many of them illegal for their board) with out-of-range values mixed in; random play ends a
    game after one to two hundred moves, so natural ends, resets in the launch and truncation (max 211) all occur."""
    env = Env(N, 211, seed=5, shift=3)
    ref = _reference(env)
    rng = np.random.default_rng(N)
    assert env.reset() == _lib.MZS_OK
    ref.reset()
    env.check(ref)
    noops = ends = natural = merged = 0
    for i in range(300):
        a = np.where(rng.random(N) < 0.9, rng.integers(0, 4, N), rng.choice(ODD_ACTIONS, N))
        draws, t = list(ref.draws), list(ref.t)
        _, r, done = ref.step(a)
        assert env.step(a) == _lib.MZS_OK
        env.check(ref, r, done)
        noops += sum(d1 == d0 for d0, d1, dn in zip(draws, ref.draws, done) if not dn)
        ends, merged = ends + int(done.sum()), merged + int((r > 0).sum())
        natural += sum(bool(dn) and t0 + 1 < 211 for t0, dn in zip(t, done))
    assert noops > 0 and merged > 0 and ends >= N
    if N > 1:
        assert natural > 0 and natural < ends


FULL_WITH_MERGE = [[1, 2, 1, 2], [2, 1, 2, 1], [1, 2, 1, 2], [2, 1, 3, 3]]
CHECKERBOARD = [[1, 2, 1, 2], [2, 1, 2, 1], [1, 2, 1, 2], [2, 1, 2, 1]]
ALL_15 = [[15] * 4 for _ in range(4)]
ONLY_LEFT = [[0, 1, 2, 3], [0, 2, 3, 4], [0, 3, 4, 5], [0, 4, 5, 6]]
ONE_EMPTY = [[1, 2, 1, 2], [2, 1, 2, 1], [1, 2, 0, 3], [2, 1, 4, 1]]  # every move slides one line, none merges
EMPTY = [[0] * 4 for _ in range(4)]
BIG = [[10, 10, 0, 0], [0] * 4, [0] * 4, [0] * 4]
EDGES = [FULL_WITH_MERGE, CHECKERBOARD, ALL_15, ONLY_LEFT, ONE_EMPTY, EMPTY, BIG,
         [[15, 15, 0, 0], [0, 15, 0, 15], [14, 14, 15, 15], [15, 14, 14, 15]]]


@pytest.mark.parametrize("a", [0, 1, 2, 3, 9])
def test_uploaded_edge_boards(a):
    """One empty cell (n = 1), a dead board (ends and resets on this step), a board full of 15s, a board whose only
    legal move is `left`, the empty board, ...: one step of action `a` on each, then three more of mixed actions."""
    N = len(EDGES)
    env = Env(N, 50, seed=9, boards=_u64(EDGES), t=np.arange(N), draws=3 * np.arange(N))
    ref = _reference(env)
    ref.load(_u64(EDGES), np.arange(N), 3 * np.arange(N))
    _, r, done = ref.step([a] * N)
    assert env.step([a] * N) == _lib.MZS_OK
    h = env.check(ref, r, done)
    dead = [EDGES.index(x) for x in (CHECKERBOARD, ALL_15, EMPTY)]
    assert all(h["done"][e] == 1 and h["t"][e] == 0 and h["draws"][e] == 3 * e + 2 and h["r"][e] == 0.0 for e in dead)
    e = EDGES.index(ONLY_LEFT)
    assert (h["draws"][e], h["t"][e], h["done"][e]) == (3 * e + (a == 3), e + 1, 0)
    e = EDGES.index(ONE_EMPTY)  # a move slides tiles over the hole and the spawn fills the one cell left free (n = 1)
    if a in (0, 1, 2, 3):  # (the filled board may be dead and reset at once: draws is the reference's, checked above)
        moved = g.move(ONE_EMPTY, a)[0]
        assert moved != ONE_EMPTY and sum(v == 0 for row in moved for v in row) == 1 and h["draws"][e] > 3 * e
    for k in range(3):
        b = [(a + e + k) % 5 for e in range(N)]
        _, r, done = ref.step(b)
        assert env.step(b) == _lib.MZS_OK
        env.check(ref, r, done)


def test_masks_of_uploaded_boards_after_a_no_op():
    """Action 9 changes nothing, so the masks returned are those of the uploaded boards themselves."""
    boards = [FULL_WITH_MERGE, ONLY_LEFT, ONE_EMPTY, BIG]
    env = Env(4, 50, seed=1, boards=_u64(boards))
    assert env.step([9] * 4) == _lib.MZS_OK
    h = env.host()
    assert h["invalid"].tolist() == [[1, 0, 1, 0], [1, 1, 1, 0], [0, 0, 0, 0], [1, 0, 0, 0]]
    assert h["invalid"].tolist() == [g.mask(b) for b in boards] and (h["r"] == 0).all() and (h["draws"] == 0).all()
    assert np.array_equal(h["board"], _u64(boards)) and h["t"].tolist() == [1] * 4 and not h["done"].any()


def test_max_episode_steps_one():
    env = Env(5, 1, seed=2)
    ref = _reference(env)
    assert env.reset() == _lib.MZS_OK
    ref.reset()
    for i in range(4):
        a = [(e + i) % 4 for e in range(5)]
        _, r, done = ref.step(a)
        assert env.step(a) == _lib.MZS_OK
        h = env.check(ref, r, done)
        assert h["done"].tolist() == [1] * 5 and h["t"].tolist() == [0] * 5
    assert (h["draws"] >= 2 * 5).all()


@pytest.mark.parametrize("shift,want", [(0, 2048.0), (11, 1.0), (3, 256.0)])
def test_reward_shift_on_a_2048_merge(shift, want):
    env = Env(2, 50, seed=3, shift=shift, boards=_u64([BIG, [[1, 1, 0, 0], [0] * 4, [0] * 4, [0] * 4]]))
    ref = _reference(env)
    ref.load(_u64([BIG, [[1, 1, 0, 0], [0] * 4, [0] * 4, [0] * 4]]))
    _, r, done = ref.step([3, 3])
    assert env.step([3, 3]) == _lib.MZS_OK
    h = env.check(ref, r, done)
    assert h["r"].tolist() == [want, 4.0 / 2 ** shift]


def test_mask_kernel_on_observations():
    """All-zero rows report 0; inexact observations are decoded by rint and clamped to 0..15; 257 rows, two blocks."""
    rng = np.random.default_rng(4)
    N = 257
    env = Env(N, 50, seed=0)
    cells = np.where(rng.random((N, 16)) < 0.7, rng.integers(1, 16, (N, 16)), 0)
    cells[0] = 0
    cells[1:1 + len(EDGES)] = [np.array(x).reshape(-1) for x in EDGES]
    obs = (cells / 16.0).astype(np.float32)
    obs[40:80] += rng.uniform(-0.03, 0.03, (40, 16)).astype(np.float32)  # within half a step (1 / 32) of the cell
    obs[80] = cells[80] / 16.0 + 4.0   # far above: clamped to 15
    obs[81] = -cells[81] / 16.0        # negative: clamped to 0, an empty board
    env.g["obs"].t.copy_(torch.as_tensor(obs))
    assert env.mask() == _lib.MZS_OK
    got = env.host()["witness"]
    want = np.array([g.mask(g.grid_of_obs(row)) for row in obs], np.uint8)
    assert np.array_equal(got, want)
    assert got[0].tolist() == [0, 0, 0, 0] and got[81].tolist() == [0, 0, 0, 0] and got[80].tolist() == [1, 1, 1, 1]
    assert np.array_equal(want[40:80], np.array([g.mask(c.reshape(4, 4).tolist()) for c in cells[40:80]], np.uint8))
    assert 0 < want.sum() < want.size
    # B below the buffer's rows: the rows past B keep what they held
    env.g["obs"].t.zero_()
    assert env.mask(B=3) == _lib.MZS_OK
    after = env.host()["witness"]
    assert not after[:3].any() and np.array_equal(after[3:], want[3:])


def test_refusals_write_nothing():
    env = Env(5, 3, seed=0)
    E, S = env.descriptor, env.step_args
    g4 = env.g
    bad_envs = [E(struct_size=C.sizeof(_lib.MzsEnv2048) - 8), E(board=None), E(t=None), E(draws=None), E(invalid=None),
                E(num_envs=0), E(num_envs=-1), E(max_episode_steps=0), E(reward_shift=-1), E(reward_shift=12),
                E(board=g4["board"].ptr + 4), E(invalid=g4["invalid"].ptr + 2), E(invalid=g4["invalid"].ptr + 1),
                E(t=g4["t"].ptr + 2), E(draws=g4["draws"].ptr + 1)]
    for d in bad_envs:
        assert env.reset(env=d) == _lib.MZS_E_INVALID
        assert env.step([1] * 5, env=d) == _lib.MZS_E_INVALID
    assert env.reset(env=E(reward_shift=12)) == _lib.MZS_E_INVALID
    assert b"reward_shift" in env.L.mzs_last_error(None)
    assert env.reset(env=E(board=g4["board"].ptr + 4)) == _lib.MZS_E_INVALID
    assert b"board must be 8-byte aligned" in env.L.mzs_last_error(None)
    assert env.step([1] * 5, env=E(invalid=g4["invalid"].ptr + 2)) == _lib.MZS_E_INVALID
    assert b"mzs_env_2048_step: invalid must be 4-byte aligned" in env.L.mzs_last_error(None)
    assert env.L.mzs_env_2048_reset(None, C.c_void_p(g4["obs"].ptr), _stream()) == _lib.MZS_E_INVALID
    assert env.L.mzs_env_2048_step(C.byref(env.env), None, _stream()) == _lib.MZS_E_INVALID
    assert env.reset(obs=None) == _lib.MZS_E_INVALID
    for off in (4, 8):
        assert env.reset(obs=g4["obs"].ptr + off) == _lib.MZS_E_INVALID
        assert env.step([1] * 5, args=S(obs_out=g4["obs"].ptr + off)) == _lib.MZS_E_INVALID
        assert b"obs_out must be 16-byte aligned" in env.L.mzs_last_error(None)
    for s in (S(struct_size=C.sizeof(_lib.MzsEnvStepArgs) + 8), S(a=None), S(obs_out=None), S(r_out=None),
              S(done_out=None), S(a=g4["a"].ptr + 2), S(r_out=g4["r"].t[1].data_ptr() + 4)):
        assert env.step([1] * 5, args=s) == _lib.MZS_E_INVALID
    assert b"mzs_env_2048_step" in env.L.mzs_last_error(None)
    for kw in (dict(obs=None), dict(out=None), dict(B=0), dict(B=-3), dict(obs=g4["obs"].ptr + 8),
               dict(out=g4["witness"].ptr + 2), dict(device=-1), dict(device=4096)):
        assert env.mask(**kw) == _lib.MZS_E_INVALID
    assert b"mzs_env_2048_mask" in env.L.mzs_last_error(None)
    assert env.reset() == _lib.MZS_OK  # the buffers are still usable
    ref = _reference(env)
    ref.reset()
    env.check(ref)


def test_host_and_device_protocols_give_one_stream():
    N, rng = 6, np.random.default_rng(0)
    host, dev, mixed = (mx.Device2048(N, max_episode_steps=5, seed=21, reward_shift=2) for _ in range(3))
    ref = g.Vector2048(N, 5, seed=21, reward_shift=2)
    assert (dev.n, dev.spec.max_episode_steps, dev.device.type, dev.spec.id) == (N, 5, "cuda", "2048")
    assert mx.Device2048(2).spec.max_episode_steps == 2000 and mx.Device2048(2).reward_shift == 0
    r_out = torch.zeros(N, dtype=torch.float64, device=dev.device)
    done_out = torch.zeros(N, dtype=torch.uint8, device=dev.device)
    mask = dev.invalid_actions_device()
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (N, 4) and mask.is_cuda
    obs_h, obs_d, obs_r = host.reset(), dev.reset_device(), ref.reset()
    assert obs_d.dtype == torch.float32 and tuple(obs_d.shape) == (N, 16) and obs_h.dtype == np.float32
    assert np.array_equal(obs_h, obs_d.cpu().numpy()) and np.array_equal(obs_h, mixed.reset())
    assert np.array_equal(obs_h, obs_r)
    ends = 0
    for i in range(12):
        assert dev.invalid_actions_device() is mask  # the same object, overwritten in place
        assert np.array_equal(mask.cpu().numpy(), ref.invalid_actions())
        assert np.array_equal(host.invalid_actions(), ref.invalid_actions())
        assert torch.equal(dev.invalid_actions_of(obs_d), mask)
        a = rng.integers(0, 4, N)
        oh, rh, dh = host.step(a)
        obs_d = dev.step_device(torch.as_tensor(a, dtype=torch.int32, device=dev.device), r_out, done_out)
        if i % 2:
            om = mixed.step_device(torch.as_tensor(a, dtype=torch.int32, device=dev.device), r_out, done_out)
            om = om.cpu().numpy()
        else:
            om = mixed.step(a)[0]
        orf, rr, dr = ref.step(a)
        assert np.array_equal(oh, obs_d.cpu().numpy()) and np.array_equal(oh, om) and np.array_equal(oh, orf)
        assert rh.dtype == np.float64 and np.array_equal(rh, r_out.cpu().numpy()) and np.array_equal(rh, rr)
        assert dh.dtype == bool and np.array_equal(dh, done_out.cpu().numpy().astype(bool)) and np.array_equal(dh, dr)
        assert torch.equal(host._board, dev._board) and torch.equal(host._board, mixed._board)
        ends += int(dh.sum())
    assert ends == 2 * N and dev._draws.cpu().tolist() == ref.draws
    zero = torch.zeros((3, 16), dtype=torch.float32, device=dev.device)
    assert not dev.invalid_actions_of(zero).any()
    with pytest.raises(ValueError, match="r_out"):
        dev.step_device(torch.zeros(N, dtype=torch.int32, device=dev.device), r_out.float(), done_out)
    with pytest.raises(ValueError, match="invalid_actions_of"):
        dev.invalid_actions_of(zero[:, :8])
    with pytest.raises(ValueError, match="invalid_actions_of"):
        dev.invalid_actions_of(zero.double())
