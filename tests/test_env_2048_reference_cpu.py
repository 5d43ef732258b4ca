"""The plain-Python restatement of the device 2048 (tests/game2048_reference.py) checked without a GPU: known-answer
lines in every direction, termination, the spawn rule on a fixed key, no-ops, rewards; then the Python side of the ABI,
the public names and the constructor's refusals.  Everything is integers (or powers of two): every comparison is ==."""
import ctypes as C
import inspect

import numpy as np
import pytest

import game2048_reference as g
import muax_amd as mx
from muax_amd import _lib, prng

# exponents: 1 is the tile 2, 2 the tile 4, ...; (line read from the edge the tiles slide to, result, tiles created)
LINES = [([1, 1, 1, 1], [2, 2, 0, 0], 8),        # 2 2 2 2 -> 4 4 . .
         ([1, 1, 2, 0], [2, 2, 0, 0], 4),        # 2 2 4 . -> 4 4 . .   (the new 4 does not merge again)
         ([2, 0, 2, 2], [3, 2, 0, 0], 8),        # 4 . 4 4 -> 8 4 . .   (merges start from the edge)
         ([1, 0, 0, 1], [2, 0, 0, 0], 4),        # 2 . . 2 -> 4 . . .
         ([15, 15, 0, 0], [15, 15, 0, 0], 0),    # two 32768s do not merge (and here do not move)
         ([0, 15, 0, 15], [15, 15, 0, 0], 0),    # ... but they slide
         ([3, 2, 1, 0], [3, 2, 1, 0], 0),        # a line that does not move
         ([14, 14, 0, 0], [15, 0, 0, 0], 32768)]


@pytest.mark.parametrize("a", [g.UP, g.RIGHT, g.DOWN, g.LEFT])
@pytest.mark.parametrize("line,want,gained", LINES)
@pytest.mark.parametrize("where", [0, 1, 2, 3])
def test_known_lines_in_every_direction(a, line, want, gained, where):
    """The line laid into line `where` of move `a` (the other cells empty), by hand: for `up` the line is a column read
    from the top, for `right` a row read from the right, ..."""
    cells = {g.LEFT: [(where, c) for c in range(4)], g.RIGHT: [(where, 3 - c) for c in range(4)],
             g.UP: [(r, where) for r in range(4)], g.DOWN: [(3 - r, where) for r in range(4)]}[a]
    grid, expect = [[0] * 4 for _ in range(4)], [[0] * 4 for _ in range(4)]
    for (r, c), v, w in zip(cells, line, want):
        grid[r][c], expect[r][c] = v, w
    assert g.slide(line) == (want, gained)
    assert g.move(grid, a) == (expect, gained)
    assert g.legal(grid, a) is (line != want)
    assert g.mask(grid)[a] == (1 if line == want else 0)


def test_moves_by_hand_on_a_whole_grid():
    grid = [[1, 1, 0, 0],
            [2, 0, 2, 0],
            [0, 0, 0, 3],
            [1, 0, 0, 3]]
    assert g.move(grid, g.LEFT) == ([[2, 0, 0, 0], [3, 0, 0, 0], [3, 0, 0, 0], [1, 3, 0, 0]], 4 + 8)
    assert g.move(grid, g.RIGHT) == ([[0, 0, 0, 2], [0, 0, 0, 3], [0, 0, 0, 3], [0, 0, 1, 3]], 4 + 8)
    assert g.move(grid, g.UP) == ([[1, 1, 2, 4], [2, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]], 16)
    assert g.move(grid, g.DOWN) == ([[0, 0, 0, 0], [1, 0, 0, 0], [2, 0, 0, 0], [1, 1, 2, 4]], 16)
    for a in (-1, 4, 7, 2 ** 31 - 1, -2 ** 31):
        assert g.move(grid, a) == (grid, 0) and not g.legal(grid, a)
    assert g.pack(grid) == 0x3001_3000_0202_0011 and g.unpack(g.pack(grid)) == grid
    assert g.obs(grid)[:5] == [1 / 16, 1 / 16, 0.0, 0.0, 2 / 16] and len(g.obs(grid)) == g.OBS_DIM
    assert g.grid_of_obs(g.obs(grid)) == grid


FULL_WITH_MERGE = [[1, 2, 1, 2], [2, 1, 2, 1], [1, 2, 1, 2], [2, 1, 3, 3]]   # the last two of the bottom row are equal
CHECKERBOARD = [[1, 2, 1, 2], [2, 1, 2, 1], [1, 2, 1, 2], [2, 1, 2, 1]]
ALL_15 = [[15] * 4 for _ in range(4)]
ONLY_LEFT = [[0, 1, 2, 3], [0, 2, 3, 4], [0, 3, 4, 5], [0, 4, 5, 6]]         # only `left` changes it


def test_termination_and_masks():
    assert not g.dead(FULL_WITH_MERGE) and g.mask(FULL_WITH_MERGE) == [1, 0, 1, 0]
    assert g.dead(CHECKERBOARD) and g.mask(CHECKERBOARD) == [1, 1, 1, 1]
    assert g.dead(ALL_15) and g.mask(ALL_15) == [1, 1, 1, 1]  # 15 | 15 does not merge: a full board of them is dead
    assert not g.dead(ONLY_LEFT) and g.mask(ONLY_LEFT) == [1, 1, 1, 0]
    empty = [[0] * 4 for _ in range(4)]
    assert g.mask(empty) == [0, 0, 0, 0]  # the zero-padded reanalysis row: every move "legal"
    assert g.dead(empty)                  # ... while no move changes it, so an uploaded empty board ends at once
    key = prng.PRNGKey(3)
    # a dead board ends on its next step whatever the action, and the environment is reset in that step
    for a in (0, 3, 9):
        new, t, d, r, done = g.step(CHECKERBOARD, 5, 7, a, key, 2, 100)
        assert done and (t, d, r) == (0, 9, 0.0) and new == g.reset(7, key, 2)[0]
    # a full board with a merge goes on, and the merge frees the cell of the spawn
    new, t, d, r, done = g.step(FULL_WITH_MERGE, 5, 7, g.RIGHT, key, 2, 100)
    assert not done and (t, d, r) == (6, 8, 16.0) and sum(v == 0 for row in new for v in row) == 0
    assert new[3][1:] == [2, 1, 4] and new[3][0] in (1, 2)
    # truncation: t reaches max_episode_steps
    assert g.step(ONLY_LEFT, 0, 0, g.LEFT, key, 0, 1)[4] and not g.step(ONLY_LEFT, 0, 0, g.LEFT, key, 0, 2)[4]


def test_spawn_rule_on_a_fixed_key():
    """k = (x0 * n) >> 32 of the empty cells in ascending cell index, n = 1, 15 and 16; exponent 2 below 0x1999999A."""
    key = prng.PRNGKey(5)
    one_empty = [[1, 2, 1, 2], [2, 1, 2, 1], [1, 2, 0, 2], [2, 1, 2, 1]]
    fifteen = [[0] * 4 for _ in range(4)]
    fifteen[1][2] = 3
    sixteen = [[0] * 4 for _ in range(4)]
    seen_k = set()
    for e in range(4):
        for d in range(40):
            x0, x1 = g.block(key, e, d)
            assert (x0, x1) == tuple(int(w) for w in prng.threefry2x32(key, e, d))
            v = 2 if x1 < 0x1999999A else 1
            assert g.spawn_block(one_empty, x0, x1) == (2, 2, v)  # n = 1: k = 0 for every x0
            k15, k16 = (x0 * 15) >> 32, (x0 * 16) >> 32
            assert 0 <= k15 < 15 and k16 == x0 >> 28
            cells15 = [c for c in range(16) if c != 6]
            assert g.spawn_block(fifteen, x0, x1) == (cells15[k15] // 4, cells15[k15] % 4, v)
            assert g.spawn_block(sixteen, x0, x1) == (k16 // 4, k16 % 4, v)
            seen_k.add(k16)
            grid, d1 = g.spawn(sixteen, key, e, d)
            assert d1 == d + 1 and grid[k16 // 4][k16 % 4] == v and sum(x != 0 for row in grid for x in row) == 1
    assert len(seen_k) >= 12
    # x1 on either side of the threshold, and the ends of x0's range
    assert g.spawn_block(sixteen, 0, 0x19999999) == (0, 0, 2)
    assert g.spawn_block(sixteen, 0, 0x1999999A) == (0, 0, 1)
    assert g.spawn_block(sixteen, 0xFFFFFFFF, 0) == (3, 3, 2)
    assert g.spawn_block(sixteen, 0xFFFFFFFF, 0xFFFFFFFF) == (3, 3, 1)
    assert g.spawn_block(fifteen, 0xFFFFFFFF, 0xFFFFFFFF) == (3, 3, 1) and g.spawn_block(fifteen, 0x6FFFFFFF, 0)[:2] == (1, 3)
    assert g.spawn_block(CHECKERBOARD, 1, 2) is None
    fours = sum(g.block(key, 0, d)[1] < 0x1999999A for d in range(2000))
    assert 150 <= fours <= 250  # one in ten
    grid, t, d = g.reset(4, key, 1)
    assert (t, d) == (0, 6) and sum(x != 0 for row in grid for x in row) == 2
    assert grid == g.spawn(g.spawn(sixteen, key, 1, 4)[0], key, 1, 5)[0]


def test_a_no_op_consumes_no_draw_and_earns_nothing():
    key = prng.PRNGKey(1)
    for a in (g.UP, g.RIGHT, g.DOWN, 4, -1):
        assert g.step(ONLY_LEFT, 3, 11, a, key, 0, 100) == (ONLY_LEFT, 4, 11, 0.0, False)
    new, t, d, r, done = g.step(ONLY_LEFT, 3, 11, g.LEFT, key, 0, 100)
    assert (t, d, r, done) == (4, 12, 0.0, False) and sum(x != 0 for row in new for x in row) == 13
    # a no-op on the last allowed step still truncates
    assert g.step(ONLY_LEFT, 99, 11, g.UP, key, 0, 100)[1:] == (0, 13, 0.0, True)


def test_rewards_are_exact_powers_of_two():
    key = prng.PRNGKey(0)
    big = [[10, 10, 0, 0], [0] * 4, [0] * 4, [0] * 4]  # 1024 + 1024
    assert g.step(big, 0, 0, g.LEFT, key, 0, 100)[3] == 2048.0
    assert g.step(big, 0, 0, g.LEFT, key, 0, 100, reward_shift=11)[3] == 1.0
    two = [[1, 1, 0, 0], [0] * 4, [0] * 4, [0] * 4]
    assert g.step(two, 0, 0, g.LEFT, key, 0, 100, reward_shift=11)[3] == 4.0 / 2048.0
    top = [[14, 14, 14, 14], [14, 14, 14, 14], [0] * 4, [0] * 4]
    assert g.step(top, 0, 0, g.LEFT, key, 0, 100)[3] == 4 * 32768.0
    assert g.step(top, 0, 0, g.UP, key, 0, 100)[3] == 4 * 32768.0


def test_vector_reference_plays_and_meets_illegal_moves():
    """The collection test's setting on the reference alone: 8 games, episodes of 16 steps, 48 steps of a random LEGAL
    policy.  Some state must have an illegal move (else "no stored action is illegal" could pass vacuously), every
    game must finish episodes, and rewards must occur."""
    import test_gpu_collect_2048 as t
    env = g.Vector2048(t.N, t.MAX_STEPS, seed=t.SEED, reward_shift=t.SHIFT)
    rng = np.random.default_rng(0)
    env.reset()
    with_illegal = ends = 0
    total = 0.0
    for _ in range(sum(t.CALLS)):
        m = env.invalid_actions()
        with_illegal += int(m.any(1).sum())
        assert not m.all(1).any()
        a = [int(rng.choice(np.flatnonzero(row == 0))) for row in m]
        _, r, done = env.step(a)
        ends, total = ends + int(done.sum()), total + float(r.sum())
    assert with_illegal >= t.N and ends == t.N * (sum(t.CALLS) // t.MAX_STEPS) and total > 0.0


# ---------------------------------------------------------------- the ABI's Python side and the public names
def test_abi_declares_the_2048_environment():
    """(EXPORTED_SYMBOLS and the field lists against the header: tests/test_abi_cpu.py, for the whole ABI.)"""
    assert {"mzs_env_2048_reset", "mzs_env_2048_step", "mzs_env_2048_mask"} <= set(_lib.EXPORTED_SYMBOLS)
    assert len(set(_lib.EXPORTED_SYMBOLS)) == len(_lib.EXPORTED_SYMBOLS)
    fields = [n for n, _ in _lib.MzsEnv2048._fields_]
    assert fields == ["struct_size", "device", "num_envs", "max_episode_steps", "key", "reward_shift", "reserved0",
                      "board", "t", "draws", "invalid"]
    assert C.sizeof(_lib.MzsEnv2048) == 64 and _lib.MzsEnv2048.board.offset == 32
    # the other descriptors and the step arguments are as they were
    assert C.sizeof(_lib.MzsEnvCartPole) == 48 and C.sizeof(_lib.MzsEnvClassic) == 56
    assert C.sizeof(_lib.MzsEnvStepArgs) == 40
    from muax_amd import _build
    assert "mz_env2048.hip" in _build.UNITS and "mz_2048.h" in _build.UNITS["mz_env2048.hip"]


def test_public_names_and_refusals_without_a_gpu():
    cls = mx.Device2048
    assert (cls.obs_dim, cls.num_actions) == (g.OBS_DIM, g.NUM_ACTIONS) == (16, 4)
    p = inspect.signature(cls.__init__).parameters
    assert list(p)[1:] == ["n", "max_episode_steps", "seed", "reward_shift", "device"]
    assert [p[k].default for k in list(p)[2:]] == [2000, 0, 0, None]
    for name in ("reset_device", "step_device", "reset", "step", "invalid_actions_device", "invalid_actions_of",
                 "invalid_actions"):
        assert callable(getattr(cls, name))
    for bad in (dict(n=0), dict(n=2, max_episode_steps=0)):
        with pytest.raises(ValueError, match="at least 1"):
            cls(**bad)
    for shift in (-1, 12):
        with pytest.raises(ValueError, match="reward_shift"):
            cls(2, reward_shift=shift)
    with pytest.raises(ValueError, match="GPU"):
        cls(2, device="cpu")
    # the three control tasks have no mask methods: they are stepped as before
    for other in (mx.DeviceCartPole, mx.DeviceAcrobot, mx.DeviceMountainCar):
        assert not hasattr(other, "invalid_actions_device") and not hasattr(other, "invalid_actions_of")
    assert "mask_fn" in inspect.signature(mx.DeviceReplayBuffer.reanalyse).parameters
    assert inspect.signature(mx.DeviceReplayBuffer.reanalyse).parameters["mask_fn"].default is None
