"""2048 as the device environment plays it (include/mzsearch.h, "2048"), restated in plain Python on 4 x 4 lists of
exponents: no bit tricks, nothing shared with the kernel; the threefry block comes from muax_amd.prng.

A grid is a list of four rows of four exponents (0: empty, k: tile 2^k), row 0 on top.  Actions 0 up, 1 right, 2 down,
3 left; anything else changes nothing.  `Vector2048` plays N games in lock step with the host protocol of
muax_amd/vector.py and `invalid_actions()`."""
import functools

import numpy as np

from muax_amd import prng

OBS_DIM, NUM_ACTIONS = 16, 4
FOUR_BELOW = 0x1999999A  # x1 below this spawns a 4 (exponent 2): one block in ten
UP, RIGHT, DOWN, LEFT = 0, 1, 2, 3


def slide(line):
    """Four exponents slid toward index 0, equal neighbours merged once per tile from there -> (line, tiles created)."""
    out, gained = _slide(tuple(line))
    return list(out), gained


@functools.lru_cache(maxsize=None)  # (at most 16^4 lines: the tests step tens of thousands of boards)
def _slide(line):
    tiles = [v for v in line if v]
    out, gained, i = [], 0, 0
    while i < len(tiles):
        if i + 1 < len(tiles) and tiles[i] == tiles[i + 1] and tiles[i] != 15:
            out.append(tiles[i] + 1)
            gained += 2 ** (tiles[i] + 1)
            i += 2
        else:
            out.append(tiles[i])
            i += 1
    return tuple(out + [0] * (4 - len(out))), gained


def lines_of(a):
    """The four lines of move `a`, each as its cells (row, column) from the edge the tiles slide to."""
    if a == LEFT:
        return [[(i, c) for c in range(4)] for i in range(4)]
    if a == RIGHT:
        return [[(i, 3 - c) for c in range(4)] for i in range(4)]
    if a == UP:
        return [[(r, i) for r in range(4)] for i in range(4)]
    if a == DOWN:
        return [[(3 - r, i) for r in range(4)] for i in range(4)]
    return []


_LINES = {a: lines_of(a) for a in range(4)}


def move(grid, a):
    """(grid after move `a`, sum of the tiles its merges created); an action outside 0..3 changes nothing."""
    new, gained = [list(row) for row in grid], 0
    for cells in _LINES.get(a, []):
        line, g = _slide(tuple(grid[r][c] for r, c in cells))
        gained += g
        for (r, c), v in zip(cells, line):
            new[r][c] = v
    return new, gained


def legal(grid, a):
    return move(grid, a)[0] != [list(row) for row in grid]


def dead(grid):
    """No move changes the grid (true of the empty grid as well)."""
    return not any(legal(grid, a) for a in range(4))


def mask(grid):
    """1 where the move is illegal; a grid with no tile at all reports every move as legal."""
    if not any(v for row in grid for v in row):
        return [0, 0, 0, 0]
    return [0 if legal(grid, a) else 1 for a in range(4)]


def spawn_block(grid, x0, x1):
    """One spawn from the block (x0, x1): (row, column, exponent) or None on a full grid."""
    empty = [(r, c) for r in range(4) for c in range(4) if grid[r][c] == 0]
    if not empty:
        return None
    r, c = empty[(x0 * len(empty)) >> 32]
    return r, c, 2 if x1 < FOUR_BELOW else 1


def block(key, e, d):
    return prng._threefry_int(int(key[0]), int(key[1]), e & 0xFFFFFFFF, d & 0xFFFFFFFF)


def spawn(grid, key, e, d):
    """Spawn number d of environment e -> (grid, d + 1)."""
    new = [list(row) for row in grid]
    got = spawn_block(grid, *block(key, e, d))
    if got is not None:
        new[got[0]][got[1]] = got[2]
    return new, d + 1


def reset(d, key, e):
    """Two spawns on an empty grid -> (grid, t = 0, draws)."""
    grid, d = spawn([[0] * 4 for _ in range(4)], key, e, d)
    grid, d = spawn(grid, key, e, d)
    return grid, 0, d


def step_with_mask(grid, t, d, a, key, e, max_steps, reward_shift=0):
    """-> (grid, t, draws, reward, done, mask of the returned grid).  An illegal move is a no-op (reward 0, no spawn,
    no draw); t advances; a finished environment is reset."""
    new, gained = move(grid, a)
    if new != [list(row) for row in grid]:
        new, d = spawn(new, key, e, d)
    t += 1
    m = mask(new)
    has_tile = any(v for row in new for v in row)
    done = m == [1, 1, 1, 1] or not has_tile or t >= max_steps  # (the empty grid is dead although its mask is 0)
    if done:
        new, t, d = reset(d, key, e)
        m = mask(new)
    return new, t, d, gained / float(2 ** reward_shift), done, m


def step(grid, t, d, a, key, e, max_steps, reward_shift=0):
    """-> (grid, t, draws, reward, done)."""
    return step_with_mask(grid, t, d, a, key, e, max_steps, reward_shift)[:5]


def obs(grid):
    return [v / 16.0 for row in grid for v in row]


def pack(grid):
    """The uint64 of the ABI: nibble 4 r + c is grid[r][c]."""
    return sum(grid[r][c] << (4 * (4 * r + c)) for r in range(4) for c in range(4))


def unpack(board):
    return [[(int(board) >> (4 * (4 * r + c))) & 15 for c in range(4)] for r in range(4)]


def grid_of_obs(row):
    """exponent = rint(obs * 16) in float32, clamped to 0..15."""
    k = np.clip(np.rint(np.asarray(row, np.float32) * np.float32(16)), 0, 15).astype(int).tolist()
    return [k[4 * r:4 * r + 4] for r in range(4)]


class Vector2048:
    """N reference games in lock step: `reset()`, `step(actions)`, `invalid_actions()` as NumPy, like the host protocol
    of `muax_amd.Device2048` with the same seed."""

    def __init__(self, n, max_episode_steps=2000, seed=0, reward_shift=0):
        self.n, self.max_steps, self.reward_shift, self.key = n, max_episode_steps, reward_shift, prng.PRNGKey(seed)
        self.grids, self.t, self.draws, self.masks = [None] * n, [0] * n, [0] * n, [None] * n

    def load(self, boards, t=None, draws=None):
        """Start from uploaded boards (uint64 of the ABI) instead of a reset."""
        self.grids = [unpack(b) for b in boards]
        self.masks = [mask(g) for g in self.grids]
        self.t = [0] * self.n if t is None else [int(x) for x in t]
        self.draws = [0] * self.n if draws is None else [int(x) for x in draws]

    def reset(self):
        for e in range(self.n):
            self.grids[e], self.t[e], self.draws[e] = reset(self.draws[e], self.key, e)
            self.masks[e] = mask(self.grids[e])
        return self.obs()

    def step(self, actions):
        r, done = np.zeros(self.n), np.zeros(self.n, bool)
        for e in range(self.n):
            self.grids[e], self.t[e], self.draws[e], r[e], done[e], self.masks[e] = step_with_mask(
                self.grids[e], self.t[e], self.draws[e], int(actions[e]), self.key, e, self.max_steps, self.reward_shift)
        return self.obs(), r, done

    def obs(self):
        return np.array([obs(g) for g in self.grids], np.float32)

    def invalid_actions(self):
        return np.array(self.masks, np.uint8)

    def boards(self):
        return np.array([pack(g) for g in self.grids], np.uint64)
