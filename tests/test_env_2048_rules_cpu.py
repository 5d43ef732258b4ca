"""The rules header the 2048 kernels are made of (muax_amd/csrc/mz_2048.h: transpose, mirror, slide and merge, legality,
masks, spawn) under the HOST compiler, against tests/game2048_reference.py -- the same text the device runs, checked
before a GPU is involved.  tests/rules2048_main.cpp is built with -fsanitize=address,undefined (the runtime is linked
into that program only) and run as a child process; every printed integer must equal the reference's."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import game2048_reference as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("rules2048") / "rules2048_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "muax_amd", "csrc"), os.path.join(ROOT, "tests", "rules2048_main.cpp"),
                           "-o", exe])

    def run(rows):
        """rows: (board, action, x0, x1) -> one list of eight ints per row"""
        text = "".join(f"{b} {a} {x0} {x1}\n" for b, a, x0, x1 in rows)
        p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]  # (a sanitizer report goes to stderr)
        lines = p.stdout.splitlines()
        assert len(lines) == len(rows)
        return [[int(w) for w in line.split()] for line in lines]
    return run


def _boards():
    """Sparse, half-full, full and high-exponent boards, the hand-made edge boards, and every direction and some
    out-of-range actions for each."""
    rng = np.random.default_rng(7)
    grids = []
    for fill, top in ((0.15, 3), (0.5, 3), (0.8, 2), (1.0, 2), (1.0, 3), (0.7, 15), (1.0, 15)):
        for _ in range(60):
            cells = np.where(rng.random(16) < fill, rng.integers(1, top + 1, 16), 0)
            grids.append(cells.reshape(4, 4).tolist())
    grids += [[[0] * 4 for _ in range(4)], [[15] * 4 for _ in range(4)], [[14] * 4 for _ in range(4)],
              [[1, 2, 1, 2], [2, 1, 2, 1], [1, 2, 1, 2], [2, 1, 2, 1]],
              [[0, 1, 2, 3], [0, 2, 3, 4], [0, 3, 4, 5], [0, 4, 5, 6]],
              [[1, 1, 1, 1], [1, 1, 2, 0], [2, 0, 2, 2], [1, 0, 0, 1]],
              [[15, 15, 0, 0], [0, 15, 0, 15], [14, 14, 15, 15], [15, 14, 14, 15]]]
    rows = []
    for grid in grids:
        for a in (0, 1, 2, 3, -1, 4, 2 ** 31 - 1):
            rows.append((grid, a, int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 32))))
    for x0, x1 in ((0, 0x19999999), (0, 0x1999999A), (0xFFFFFFFF, 0), (0xFFFFFFFF, 0xFFFFFFFF)):
        rows += [(grid, 3, x0, x1) for grid in grids[:40] + grids[-7:]]
    return rows


def test_every_rule_equals_the_reference(program):
    rows = _boards()
    got = program([(g.pack(grid), a, x0, x1) for grid, a, x0, x1 in rows])
    changed = merged = full_spawn = 0
    for (grid, a, x0, x1), (moved, gained, unchanged, mask, empty, spawned, transposed, mirrored) in zip(rows, got):
        want, want_gained = g.move(grid, a)
        assert (g.unpack(moved), gained) == (want, want_gained), (grid, a)
        assert [(unchanged >> (8 * k)) & 255 for k in range(4)] == [0 if g.legal(grid, k) else 1 for k in range(4)]
        assert [(mask >> (8 * k)) & 255 for k in range(4)] == g.mask(grid), grid
        assert (unchanged == 0x01010101) is g.dead(grid)
        assert empty == sum(v == 0 for row in want for v in row)
        cell = g.spawn_block(want, x0, x1)
        after = [list(row) for row in want]
        if cell is not None:
            after[cell[0]][cell[1]] = cell[2]
        else:
            full_spawn += 1
        assert g.unpack(spawned) == after, (grid, a, x0, x1)
        assert g.unpack(transposed) == [[grid[c][r] for c in range(4)] for r in range(4)]
        assert g.unpack(mirrored) == [row[::-1] for row in grid]
        changed, merged = changed + (want != grid), merged + (gained > 0)
    assert changed > 500 and merged > 200 and full_spawn > 50  # the cases are there
