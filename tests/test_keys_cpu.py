"""The library's host integer code (muax_amd/csrc/mz_keys.h) on the CPU: the JAX threefry key walk and mctx's table of
considered visits decide every PRNG stream of every search, and are otherwise reached only through a GPU launch.

tests/keys_main.cpp includes that header and prints what it computes; here it is built with the host compiler and
-fsanitize=address,undefined (the sanitizer runtime is linked into that program only), run as a child process, and every
printed word compared -- exactly: these are integers -- with the oracle (oracle.pyoracle: split, considered_visits) and
with the independent restatement in oracle/mz_numpy.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import mz_numpy as mn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = [(0, 0), (0, 1), (0xFFFFFFFF, 0xFFFFFFFF), (0x13198A2E, 0x03707344), (2718843009, 1272950319)]
WALK_S = [1, 2, 50, 255, 256, 1023, 65534]  # 65534: the largest num_simulations mzs_create accepts
VISITS_M = [0, 1, 2, 3, 4, 16, 64]
VISITS_S = [1, 2, 5, 8, 50, 255]  # 18 pairs have S < ceil(log2 m) m (14 of them S < m): the halving loop's divisions at their floors


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("keys") / "keys_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "muax_amd", "csrc"), os.path.join(ROOT, "tests", "keys_main.cpp"),
                           "-o", exe])

    def run(commands):
        """commands: tuples (name, int...) -> one list of ints per command"""
        argv = [exe] + [str(x) for c in commands for x in c]
        p = subprocess.run(argv, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]  # (a sanitizer report goes to stderr)
        lines = p.stdout.splitlines()
        assert len(lines) == len(commands)
        return [[int(w) for w in line.split()] for line in lines]
    return run


def test_runner_reports_a_failing_child(program):
    # (an unknown command exits with status 2: the runner does tell a failing child from a passing one)
    with pytest.raises(AssertionError):
        program([("nosuch",)])


def test_split_rows(program, oracle):
    cmds = [("split", k0, k1, n, row) for k0, k1 in KEYS for n in (2, 3) for row in range(n)]
    got = program(cmds)
    for (_, k0, k1, n, row), words in zip(cmds, got):
        assert words == oracle.split([k0, k1], n)[row].tolist(), (k0, k1, n, row)


def test_gumbel_root_key(program, oracle):
    got = program([("gumbel", k0, k1) for k0, k1 in KEYS])
    for (k0, k1), words in zip(KEYS, got):
        assert words == oracle.split([k0, k1], 2)[1].tolist(), (k0, k1)


def _oracle_walk(oracle, key, S):
    """(k_sample, simulate keys [S, 2]) by the oracle's split, as pyoracle.sim_keys_from_act_key walks them (rows 0 and 1
    of every split(rng, 3) only, through preallocated buffers: 65534 simulations are 131068 calls)."""
    top = oracle.split(key, 3)
    split = oracle.lib().mzo_split
    rk = np.array(top[2], np.uint32)
    nk = np.zeros(2, np.uint32)
    sims = np.zeros((S, 2), np.uint32)
    u32p = C.POINTER(C.c_uint32)
    rkp, nkp, base = rk.ctypes.data_as(u32p), nk.ctypes.data_as(u32p), sims.ctypes.data
    three, zero, one = C.c_int64(3), C.c_int64(0), C.c_int64(1)
    for s in range(S):
        split(rkp, three, one, C.cast(base + 8 * s, u32p))
        split(rkp, three, zero, nkp)
        rk[:] = nk
    return top[0], sims


def test_key_walk(program, oracle):
    cmds = [("walk", k0, k1, S) for k0, k1 in KEYS for S in WALK_S]
    got = program(cmds)
    want = {}
    for key in KEYS:  # the walk of S simulations is the head of the walk of more: one oracle walk per key, the longest
        k_sample, sims = _oracle_walk(oracle, key, max(WALK_S))
        want[key] = (k_sample.tolist(), sims)
        ks, _, short = oracle.sim_keys_from_act_key(key, 50)  # ... whose head is pyoracle's own walk
        assert ks.tolist() == k_sample.tolist() and np.array_equal(short, sims[:50])
    for (_, k0, k1, S), words in zip(cmds, got):
        k_sample, sims = want[(k0, k1)]
        assert len(words) == 2 + 2 * S
        assert words[:2] == k_sample, (k0, k1, S)
        assert np.array_equal(np.array(words[2:], np.uint32).reshape(S, 2), sims[:S]), (k0, k1, S)


def test_considered_visits(program, oracle):
    cmds = [("visits", m, S) for m in VISITS_M for S in VISITS_S]
    got = program(cmds)
    for (_, m, S), words in zip(cmds, got):
        assert words == oracle.considered_visits(m, S).tolist(), (m, S)
        assert words == list(mn.considered_visits(m, S)), (m, S)
