"""GPU tests of the two plan kernels (muax_amd/csrc/mz_replay.cuh: replay_plan_count_kernel, replay_plan_emit_kernel)
through the C ABI alone (tests/plan_abi.py: guarded buffers), against the plain-loop reference tests/plan_reference.py.
Everything the call writes -- ep, ret, counts, open_len, open_ret -- is integer arithmetic or fp64 additions in a
stated order, so every comparison is bit for bit.

Shapes, the smallest that cross each boundary: N of 1, 63, 64, 65 (a wavefront's edge), 257 (one past the 256-thread
workgroup: the scan's carry into a second workgroup) and 1025 (five workgroups); T of 1, 2, 64, 65.  Two layouts of a
ring of 2 T + 3 rows: "behind" starts at row 1 with carried episodes of up to 3 steps, so their first rows lie behind
row 0, and neither call wraps; "wrap" starts max(1, T // 2) rows before the ring's end, so the first call's rows wrap
(T >= 2).  Every case is two consecutive calls that carry open_len / open_ret, the first with min_length 3, the second
with 1; the rewards and the carried returns are general doubles, so the order of the additions shows; ring rows outside
a call hold the pattern (non-zero flags; the rewards' pattern is a NaN with a payload, replay_abi._PATTERN), so a row
read out of turn shows too."""
import numpy as np
import pytest

import plan_reference as plan
from muax_amd import _lib
from plan_abi import Plan

pytestmark = pytest.mark.gpu
NS = (1, 63, 64, 65, 257, 1025)
TS = (1, 2, 64, 65)
FLAGS = ("none", "all", "random", "last", "first")
ABOVE = 10 ** 6  # a min_length above every length


def _flags(kind, T, N, rng):
    D = np.zeros((T, N), np.uint8)
    if kind == "all":
        D[:] = 1
    elif kind == "random":
        D[:] = (rng.random((T, N)) < 0.3) * rng.integers(1, 256, (T, N))  # any non-zero byte is a flag
    elif kind == "last":
        D[-1] = 1
    elif kind == "first":
        D[0] = 1
    return D


def _u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _run(rig, row0, T, min_length, D, R, max_out=None):
    """Write the call's rows, run it, hold every output against the reference.  Returns the reference's counts."""
    S, N = rig.S, rig.N
    rows = (row0 + np.arange(T)) % S
    done, r = rig.host("done").reshape(S, N).copy(), rig.host("r").reshape(S, N).copy()
    done[rows], r[rows] = D, R
    rig.put("done", done), rig.put("r", r)
    open_len, open_ret = rig.host("open_len").tolist(), rig.host("open_ret").tolist()
    ep, ret, counts, new_len, new_ret = plan.plan_steps(done.tolist(), r.tolist(), row0, T, S, open_len, open_ret,
                                                        min_length)
    assert rig.call(rig.args(row0, T, min_length, max_out)) == _lib.MZS_OK
    assert rig.host("counts").tolist() == counts
    shown = min(counts[0], rig.out_rows if max_out is None else max_out)
    assert np.array_equal(rig.host("ep")[:shown], np.array(ep[:shown], np.int32).reshape(shown, 4))
    assert np.array_equal(_u64(rig.host("ret")[:shown]), _u64(ret[:shown]))
    assert rig.host("open_len").tolist() == new_len
    assert np.array_equal(_u64(rig.host("open_ret")), _u64(new_ret))
    return counts


@pytest.mark.parametrize("layout", ["behind", "wrap"])
@pytest.mark.parametrize("kind", FLAGS)
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("N", NS)
def test_two_calls_equal_the_reference(N, T, kind, layout):
    rng = np.random.default_rng(100000 * N + 100 * T + FLAGS.index(kind))
    S = 2 * T + 3
    rig = Plan(S, N, N * T)
    carried = rng.integers(0, 4, N)
    carried[0] = 3
    row0 = 1 if layout == "behind" else S - max(1, T // 2)
    rig.put("open_len", carried)
    rig.put("open_ret", np.where(carried > 0, rng.uniform(-2, 3, N), 0.0))
    total = 0
    for min_length in (3, 1):
        counts = _run(rig, row0, T, min_length, _flags(kind, T, N, rng), rng.uniform(-2, 3, (T, N)))
        total += counts[0]
        row0 = (row0 + T) % S
    assert total == {"none": 0, "all": 2 * N * T, "last": 2 * N, "first": 2 * N}.get(kind, total)


@pytest.mark.parametrize("kind", FLAGS)
@pytest.mark.parametrize("N,T", [(1, 1), (65, 2), (257, 65)])
def test_min_length_above_every_length_drops_everything(N, T, kind):
    rng = np.random.default_rng(7 * N + T)
    rig = Plan(2 * T + 3, N, N * T)
    rig.put("open_len", np.zeros(N)), rig.put("open_ret", np.zeros(N))
    counts = _run(rig, 2, T, ABOVE, _flags(kind, T, N, rng), rng.uniform(-2, 3, (T, N)))
    assert counts[1] == 0
    if counts[0]:
        assert not rig.host("ep")[:counts[0], 3].any()


def test_max_out_below_the_total_leaves_the_rows_beyond_it():
    """325 episodes into 100 rows: counts reports 325 and the stored total, rows 100.. keep the pattern (plan_abi checks
    every row at or beyond min(counts[0], max_out) bit for bit), and the carried state is that of the whole walk."""
    N, T = 65, 5
    rng = np.random.default_rng(3)
    rig = Plan(2 * T + 3, N, N * T)
    rig.put("open_len", rng.integers(0, 3, N)), rig.put("open_ret", rng.uniform(-1, 1, N))
    counts = _run(rig, 9, T, 2, _flags("all", T, N, rng), rng.uniform(-2, 3, (T, N)), max_out=100)
    assert counts[0] == N * T and 0 < counts[1] < counts[0]
    assert (rig.host("ep")[100:] == 0x5A5A5A5A).all()


def _bad_cases():
    def field(name, value):
        return lambda a, ring: setattr(a, name, value)

    def rfield(name, value):
        return lambda a, ring: setattr(ring, name, value)

    cases = [("struct_size", field("struct_size", 8), "size"), ("ring struct_size", rfield("struct_size", 8), "size"),
             ("row0 negative", field("row0", -1), "row0"), ("row0 at ring_steps", field("row0", 13), "row0"),
             ("steps zero", field("steps", 0), "steps"), ("steps above ring_steps", field("steps", 14), "steps"),
             ("min_length zero", field("min_length", 0), "min_length"), ("max_out zero", field("max_out", 0), "max_out"),
             ("ring_steps zero", rfield("ring_steps", 0), "ring_steps"), ("num_envs zero", rfield("num_envs", 0), "num_envs"),
             ("obs_dim negative", rfield("obs_dim", -1), "obs_dim"), ("num_actions zero", rfield("num_actions", 0), "num_actions"),
             ("ring r null", rfield("r", None), "ring pointer")]
    cases += [(f"{n} null", field(n, None), n) for n in ("done", "open_len", "open_ret", "ep", "ret", "counts", "scratch")]
    return cases


@pytest.mark.parametrize("name,mutate,word", _bad_cases(), ids=[c[0] for c in _bad_cases()])
def test_bad_arguments_are_refused_before_any_launch(name, mutate, word):
    rig = Plan(13, 5, 20)
    a = rig.args(2, 4, 1)
    ring = _lib.MzsReplayRing.from_buffer_copy(rig.ring)
    mutate(a, ring)
    assert rig.call(a, ring) == _lib.MZS_E_INVALID  # (Plan.call has checked that not one byte changed)
    msg = rig.L.mzs_last_error(None).decode()
    assert "mzs_replay_plan_steps" in msg and word in msg, msg


def test_too_many_episode_rows_are_refused():
    """num_envs * steps >= 2^31 is refused on the numbers alone: nothing of that size is allocated or read."""
    rig = Plan(13, 5, 20)
    a = rig.args(0, 2 ** 16, 1)
    ring = _lib.MzsReplayRing.from_buffer_copy(rig.ring)
    ring.ring_steps, ring.num_envs = 2 ** 16, 2 ** 15
    assert rig.call(a, ring) == _lib.MZS_E_INVALID
    assert "2^31" in rig.L.mzs_last_error(None).decode()
    assert rig.call(None) == _lib.MZS_E_INVALID and rig.call(rig.args(0, 1, 1), False) == _lib.MZS_E_INVALID
