"""On-demand instances of the stochastic family's fused training step, without a GPU: _jit.stochastic_train_plan's limits
and arithmetic, one small instance cross-compiled and held against the plan through its own queries, the scratch figure
taken from the build, the MUAX_AMD_JIT=0 switch, and the two corner shapes of the lane limits."""
import ctypes as C

import pytest

from muax_amd import _jit, _lib

SMALL = (2, 3, 5, 17, 33)  # (A, C, E, F, obs_dim): cap 64


def test_plan_limits():
    plan = _jit.stochastic_train_plan
    assert plan(4, 32, 32, 63, 16) is not None
    for bad in ((0, 4, 8, 21, 4), (17, 4, 8, 21, 4), (4, 0, 8, 21, 4), (4, 61, 8, 21, 4), (16, 49, 8, 21, 4),
                (4, 4, 0, 21, 4), (4, 4, 65, 21, 4), (4, 4, 8, 16, 4), (4, 4, 8, 64, 4), (4, 4, 8, 21, 0), (4, 4, 8, 21, 129)):
        assert plan(*bad) is None, bad
    for good in ((1, 1, 1, 17, 1), (16, 48, 8, 21, 4), (4, 60, 8, 21, 4), (4, 4, 64, 17, 4), (4, 4, 8, 63, 128)):
        assert plan(*good) is not None, good
    # beyond the tile budget of the register file: named by the plan, not left to the build
    assert _jit.stochastic_train_tiles(16, 48, 64, 63, 128) > _jit.STOCH_TRAIN_MAX_TILES
    assert _jit.stochastic_train_tiles(4, 32, 32, 63, 32) == 42


def test_plan_rounds_the_cap_and_the_unroll_shrinks_with_it():
    plan = _jit.stochastic_train_plan
    caps = {od: plan(4, 17, 8, 17, od) for od in (1, 32, 33, 64, 65, 96, 97, 128, 129)}
    assert [caps[od] and caps[od][0] for od in (1, 32, 33, 64, 65, 96, 97, 128)] == [32, 32, 64, 64, 96, 96, 128, 128]
    assert caps[129] is None
    words = [caps[od][1] for od in (32, 64, 96, 128)]
    assert [b - a for a, b in zip(words, words[1:])] == [32 * 17] * 3  # 32 more rows of the encoder's [obs][17] block
    unroll = [plan(4, 32, 64, 63, od)[2] if plan(4, 32, 64, 63, od) else None for od in (32, 64, 96, 128)]
    wide = [plan(4, 17, 8, 17, od)[2] for od in (32, 64, 96, 128)]
    assert all(a >= b for a, b in zip(wide, wide[1:])) and wide[0] > wide[-1], (wide, unroll)
    # StochTrainCfg<4, 32, 32, 63>: the listed instance's figures (MAX_UNROLL = (40960 - words) / 1040)
    cap, w, mu = plan(4, 32, 32, 63, 16)
    assert cap == 32 and mu == (40960 - w) // (2 * 16 * 16 * 2 + 16) and w % 4 == 0


def test_a_small_instance_agrees_with_the_plan_and_has_no_scratch():
    L = _lib.load()
    A, Cn, E, F, od = SMALL
    assert _jit.ensure_stochastic_train_instance(*SMALL), _jit.build_log_tail()
    assert _jit.ensure_stochastic_train_instance(*SMALL)  # (cached in the process)
    cap, words, max_unroll = _jit.stochastic_train_plan(*SMALL)
    assert cap == 64
    side = _jit._loaded["stoch_train", A, Cn, E, F, cap]
    got = tuple(C.c_int32() for _ in range(5))
    side.mzs_jit_stoch_train_shape(*(C.byref(x) for x in got))
    assert tuple(x.value for x in got) == (A, Cn, E, F, cap)
    assert side.mzs_jit_stoch_train_abi() == L.mzs_stochastic_train_jit_abi() != L.mzs_train_jit_abi()
    out = (C.c_int32 * 3)()
    side.mzs_jit_stoch_train_plan(out)
    assert (out[0], out[2]) == (words, max_unroll) and out[1] == 2 * 16 * 16 * 1 + 16
    info = _jit.stochastic_train_instance_info(*SMALL)
    assert info["scratch_bytes"] == 0 and info["vgprs"] <= 256 and info["agprs"] <= 256
    assert info["max_unroll"] == max_unroll and info["lds_bytes"] <= 160 * 1024 and info["obs_cap"] == 64
    # registration: another ABI word, a null launcher and a cap that is none of the four are refused
    fn = C.cast(side.mzs_jit_stoch_train_launch, C.c_void_p)
    abi = L.mzs_stochastic_train_jit_abi()
    assert L.mzs_register_stochastic_train_dispatch(fn, A, Cn, E, F, cap, abi + 1) != 0
    assert L.mzs_register_stochastic_train_dispatch(None, A, Cn, E, F, cap, abi) != 0
    assert L.mzs_register_stochastic_train_dispatch(fn, A, Cn, E, F, 48, abi) != 0
    assert L.mzs_register_stochastic_train_dispatch(fn, A, Cn, E, F, cap, abi) == 0  # (registered already: a no-op)


def test_the_switch_turns_the_build_off(monkeypatch):
    monkeypatch.setenv("MUAX_AMD_JIT", "0")
    monkeypatch.setattr(_jit, "_ensure_side_library", lambda *a, **k: pytest.fail("compiled under MUAX_AMD_JIT=0"))
    assert _jit.ensure_stochastic_train_instance(2, 3, 6, 17, 33) is False
    assert _jit.ensure_train_instance(3, 9, 21) is False


def test_a_build_with_scratch_is_declined_from_the_compilers_own_remarks():
    remarks = ("remark: Function Name: _ZN2mz21mz_stoch_train_kernelIX [-Rpass]\nremark:     VGPRs: 256 [-Rpass]\n"
               "remark:     AGPRs: 256 [-Rpass]\nremark:     ScratchSize [bytes/lane]: 72 [-Rpass]\n"
               "remark:     LDS Size [bytes/block]: 0 [-Rpass]\n")
    assert _jit.parse_resource_usage(remarks, "mz_stoch_train_kernel") == dict(vgprs=256, agprs=256, scratch_bytes=72, lds_bytes=0)
    assert "72 bytes of scratch" in _jit._no_scratch(remarks)
    assert _jit._no_scratch(remarks.replace(": 72", ": 0")) is None
    assert "no resource usage" in _jit._no_scratch("")


@pytest.mark.parametrize("corner", [(16, 48, 64, 63, 128), (1, 63, 64, 63, 128)])
def test_corner_shapes_build_without_scratch_or_are_declined_by_the_plan(corner):
    """What the plan promises, no more: a corner of the lane limits is either declined by stochastic_train_plan (then
    nothing is built or registered) or its instance builds without scratch."""
    if _jit.stochastic_train_plan(*corner) is None:
        assert _jit.ensure_stochastic_train_instance(*corner) is False
        assert _jit.stochastic_train_instance_info(*corner) is None
    else:
        assert _jit.ensure_stochastic_train_instance(*corner), _jit.build_log_tail()
        assert _jit.stochastic_train_instance_info(*corner)["scratch_bytes"] == 0
