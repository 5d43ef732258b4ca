"""Host-side tests of the wide fused training step (17 to 64 actions; muax_amd/csrc/mz_train.cuh built with
-DMZ_TRAIN_WIDE=1 through muax_amd/_jit.py::ensure_wide_train_instance): the translation unit cross-compiles for
gfx950 at every policy-head slot count, its side library names the shape and argument layout it was built for, the
narrow build still refuses more than 16 actions, and the two ensure functions keep to their own limits.  No GPU."""
import ctypes
import os
import re
import subprocess

import pytest

from muax_amd import _build, _jit

JIT_UNIT = os.path.join(_build.CSRC, "mz_train_jit.hip")
WIDE = ["-DMZ_TRAIN_WIDE=1"]


def _hipcc():
    try:
        return _build.hipcc()
    except RuntimeError:
        pytest.skip("no hipcc")


def _cmd(cc, A, E, F, out, defines):
    return [cc] + _build.FLAGS + [f"-DMZ_TRAIN_A={A}", f"-DMZ_TRAIN_E={E}", f"-DMZ_TRAIN_F={F}"] + list(defines) + \
        ["-shared", JIT_UNIT, "-o", str(out)]


def test_wide_instances_cross_compile_and_name_their_shape(tmp_path):
    """(18, 8, 21), (33, 16, 21) and (64, 64, 63): two, three and four policy-head slots, the last with every slot
    count at its largest.  Each side library reports the requested shape and the library's own argument-layout value.
    The largest one is also compiled with the compiler's resource summary: its register counts are printed, and it
    has no spilled register and no scratch memory."""
    cc = _hipcc()
    shapes = [(18, 8, 21), (33, 16, 21), (64, 64, 63)]
    procs = []
    for A, E, F in shapes:
        extra = ["-Rpass-analysis=kernel-resource-usage"] if (A, E, F) == shapes[-1] else []
        cmd = _cmd(cc, A, E, F, tmp_path / f"wide_{A}_{E}_{F}.so", WIDE + extra)
        procs.append(((A, E, F), subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    logs = {}
    for shape, p in procs:
        logs[shape], _ = p.communicate(timeout=600)
        assert p.returncode == 0, (shape, logs[shape][-1500:])
    L = ctypes.CDLL(_build.build())
    for A, E, F in shapes:
        side = ctypes.CDLL(str(tmp_path / f"wide_{A}_{E}_{F}.so"))
        a, e, f = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        side.mzs_jit_train_shape(ctypes.byref(a), ctypes.byref(e), ctypes.byref(f))
        assert (a.value, e.value, f.value) == (A, E, F) and side.mzs_jit_train_launch
        assert side.mzs_jit_train_abi() == L.mzs_train_jit_abi()
    # the resource summary of mz_train_kernel<TrainCfg<64, 64, 63>>: about 40 accumulator tiles, and nothing in scratch
    lines = logs[shapes[-1]].splitlines()
    start = next(i for i, ln in enumerate(lines) if "Function Name" in ln and "mz_train_kernel" in ln)
    end = next((i for i in range(start + 1, len(lines)) if "Function Name" in lines[i]), len(lines))
    got = {}
    for ln in lines[start:end]:
        m = re.search(r"remark:\s+(?:\S+:\d+:\d+:\s+)?([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass", ln)
        if m:
            got[m.group(1)] = int(m.group(2))
    print(f"[(64, 64, 63) wide: {got}]", end=" ")
    assert {"VGPRs", "AGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize"} <= set(got), lines[start:end]
    assert got["VGPRs Spill"] == 0 and got["SGPRs Spill"] == 0 and got["ScratchSize"] == 0, got
    assert got["VGPRs"] + got["AGPRs"] <= 512, got  # one wavefront per SIMD under __launch_bounds__(256)


def test_narrow_build_still_refuses_more_than_16_actions(tmp_path):
    cc = _hipcc()
    p = subprocess.run(_cmd(cc, 18, 8, 21, tmp_path / "narrow.so", []), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert p.returncode != 0 and "policy head in one slot" in p.stdout
    assert not (tmp_path / "narrow.so").exists()
    # ... and the wide build has a limit of its own
    p = subprocess.run(_cmd(cc, 65, 8, 21, tmp_path / "wide65.so", WIDE), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode != 0 and "policy head in at most four slots" in p.stdout


def test_ensure_functions_keep_to_their_limits(monkeypatch):
    monkeypatch.delenv("MUAX_AMD_JIT", raising=False)
    monkeypatch.delenv("MUAX_AMD_WIDE", raising=False)
    assert list(_jit.WIDE_TRAIN_DEFINES) == WIDE
    assert not _jit.ensure_train_instance(17, 8, 21)
    for shape in ((16, 8, 21), (65, 8, 21), (18, 65, 21), (18, 0, 21), (18, 8, 65), (18, 8, 15)):
        assert not _jit.ensure_wide_train_instance(*shape), shape


@pytest.mark.parametrize("var", ["MUAX_AMD_JIT", "MUAX_AMD_WIDE"])
def test_switches_turn_the_wide_instances_off(monkeypatch, var):
    """Checked before anything is compiled or loaded: no compiler is started, no file is written."""
    def boom(*a, **k):
        raise AssertionError("the compiler was looked for")
    monkeypatch.setattr(_build, "hipcc", boom)
    monkeypatch.setattr(_jit, "_loaded", {("train_wide", 18, 8, 21): object()})  # even a loaded instance is not offered
    monkeypatch.setenv(var, "0")
    for shape in ((18, 8, 21), (33, 16, 21), (64, 64, 63)):
        assert not _jit.ensure_wide_train_instance(*shape)
    if var == "MUAX_AMD_WIDE":  # the act side's switch leaves the narrow training instances alone
        monkeypatch.setattr(_jit, "_loaded", {("train", 5, 12, 25): object()})
        assert _jit.ensure_train_instance(5, 12, 25)


def test_wide_and_narrow_instances_have_their_own_cache_files(monkeypatch, tmp_path):
    """The two functions share the build / lock / load code; what differs is the file prefix and the define."""
    seen = []

    def fake_compiler(cmd, log, verbose):
        seen.append(cmd)
        return False  # (a failed build: nothing is loaded, the shape is remembered as failed)
    monkeypatch.delenv("MUAX_AMD_JIT", raising=False)
    monkeypatch.delenv("MUAX_AMD_WIDE", raising=False)
    monkeypatch.setattr(_jit, "JIT_DIR", str(tmp_path))
    monkeypatch.setattr(_jit, "_run_compiler", fake_compiler)
    monkeypatch.setattr(_build, "hipcc", lambda: "hipcc")
    monkeypatch.setattr(_jit, "_failed", set())
    monkeypatch.setattr(_jit, "_loaded", {})
    assert not _jit.ensure_wide_train_instance(18, 8, 21) and not _jit.ensure_train_instance(5, 8, 21)
    wide, narrow = seen
    assert "-DMZ_TRAIN_WIDE=1" in wide and "-DMZ_TRAIN_A=18" in wide and not any("MZ_TRAIN_WIDE" in x for x in narrow)
    assert os.path.basename(wide[-1]).startswith("mztrainwide_a18_e8_f21-")
    assert os.path.basename(narrow[-1]).startswith("mztrain_a5_e8_f21-")
    assert not _jit.ensure_wide_train_instance(18, 8, 21) and len(seen) == 2  # a failed shape is not built again
