"""On-demand instances of the fused act() kernel (muax_amd/csrc/mz_fused_jit.hip).

libmzsearch.so carries the (num_actions, embedding_dim, support slots, tree size) instances listed in
muax_amd/csrc/mz_instances.def; the reference's act() takes ANY num_simulations / network widths (muax/model.py:82-96,
muax/nn.py:59-115).  When mzs_act_mlp has no instance for a shape and a hipcc is present, `ensure_instance` compiles one
translation unit for that shape (~25 s, once: cached as muax_amd/lib/jit/<shape>-<source hash>.so), loads it and registers
it with the library (mzs_register_fused_dispatch) -- the shape then runs as ONE launch per act() like a listed one, same
kernel source, same bits.  Shapes outside the kernel's own limits (more than 16 actions, more than 255 simulations,
embeddings wider than 64) cannot be instantiated: they take the one-launch generic search (mzs_mlp_search) or the
step-wise path.  MUAX_AMD_JIT=0 turns the on-demand build off.
"""
from __future__ import annotations

import ctypes as C
import ctypes as C_  # (where a function's own argument is named C: the stochastic family's chance outcomes)
import hashlib
import os
import subprocess

from . import _build

JIT_DIR = os.path.join(_build.LIB_DIR, "jit")
_SOURCES = ["mz_fused_jit.hip", "mz_fused_group.inc", "mz_fused_launch.h", "mz_fused.cuh", "mz_spec.cuh", "mz_host.h"]
_loaded = {}   # shape -> CDLL (kept alive: the library calls into it)
_failed = set()
_TRAIN_SOURCES = ["mz_train_jit.hip", "mz_train_launch.h", "mz_train.cuh", "mz_train_blocks.cuh", "mz_spec.cuh", "mz_host.h"]
# Bump when plan() changes its answer for any shape: the number is part of every cached file's name (and this file is
# hashed into it as well), so a cache directory that survives a planner change cannot serve an instance whose record
# kind / roots per workgroup differ from what the planner now says.
PLAN_VERSION = 2
last_build_log = None  # path of the compiler log of the most recent FAILED on-demand build (surfaced in MuZero's warning)


def _ceil_log2(n: int) -> int:
    return 0 if n <= 1 else 1 + _ceil_log2((n + 1) // 2)


def lds_bytes(A: int, E: int, NMAX: int, WAVES: int, long_paths: bool = False, gumbel: bool = True) -> int:
    """FusedCfg::LDS_BYTES of a plain (non-compact) instance -- mz_fused.cuh -- for the widest record the instance is
    compiled with: `gumbel` = the Gumbel modes too (five words per child: the prior logit; the raw value in the header;
    root noise behind the tree), else the MuZero policy's modes only (four words per child; round 6: an on-demand
    instance is planned per policy).  `long_paths`: FusedCfg::LONG -- root paths (and embeddings) in HBM."""
    selw = ((2 * A + 3) // 4) * 4
    st0 = selw + (4 if (gumbel or not long_paths) else 3)  # HDRW: the raw value leaves a PH_ record unless MODE 3 reads it
    path0 = st0 + (5 if gumbel else 4) * A + (E if (E <= 16 and not long_paths) else 0)  # (LONG: embeddings in HBM too)
    entry = 8 if _ceil_log2(NMAX) + max(1, _ceil_log2(A)) <= 8 else 16
    pathw = (NMAX * entry + 31) // 32
    ns = (path0 + (0 if long_paths else pathw)) | 1
    tree = ((ns * NMAX + 3) // 4) * 4 + (((A + 3) // 4) * 4 if (long_paths and gumbel) else 0)
    root = tree + ((8 - tree % 32 + 32) % 32)
    tbl = 2 * (((NMAX + 2 + 3) // 4) * 4)
    return 4 * (tbl + 4 * WAVES * root)


def plan(A: int, E: int, F: int, S: int, gumbel: bool = True):
    """(FS, NMAX, WAVES, LONG) of an instance that serves the shape, or None when the kernel's own limits rule it out:
    A <= 16 (all scores of a node in one lane's registers; four action bits per JUMP word), S <= 255 (depths are bytes).
    Up to 127 simulations the nodes' root paths may live in the LDS record; beyond -- or when that lets a workgroup
    hold more roots -- in HBM (FusedCfg::LONG).  `gumbel` False: an instance of the MuZero policy's modes only, sized for
    their four-word children (e.g. CartPole's shape at 160 simulations: 16 roots per workgroup instead of 12)."""
    if not (1 <= A <= 16 and 17 <= F <= 63 and 1 <= S <= 255):
        return None
    if E < 1 or E > 64:  # (round 5: any width up to 64; widths above 16 that are no multiple of 8 take the packed-fma
        return None      # first layers instead of the eight-input v_fmac_f32_dpp blocks)
    FS = 2 if F <= 32 else 4
    for NMAX in (51, 64, 101, 128, 161, 201, 256):
        if S + 1 > NMAX:
            continue
        entry = 8 if _ceil_log2(NMAX) + max(1, _ceil_log2(A)) <= 8 else 16
        pathw = (NMAX * entry + 31) // 32
        best = None
        for long_paths in (False, True):  # (paths in LDS are the faster record: taken unless HBM paths hold more roots)
            # (ties go to the LDS record, the faster one; the LONG record is taken where it holds more roots per workgroup)
            if (pathw + 15) // 16 > (8 if long_paths else 4) or (A > pathw and not long_paths):
                continue
            for W in (4, 3, 2, 1):
                if lds_bytes(A, E, NMAX, W, long_paths, gumbel) <= 160 * 1024:
                    if best is None or W > best[2]:
                        best = (FS, NMAX, W, long_paths)
                    break
        if best is not None:
            return best
    return None


def _source_hash() -> str:
    # everything the side library's code depends on: its sources, the ABI header, the compiler flags (they name the
    # offload arch) -- a cache directory shared across flag or header changes must not serve a stale instance
    h = hashlib.sha256()
    for f in _SOURCES + [_build._ABI]:
        with open(os.path.join(_build.CSRC, f), "rb") as fh:
            h.update(fh.read())
    with open(os.path.abspath(__file__), "rb") as fh:  # the planner and the compile recipe live here
        h.update(fh.read())
    h.update("\0".join(_build.FLAGS + _build.UNIT_FLAGS["mz_fused_g0.hip"]).encode())
    h.update(f"plan{PLAN_VERSION}".encode())
    return h.hexdigest()[:12]


def _run_compiler(cmd, log, verbose, keep_log: bool = False) -> bool:
    """hipcc with its output kept: `log` holds the command and everything the compiler said (a failed on-demand build
    used to be silent); the file stays after a failure and is removed after a success, unless `keep_log`."""
    global last_build_log
    with open(log, "w") as lf:
        lf.write(" ".join(cmd) + "\n")
        lf.flush()
        rc = subprocess.call(cmd, stdout=lf, stderr=subprocess.STDOUT)
    if verbose:
        print(open(log).read())
    if rc != 0:
        last_build_log = log
        return False
    if not keep_log:
        os.remove(log)
    return True


def build_log_tail(lines: int = 6) -> str:
    """The last lines of the most recent failed on-demand build's compiler log ('' when none failed)."""
    if not last_build_log or not os.path.exists(last_build_log):
        return ""
    with open(last_build_log, errors="replace") as f:
        return "".join(f.readlines()[-lines:]).strip()


def _compile(cc, so, tag, A, E, FS, NMAX, W, LONG, gumbel, verbose, extra_flags=()) -> bool:
    """One translation unit for one shape -> `so` (under the cache directory's file lock).  OSError propagates."""
    import fcntl
    with open(os.path.join(JIT_DIR, ".jit.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)  # ranks that miss the same shape build it once
        if os.path.exists(so):
            return True
        deff = os.path.join(JIT_DIR, f"inst_{tag}.def")
        with open(deff, "w") as f:
            f.write(f"MZS_INST(100, {A}, {E}, {FS}, {NMAX}, {W}, {'2' if LONG else 'false'})\n")
        tmp = so + f".tmp{os.getpid()}"
        cmd = [cc] + _build.FLAGS + _build.UNIT_FLAGS["mz_fused_g0.hip"] + [
            f'-DMZ_INSTANCES_FILE="{deff}"', "-DMZ_FUSED_GROUP=100", f"-DMZ_FUSED_MUZERO_ONLY={0 if gumbel else 1}"] + \
            list(extra_flags) + ["-shared", os.path.join(_build.CSRC, "mz_fused_jit.hip"), "-o", tmp]
        try:
            if not _run_compiler(cmd, os.path.join(JIT_DIR, f"mzfused_{tag}.log"), verbose):
                return False
            os.replace(tmp, so)
            return True
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)


def instance_tag(A: int, E: int, FS: int, NMAX: int, W: int, LONG: bool, gumbel: bool) -> str:
    """File tag of an on-demand instance: EVERYTHING the planner decided (record kind and policy class included) and the
    hash of everything the code depends on (sources, ABI header, flags, this file, PLAN_VERSION)."""
    return f"a{A}_e{E}_fs{FS}_n{NMAX}_w{W}_l{int(LONG)}_p{int(gumbel)}-{_source_hash()}"


def instance_file(A: int, E: int, F: int, S: int, gumbel: bool = True):
    """Path of the side library ensure_instance() would load for the shape (None when no instance can exist)."""
    if not gumbel and plan(A, E, F, S, False) == plan(A, E, F, S, True):
        gumbel = True
    pl = plan(A, E, F, S, gumbel)
    return None if pl is None else os.path.join(JIT_DIR, f"mzfused_{instance_tag(A, E, *pl, gumbel)}.so")


def ensure_instance(A: int, E: int, F: int, S: int, verbose: bool = False, gumbel: bool = True, extra_flags=()) -> bool:
    """Make sure mzs_act_mlp can serve (A, E, F, S) with one launch: True when an on-demand instance is registered
    (built now or earlier), False when the shape cannot be instantiated, there is no compiler, the build fails (its
    compiler output is then in muax_amd/lib/jit/mzfused_<tag>.log, see build_log_tail()) or MUAX_AMD_JIT=0.
    `gumbel`: the policy class the instance is planned for -- True (default): every mode, sized for the Gumbel modes'
    five-word children; False: the MuZero policy's modes only, taken where that record holds more roots per workgroup
    (where it does not, the all-modes instance is used: one file per shape).  `extra_flags`: more compiler flags (tests)."""
    if os.environ.get("MUAX_AMD_JIT", "1") == "0":
        return False
    if not gumbel and plan(A, E, F, S, False) == plan(A, E, F, S, True):
        gumbel = True  # nothing to gain from a policy-specific instance
    pl = plan(A, E, F, S, gumbel)
    if pl is None:
        return False
    FS, NMAX, W, LONG = pl
    shape = (A, E, FS, NMAX, W, bool(LONG), bool(gumbel)) + tuple(extra_flags)
    if shape in _loaded:
        return True
    if shape in _failed:
        return False
    try:
        cc = _build.hipcc()
    except RuntimeError:
        return False
    tag = instance_tag(A, E, FS, NMAX, W, LONG, gumbel)
    if extra_flags:
        tag += "-x" + hashlib.sha256("\0".join(extra_flags).encode()).hexdigest()[:6]
    so = os.path.join(JIT_DIR, f"mzfused_{tag}.so")
    try:  # a read-only install (no cache directory, no lock file) is "no instance", not an exception out of act()
        os.makedirs(JIT_DIR, exist_ok=True)
        if not os.path.exists(so) and not _compile(cc, so, tag, A, E, FS, NMAX, W, LONG, gumbel, verbose, extra_flags):
            _failed.add(shape)
            return False
    except OSError:
        _failed.add(shape)
        return False
    from . import _lib
    L = _lib.load()
    side = C.CDLL(so)
    side.mzs_jit_dispatch.restype = C.c_void_p
    side.mzs_jit_abi.restype = C.c_int
    register = L.mzs_register_fused_dispatch if gumbel else L.mzs_register_fused_dispatch_muzero
    _lib.check(register(C.c_void_p(side.mzs_jit_dispatch()), side.mzs_jit_abi()))
    _loaded[shape] = side
    return True


def _train_hash(sources=None, salt: str = "") -> str:
    h = hashlib.sha256()
    for f in (_TRAIN_SOURCES if sources is None else sources) + [_build._ABI]:
        with open(os.path.join(_build.CSRC, f), "rb") as fh:
            h.update(fh.read())
    with open(os.path.abspath(__file__), "rb") as fh:
        h.update(fh.read())
    h.update("\0".join(_build.FLAGS).encode())
    h.update(salt.encode())
    return h.hexdigest()[:12]


def _ensure_side_library(shape, so, unit, defines, verbose, accept=None) -> bool:
    """THE body of every on-demand training instance: build `unit` with `defines` into `so` once (under the cache
    directory's file lock, through a temporary file), compiler output in the .log beside it.  `shape`: the key in
    _loaded / _failed.  `accept(log_text)`: called on the compiler's output of a build that succeeded; a string is a
    reason to decline the instance -- it is written to the log, which then stays, nothing is installed and the answer is
    False.  True when `so` exists afterwards; False (shape noted in _failed) without a compiler, without a writable cache
    directory, or when the build fails or is declined."""
    global last_build_log
    try:
        cc = _build.hipcc()
    except RuntimeError:
        return False
    try:
        os.makedirs(JIT_DIR, exist_ok=True)
        if not os.path.exists(so):
            import fcntl
            with open(os.path.join(JIT_DIR, ".jit.lock"), "w") as lock:
                fcntl.flock(lock, fcntl.LOCK_EX)  # ranks that miss the same shape build it once
                if not os.path.exists(so):
                    tmp = so + f".tmp{os.getpid()}"
                    log = so[:-3] + ".log"
                    cmd = [cc] + _build.FLAGS + list(defines) + ["-shared", os.path.join(_build.CSRC, unit), "-o", tmp]
                    try:
                        if accept is None:
                            ok = _run_compiler(cmd, log, verbose)
                        else:
                            ok = _run_compiler(cmd, log, verbose, keep_log=True)
                            if ok:
                                with open(log, errors="replace") as f:
                                    why = accept(f.read())
                                if why:
                                    with open(log, "a") as f:
                                        f.write(f"\nnot registered: {why}\n")
                                    last_build_log, ok = log, False
                        if not ok:
                            _failed.add(shape)
                            return False
                        os.replace(tmp, so)
                    finally:
                        if os.path.exists(tmp):
                            os.remove(tmp)
    except OSError:
        _failed.add(shape)
        return False
    return True


def _ensure_train(kind: str, prefix: str, defines, A: int, E: int, F: int, verbose: bool) -> bool:
    """Build (once: cached as muax_amd/lib/jit/<prefix>_<shape>-<source hash>.so), load and register one instance of the
    fused training-step kernel, muax_amd/csrc/mz_train_jit.hip compiled with `defines` on top of the shape's; the
    caller has checked the shape against its limits.  False when there is no compiler, no writable cache directory, or
    the build fails (compiler output in the .log beside the file, see build_log_tail())."""
    shape = (kind, A, E, F)  # key in _loaded / _failed: ("train", ...) narrow, ("train_wide", ...) wide
    if shape in _loaded:
        return True
    if shape in _failed:
        return False
    so = os.path.join(JIT_DIR, f"{prefix}_a{A}_e{E}_f{F}-{_train_hash()}.so")
    if not _ensure_side_library(shape, so, "mz_train_jit.hip",
                                [f"-DMZ_TRAIN_A={A}", f"-DMZ_TRAIN_E={E}", f"-DMZ_TRAIN_F={F}"] + list(defines), verbose):
        return False
    from . import _lib
    L = _lib.load()
    side = C.CDLL(so)
    side.mzs_jit_train_abi.restype = C.c_int
    got = (C.c_int32(), C.c_int32(), C.c_int32())
    side.mzs_jit_train_shape(*(C.byref(x) for x in got))
    if tuple(x.value for x in got) != (A, E, F):  # the file name said (A, E, F); the code inside must agree
        raise RuntimeError(f"{so}: built for shape {tuple(x.value for x in got)}, asked for {(A, E, F)}")
    fn = C.cast(side.mzs_jit_train_launch, C.c_void_p)
    _lib.check(L.mzs_register_train_dispatch(fn, A, E, F, side.mzs_jit_train_abi()))
    _loaded[shape] = side
    return True


def ensure_train_instance(A: int, E: int, F: int, verbose: bool = False) -> bool:
    """Make sure mzs_mlp_loss_grad can serve (num_actions, embedding_dim, F = 2 support_size + 1): True when an on-demand
    instance of the fused training-step kernel (muax_amd/csrc/mz_train_jit.hip) is registered -- built now (one
    translation unit, cached as muax_amd/lib/jit/mztrain_<shape>-<source hash>.so) or earlier --, False when the shape is
    outside the kernel's limits (more than 16 actions, embeddings wider than 64, F outside 17..63), there is no compiler,
    the build fails, or MUAX_AMD_JIT=0.  Round 5: a model whose act() runs on an on-demand instance keeps the fused
    update() too (the reference's update() takes any widths, muax/model.py:181-201).  17 to 64 actions:
    ensure_wide_train_instance."""
    if os.environ.get("MUAX_AMD_JIT", "1") == "0":
        return False
    if not (1 <= A <= 16 and 1 <= E <= 64 and 17 <= F <= 63):
        return False
    return _ensure_train("train", "mztrain", (), A, E, F, verbose)


WIDE_TRAIN_DEFINES = ("-DMZ_TRAIN_WIDE=1",)


def ensure_wide_train_instance(A: int, E: int, F: int, verbose: bool = False) -> bool:
    """ensure_train_instance for 17 <= num_actions <= 64 (1 <= E <= 64, 17 <= F <= 63 as there): the same translation
    unit compiled with -DMZ_TRAIN_WIDE=1, which spreads the policy head over ceil(A / 16) lane slots and re-reads the
    weights from LDS in every unroll step (mz_train.cuh); cached as muax_amd/lib/jit/mztrainwide_<shape>-<source
    hash>.so.  False outside those limits, without a compiler, when the build fails, under MUAX_AMD_JIT=0, and under
    MUAX_AMD_WIDE=0 (the switch that also keeps act() off the wide-action kernel)."""
    if os.environ.get("MUAX_AMD_JIT", "1") == "0" or os.environ.get("MUAX_AMD_WIDE", "1") == "0":
        return False
    if not (17 <= A <= 64 and 1 <= E <= 64 and 17 <= F <= 63):
        return False
    return _ensure_train("train_wide", "mztrainwide", WIDE_TRAIN_DEFINES, A, E, F, verbose)


# ---- the stochastic family's training step (muax_amd/csrc/mz_stoch_train_jit.hip) ----
_STOCH_TRAIN_SOURCES = ["mz_stoch_train_jit.hip", "mz_train_launch.h", "mz_stoch_train.cuh", "mz_train_blocks.cuh", "mz_spec.cuh",
                        "mz_host.h"]
STOCH_TRAIN_LDS_BYTES = 160 * 1024  # mz_train_blocks.cuh: TRAIN_LDS_BYTES
# What one lane's 512 registers (256 VGPRs + 256 AGPRs, one wavefront per SIMD) leave for gradient tiles.  A 16 x 16
# tile is four registers that live through the whole backward sweep.  The listed (4, 32, 32, 63) instance has 42 tiles and
# takes 256 + 206 = 462 registers, so 294 are the rest of the kernel; 512 - 294 = 218 registers hold 54 tiles.  A shape
# beyond that cannot be built without scratch.  (Necessary, not sufficient: the build's own scratch figure decides --
# profiles/stochastic_train.txt has shapes of 37 to 48 tiles that spill.)
STOCH_TRAIN_MAX_TILES = 54
_RESOURCE_USAGE = ["-Rpass-analysis=kernel-resource-usage"]


def _slots(n: int) -> int:
    return (n + 15) // 16


def stochastic_train_tiles(A: int, C: int, E: int, F: int, obs_cap: int) -> int:
    """Number of 16 x 16 weight-gradient tiles mz_stoch_train_kernel keeps in registers across the unroll."""
    ES, FS, CS, XAS, XCS = _slots(E), _slots(F), _slots(C), _slots(E + A), _slots(E + C)
    # ad1, ad2 | av1, av2 | ac1, ac2 | cr1, cr2 | cn1, cn2 | pv1, pv2 | pp1, pp2 | en1, en2
    return XAS + ES + ES + FS + ES + CS + XCS + FS + XCS + ES + ES + FS + ES + 1 + obs_cap // 16 + CS


def stochastic_train_plan(A: int, C: int, E: int, F: int, obs_dim: int):
    """StochTrainCfg's arithmetic (muax_amd/csrc/mz_stoch_train.cuh) for an on-demand instance that serves the shape:
    (obs_cap, weight_words, max_unroll) -- obs_dim rounded up to 32 / 64 / 96 / 128, the words of LDS the weights take,
    the longest unroll the rest of the 160 KiB keeps -- or None when no instance can exist: outside 1 <= A <= 16, 1 <= C,
    A + C <= 64, 1 <= E <= 64, 17 <= F <= 63, 1 <= obs_dim <= 128; where not even L = 2 fits in LDS; beyond
    STOCH_TRAIN_MAX_TILES gradient tiles (the register file)."""
    if not (1 <= A <= 16 and 1 <= C and A + C <= 64 and 1 <= E <= 64 and 17 <= F <= 63 and 1 <= obs_dim <= 128):
        return None
    OB, H, XA, XC = 32 * ((obs_dim + 31) // 32), 16, E + A, E + C

    def blk(k, n):
        return k * (16 * _slots(n) + 1) + 16 * _slots(n)

    words = sum(blk(k, n) for k, n in ((XA, H), (H, E), (E, H), (H, F), (E, H), (H, C), (XC, H), (H, F), (XC, H), (H, E),
                                       (E, H), (H, F), (E, H), (H, A), (OB, H), (H, C)))
    words = ((words + 3) // 4) * 4
    max_unroll = (STOCH_TRAIN_LDS_BYTES // 4 - words) // (2 * 16 * 16 * _slots(E) + 16)
    if max_unroll < 2 or stochastic_train_tiles(A, C, E, F, OB) > STOCH_TRAIN_MAX_TILES:
        return None
    return OB, words, max_unroll


def parse_resource_usage(log_text: str, kernel: str):
    """The compiler's -Rpass-analysis=kernel-resource-usage remarks for the first function whose name contains `kernel`:
    {'vgprs', 'agprs', 'scratch_bytes' (per lane), 'lds_bytes' (static)}, or None when the log has no such remarks."""
    import re
    for m in re.finditer(r"Function Name: (\S+)(.*?)LDS Size \[bytes/block\]: (\d+)", log_text, re.S):
        if kernel in m.group(1):
            body = m.group(2)
            v, a, s = (re.search(p + r": (\d+)", body) for p in (r" VGPRs", r"AGPRs", r"ScratchSize \[bytes/lane\]"))
            if v and a and s:
                return {"vgprs": int(v.group(1)), "agprs": int(a.group(1)), "scratch_bytes": int(s.group(1)),
                        "lds_bytes": int(m.group(3))}
    return None


def _stochastic_train_file(A, C, E, F, OB) -> str:
    tag = _train_hash(_STOCH_TRAIN_SOURCES, "\0".join(_RESOURCE_USAGE))
    return os.path.join(JIT_DIR, f"mzstochtrain_a{A}_c{C}_e{E}_f{F}_o{OB}-{tag}.so")


def stochastic_train_instance_info(A: int, C: int, E: int, F: int, obs_dim: int):
    """Figures of the on-demand instance for the shape, from its build's own compiler remarks (kept beside the side
    library as <file>.log): {'vgprs', 'agprs', 'scratch_bytes', 'lds_bytes', 'max_unroll', 'obs_cap'} -- `lds_bytes` the
    dynamic LDS of a launch at max_unroll -- or None when the plan declines the shape or nothing has been built."""
    pl = stochastic_train_plan(A, C, E, F, obs_dim)
    if pl is None:
        return None
    OB, words, max_unroll = pl
    log = _stochastic_train_file(A, C, E, F, OB)[:-3] + ".log"
    if not os.path.exists(log):
        return None
    with open(log, errors="replace") as f:
        info = parse_resource_usage(f.read(), "mz_stoch_train_kernel")
    if info is None:
        return None
    info.update(max_unroll=max_unroll, obs_cap=OB, lds_bytes=4 * (words + max_unroll * (2 * 16 * 16 * _slots(E) + 16)))
    return info


def _no_scratch(log_text: str):
    info = parse_resource_usage(log_text, "mz_stoch_train_kernel")
    if info is None:
        return "the compiler reported no resource usage for mz_stoch_train_kernel"
    if info["scratch_bytes"]:
        return (f"the instance spills {info['scratch_bytes']} bytes of scratch per lane ({info['vgprs']} VGPRs + "
                f"{info['agprs']} AGPRs): the shape is beyond the register file")
    return None


def ensure_stochastic_train_instance(A: int, C: int, E: int, F: int, obs_dim: int, verbose: bool = False) -> bool:
    """Make sure mzs_stochastic_mlp_loss_grad can serve (num_actions, num_chance_outcomes, embedding_dim,
    F = 2 support_size + 1) with observations `obs_dim` wide: True when an on-demand instance of the stochastic family's
    fused training-step kernel (muax_amd/csrc/mz_stoch_train_jit.hip at the plan's observation cap) is registered -- built
    now (one translation unit, cached as muax_amd/lib/jit/mzstochtrain_<shape>-<source hash>.so with its compiler remarks
    in the .log beside it) or earlier.  False when stochastic_train_plan declines the shape, there is no compiler, the
    build fails, the build reports scratch (such an instance is never registered; the .log says so, build_log_tail()), or
    MUAX_AMD_JIT=0."""
    if os.environ.get("MUAX_AMD_JIT", "1") == "0":
        return False
    pl = stochastic_train_plan(A, C, E, F, obs_dim)
    if pl is None:
        return False
    OB, words, max_unroll = pl
    shape = ("stoch_train", A, C, E, F, OB)
    if shape in _loaded:
        return True
    if shape in _failed:
        return False
    so = _stochastic_train_file(A, C, E, F, OB)
    defines = [f"-DMZ_STOCH_A={A}", f"-DMZ_STOCH_C={C}", f"-DMZ_STOCH_E={E}", f"-DMZ_STOCH_F={F}", f"-DMZ_STOCH_OB={OB}"]
    if not _ensure_side_library(shape, so, "mz_stoch_train_jit.hip", defines + _RESOURCE_USAGE, verbose, accept=_no_scratch):
        return False
    from . import _lib
    L = _lib.load()
    side = C_.CDLL(so)
    side.mzs_jit_stoch_train_abi.restype = C_.c_int
    got = tuple(C_.c_int32() for _ in range(5))
    side.mzs_jit_stoch_train_shape(*(C_.byref(x) for x in got))
    if tuple(x.value for x in got) != (A, C, E, F, OB):  # the file name said so; the code inside must agree
        raise RuntimeError(f"{so}: built for shape {tuple(x.value for x in got)}, asked for {(A, C, E, F, OB)}")
    words3 = (C_.c_int32 * 3)()
    side.mzs_jit_stoch_train_plan(words3)
    if (words3[0], words3[2]) != (words, max_unroll):
        raise RuntimeError(f"{so}: its LDS plan {tuple(words3)} is not stochastic_train_plan's {(words, max_unroll)}")
    fn = C_.cast(side.mzs_jit_stoch_train_launch, C_.c_void_p)
    _lib.check(L.mzs_register_stochastic_train_dispatch(fn, A, C, E, F, OB, side.mzs_jit_stoch_train_abi()))
    _loaded[shape] = side
    return True
