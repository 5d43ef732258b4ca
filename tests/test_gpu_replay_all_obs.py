"""GPU tests of the all-steps observation block of the replay sample kernels (`mzs_replay_sample_args.obs_steps`,
muax_amd/csrc/mz_replay.cuh) through the C ABI alone, on the guarded buffers of tests/replay_abi.py, against the loop
reference tests/replay_obs_reference.py for the block and tests/replay_reference.py for the draws.

These are copies: everything is compared with ==, on the bits.  For every case every other output equals, byte for
byte, that of the same call with obs_steps = 0, whose obs is row 0 of the block.

Shapes: obs_dim 1, 3, 16, 65, 130 by k_steps 1, 2, 5, 67 -- the run of k * obs_dim floats a wavefront copies falls
below, on and across multiples of its 64 lanes (1 .. 8710) and starts on any 4-byte boundary; batches of 1, 5 and 9 rows
(never a multiple of the four rows of a workgroup) with 1 and 3 rows per trajectory.  The longest episode ends on the
arena's final row: the last start the kernel can draw is length - k_steps - 1, so its window ends one row before; a key
that draws exactly that start is found with the reference on the CPU, and a copy that ran on past the window would
carry the arena's last row or the guard pattern behind it into an output that is compared."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import replay_obs_reference as obsref
import replay_reference as ref
from muax_amd import _lib
from replay_abi import _PATTERN, Guarded, Replay

pytestmark = pytest.mark.gpu
F32 = np.float32
ACTIONS, HEAD, GAP = 3, 1, 3
OBS_DIMS, K_STEPS, BATCHES, SPTS = (1, 3, 16, 65, 130), (1, 2, 5, 67), (1, 5, 9), (1, 3)
FIELDS = ("a", "r", "Rn", "v", "done", "pi", "w", "serial", "start")
END = 2  # the episode that ends on the arena's final row


def _lengths(k):
    """Oldest first: two short eligible ones, the long one, one of exactly k and one below (neither can be drawn)."""
    return (k + 1, k + 4, 2 * k + 3, k, max(1, k - 1))


def call(rp, count, B, k, spt, key, obs_steps, obs_floats=None, is_args=None):
    """mzs_replay_sample, or with `is_args` = (beta, num_windows, normalize) mzs_replay_sample_is, with `obs_steps` set:
    (status, {field: host array}, {field: Guarded}).  obs has `obs_floats` floats per row (default: what obs_steps
    asks for); every output starts as the pattern and keeps its guards."""
    od = rp.obs_dim
    obs_floats = (k if obs_steps else 1) * od if obs_floats is None else obs_floats
    shapes = dict(obs=(B, obs_floats, torch.float32), a=(B, k, torch.int32), r=(B, k, torch.float32),
                  Rn=(B, k, torch.float32), v=(B, k, torch.float32), done=(B, k, torch.uint8),
                  pi=(B, k * rp.A, torch.float32), w=(B, k, torch.float32), serial=(B, 1, torch.int64),
                  start=(B, 1, torch.int32))
    out = {n: Guarded(rows, width, dt, flat=False) for n, (rows, width, dt) in shapes.items()}
    s = _lib.MzsReplaySampleArgs()
    s.struct_size = C.sizeof(_lib.MzsReplaySampleArgs)
    s.count, s.batch, s.k_steps, s.sample_per_trajectory = int(count), int(B), int(k), int(spt)
    s.key[0], s.key[1] = int(key[0]), int(key[1])
    s.obs_steps = int(obs_steps)
    for n, g in out.items():
        setattr(s, n, g.ptr)
    if is_args is None:
        rc = rp._call(rp.L.mzs_replay_sample, (C.byref(rp.arena), C.byref(s)), {}, [(g, True) for g in out.values()])
    else:
        out["isw"], out["scratch"] = Guarded(B, 1, torch.float32, flat=False), Guarded(B, 1, torch.float64, flat=False)
        q = _lib.MzsReplayIsArgs()
        q.struct_size = C.sizeof(_lib.MzsReplayIsArgs)
        q.beta, q.num_windows, q.normalize = float(is_args[0]), float(is_args[1]), int(is_args[2])
        q.isw, q.scratch = out["isw"].ptr, out["scratch"].ptr
        rc = rp._call(rp.L.mzs_replay_sample_is, (C.byref(rp.arena), C.byref(s), C.byref(q)), {},
                      [(g, True) for g in out.values()])
    got = {n: g.host() for n, g in out.items()}
    if obs_steps == k and obs_floats == k * od:
        got["obs"] = got["obs"].reshape(B, k, od)
    return rc, got, out


def _untouched(out):
    return all(bool((g.bits == _PATTERN[g.dtype]).all()) for g in out.values())


@functools.lru_cache(maxsize=None)
def _episodes(od, k, zero_buffer=False):
    """The episodes of a case, oldest first (host arrays; nothing below modifies them).  The window start
    length - k - 1 of END carries about half of its weight, so that a key that draws it is found quickly.
    `zero_buffer`: every buffer weight is zero, so every draw lands on the newest episode, which is shorter than k + 1."""
    rng = np.random.default_rng(100 * od + k)
    lengths = _lengths(k)
    eps = [ref.make_episode(rng, T, ACTIONS, od, w=ref.dyadic_weights(rng, T) + 2.0 ** -10) for T in lengths]
    eps[END]["w"][lengths[END] - k - 1] = 512.0 * (lengths[END] - k)  # (about the sum of the others)
    eps[END]["weight"] = 2048.0
    if zero_buffer:
        for ep in eps:
            ep["weight"] = 0.0
    return eps


@functools.lru_cache(maxsize=None)
def _stored(od, k, zero_buffer=False):
    """(store, episodes, serials): stored by the copy branch in table slots HEAD.., refreshed for k.  The arena has GAP
    uncovered rows before every episode and episode END last, ending exactly at max_steps."""
    eps, lengths = _episodes(od, k, zero_buffer), _lengths(k)
    count, cap = len(lengths), len(lengths) + 2
    rp = Replay(sum(lengths) + GAP * count, cap, od, ACTIONS)
    order = [i for i in range(count) if i != END] + [END]
    desc, at, src = np.zeros((count, 4), np.int32), 0, np.concatenate([[0], np.cumsum(lengths)[:-1]])
    for i in order:
        at += GAP
        desc[i] = (src[i], at, lengths[i], (HEAD + i) % cap)
        at += lengths[i]
    assert at == rp.max_steps == desc[END][1] + desc[END][2]
    cat = {n: np.concatenate([ep[n] for ep in eps]) for n in ("obs", "a", "r", "Rn", "v", "done", "pi", "w")}
    serial = 70 + 3 * np.arange(count)
    assert rp.store(desc, serial, cat["obs"], cat["a"], cat["pi"], cat["r"], cat["v"], raw=False,
                    ep_w=[ep["weight"] for ep in eps], Rn=cat["Rn"], done=cat["done"].astype(np.uint8),
                    w=cat["w"]) == _lib.MZS_OK
    assert rp.refresh(HEAD, count, k) == _lib.MZS_OK
    return rp, eps, serial


@functools.lru_cache(maxsize=None)
def _key_of_the_last_start(od, k, B, spt):
    """A key under which, by the loop reference, a row draws episode END at its last eligible start."""
    eps = _episodes(od, k)
    last = len(eps[END]["w"]) - k - 1
    for n in range(4000):
        e, start = ref.sample_indices([911, n], eps, B, k, spt)
        if ((e == END) & (start == last)).any():
            return (911, n)
    raise AssertionError("no key draws the last eligible start")


def _u32(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def _assert_block(rp, eps, serial, B, k, spt, key, is_args=None):
    count = len(eps)
    rc0, plain, _ = call(rp, count, B, k, spt, key, 0, is_args=is_args)
    rc1, got, _ = call(rp, count, B, k, spt, key, k, is_args=is_args)
    assert rc0 == rc1 == _lib.MZS_OK
    e, start = ref.sample_indices(key, eps, B, k, spt)
    assert np.array_equal(got["serial"][:, 0], serial[e]) and np.array_equal(got["start"][:, 0], start)
    want = obsref.batch_obs(eps, e, start, k)
    assert got["obs"].shape == want.shape == (B, k, rp.obs_dim)
    assert np.array_equal(_u32(got["obs"]), _u32(want)), (B, spt, key)
    assert np.array_equal(_u32(plain["obs"]), _u32(want[:, 0])), (B, spt, key)  # the default: transition i alone
    for n in FIELDS + (("isw", "scratch") if is_args else ()):
        assert got[n].dtype == plain[n].dtype and got[n].tobytes() == plain[n].tobytes(), (n, B, spt, key)
    if k == 1:  # obs_steps = 1 is obs_steps = 0
        assert got["obs"].tobytes() == plain["obs"].tobytes()
    return e, start


@pytest.mark.parametrize("k", K_STEPS)
@pytest.mark.parametrize("od", OBS_DIMS)
def test_every_steps_observations_equal_the_loop_reference(od, k):
    rp, eps, serial = _stored(od, k)
    last, hit = len(eps[END]["w"]) - k - 1, 0
    for B in BATCHES:
        for spt in SPTS:
            _assert_block(rp, eps, serial, B, k, spt, (40 + B, spt))
            e, start = _assert_block(rp, eps, serial, B, k, spt, _key_of_the_last_start(od, k, B, spt))
            hit += int(((e == END) & (start == last)).sum())
    assert hit >= len(BATCHES) * len(SPTS)  # the window that ends next to the arena's final row was drawn every time


@pytest.mark.parametrize("k", K_STEPS)
@pytest.mark.parametrize("od", OBS_DIMS)
def test_rows_with_nothing_to_draw_are_zero_filled_whole(od, k):
    """All buffer weights zero: every draw lands on the newest episode, which is no longer than k_steps (m <= 0)."""
    rp, eps, _ = _stored(od, k, zero_buffer=True)
    assert len(eps[-1]["w"]) <= k
    for B in BATCHES:
        rc0, plain, _ = call(rp, len(eps), B, k, 3, (5, B), 0)
        rc1, got, _ = call(rp, len(eps), B, k, 3, (5, B), k)
        assert rc0 == rc1 == _lib.MZS_OK
        assert got["obs"].shape == (B, k, od) and not _u32(got["obs"]).any()  # +0.0 in all k * obs_dim floats
        assert (got["serial"] == -1).all() and (got["start"] == -1).all()
        assert plain["obs"].shape == (B, od) and not _u32(plain["obs"]).any()
        for n in FIELDS:
            assert got[n].tobytes() == plain[n].tobytes(), n


@pytest.mark.parametrize("od,k", [(3, 5), (65, 2), (16, 67)])
def test_sample_is_takes_the_field_and_keeps_its_weights(od, k):
    rp, eps, serial = _stored(od, k)
    N = sum(len(ep["w"]) - k for ep in eps if len(ep["w"]) > k)
    for beta, normalize in ((1.0, True), (0.4, False)):
        for B in (5, 9):
            _assert_block(rp, eps, serial, B, k, 3, (77, B), is_args=(beta, N, normalize))
    # ... and the batch is that of mzs_replay_sample
    _, a, _ = call(rp, len(eps), 9, k, 3, (77, 9), k)
    _, b, _ = call(rp, len(eps), 9, k, 3, (77, 9), k, is_args=(1.0, N, True))
    assert all(a[n].tobytes() == b[n].tobytes() for n in FIELDS + ("obs",))


@pytest.mark.parametrize("is_args", [None, (1.0, 20.0, True)])
def test_other_values_of_obs_steps_are_refused_and_nothing_is_written(is_args):
    od, k = 3, 5
    rp, eps, _ = _stored(od, k)
    for bad in (2, -1, k + 1, 1):
        rc, _, out = call(rp, len(eps), 9, k, 1, (1, 2), bad, obs_floats=(k + 1) * od, is_args=is_args)
        assert rc == _lib.MZS_E_INVALID and _untouched(out), bad
        msg = rp.L.mzs_last_error(None)
        assert b"obs_steps must be 0" in msg and b"k_steps" in msg, msg
    rc, _, out = call(rp, len(eps), 9, k, 1, (1, 2), k, obs_floats=k * od, is_args=is_args)
    assert rc == _lib.MZS_OK and not _untouched(out)
