"""The Gumbel MuZero modes of the wide-action act() route (mzs_mlp_allow_wide_gumbel, mzs_mlp_wide_plan_policy) as far as a
machine without a GPU sees them: the ABI declares and exports the two entries, the Python layer offers them, the Gumbel
LDS plan (host arithmetic) gives what its formula says -- test_wide_cpu.py's with 4 + 5 A words per record -- and the
MuZero plan answers what it answered before."""
import ctypes
import inspect

import pytest

from muax_amd import MuZeroSearch, _lib
from muax_amd.search import wide_plan

NEW = ("mzs_mlp_allow_wide_gumbel", "mzs_mlp_wide_plan_policy")


def test_header_declares_and_bindings_list_the_gumbel_entries():
    assert set(NEW) <= set(_lib.EXPORTED_SYMBOLS)  # (which is the header's set: tests/test_abi_cpu.py)
    assert "gumbel" in inspect.signature(MuZeroSearch.allow_wide).parameters
    assert inspect.signature(MuZeroSearch.allow_wide).parameters["gumbel"].default is False
    assert inspect.signature(wide_plan).parameters["policy"].default == "muzero"


def test_built_library_exports_the_gumbel_entries():
    lib = _lib.load(build_if_missing=True)
    assert lib.mzs_mlp_allow_wide_gumbel and lib.mzs_mlp_wide_plan_policy
    assert lib.mzs_abi_version() == 1  # entries were added, nothing changed
    assert lib.mzs_mlp_allow_wide_gumbel(None, 1) == _lib.MZS_E_INVALID  # no handle: refused, nothing touched
    out = (ctypes.c_int32 * 4)()
    assert lib.mzs_mlp_wide_plan_policy(18, 8, 10, 50, 2, ctypes.byref(out)) == _lib.MZS_E_INVALID  # no such policy
    assert lib.mzs_mlp_wide_plan_policy(18, 8, 10, 50, 1, None) == _lib.MZS_E_INVALID


def _plan_by_formula(A, E, F, S, fields):
    """test_wide_cpu.py's budget with `fields` words per action in a record (4: MuZero policy, 5: Gumbel policy)."""
    if not (17 <= A <= 64 and 1 <= E <= 64 and 17 <= F <= 63 and 1 <= S <= 255):
        return None
    r4 = lambda w: (w + 3) // 4 * 4  # noqa: E731
    H, X, N = 16, E + A, S + 1
    weights = (E * H + H + H * F + F) + (E * H + H + H * A + A) + (X * H + H + H * F + F) + (X * H + H + H * E + E)
    wg = r4(weights) + r4(S + 2)
    best = None
    for emb in (True, False):
        for waves in (1, 2, 3, 4):
            root = r4(N * (4 + fields * A) + N + (N * E if emb else 0))
            nbytes = 4 * (wg + waves * root)
            if nbytes > 160 * 1024:
                continue
            roots = min(160 * 1024 // nbytes * waves, 32)
            if best is None or roots > best["roots_per_cu"]:
                best = dict(waves=waves, lds_bytes=nbytes, roots_per_cu=roots, emb_lds=emb)
    return best


SHAPES = [(18, 8, 10, 50), (32, 8, 10, 50), (64, 8, 10, 50), (64, 64, 10, 50), (64, 64, 20, 120), (17, 1, 8, 1),
          (64, 8, 10, 255), (18, 8, 10, 255), (33, 20, 31, 100), (48, 64, 10, 200)]  # test_wide_cpu.py's


def test_gumbel_lds_plan_follows_its_formula():
    taken = 0
    for A, E, support, S in SHAPES + [(18, 32, 10, 50), (64, 8, 10, 110), (64, 8, 10, 130)]:
        got = wide_plan(A, E, support, S, policy="gumbel")
        assert got == _plan_by_formula(A, E, 2 * support + 1, S, 5), (A, E, support, S)
        taken += got is not None
        muzero = wide_plan(A, E, support, S)
        if got is not None:  # the larger record never buys more resident roots
            assert muzero is not None and got["roots_per_cu"] <= muzero["roots_per_cu"]
    assert taken >= 8
    # 64 actions x 130 simulations: 4 (131 x (4 + 4 x 64 + 1)) bytes fit a CU's LDS with the weights, with a fifth field
    # per action they do not -- the MuZero plan takes the shape, the Gumbel plan declines it
    assert wide_plan(64, 8, 10, 130) is not None and wide_plan(64, 8, 10, 130, policy="gumbel") is None
    assert wide_plan(18, 8, 10, 50, policy="gumbel")["roots_per_cu"] >= 4
    for A, E, support, S in [(16, 8, 10, 50), (65, 8, 10, 50), (18, 8, 7, 50), (18, 8, 32, 50), (18, 8, 10, 256), (18, 65, 10, 50)]:
        assert wide_plan(A, E, support, S, policy="gumbel") is None, (A, E, support, S)
    with pytest.raises(ValueError):
        wide_plan(18, 8, 10, 50, policy="alphazero")


def test_muzero_plan_is_what_it_was():
    for A, E, support, S in SHAPES:
        want = _plan_by_formula(A, E, 2 * support + 1, S, 4)
        assert wide_plan(A, E, support, S) == want, (A, E, support, S)
        assert wide_plan(A, E, support, S, policy="muzero") == want
        out = (ctypes.c_int32 * 4)()
        rc = _lib.load().mzs_mlp_wide_plan(A, E, support, S, ctypes.byref(out))
        assert (rc != 0) == (want is None)
        if want is not None:
            assert list(out) == [want["waves"], want["lds_bytes"], want["roots_per_cu"], int(want["emb_lds"])]
