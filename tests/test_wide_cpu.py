"""The wide-action act() route (mzs_mlp_allow_wide, muax_amd/csrc/mz_wide.cuh) as far as a machine without a GPU sees it:
the ABI declares and exports it, the Python handle offers it, the on-demand planner still has nothing for such shapes, and
the LDS plan (host arithmetic) gives what its formula says."""

from muax_amd import MuZeroSearch, _build, _jit, _lib
from muax_amd.search import wide_plan


def test_header_declares_and_bindings_list_allow_wide():
    # (EXPORTED_SYMBOLS is the header's set: tests/test_abi_cpu.py)
    assert {"mzs_mlp_allow_wide", "mzs_mlp_wide_plan", "mzs_mlp_allow_generic"} <= set(_lib.EXPORTED_SYMBOLS)
    assert callable(getattr(MuZeroSearch, "allow_wide"))
    assert "mz_wide.hip" in _build.UNITS


def test_no_on_demand_instance_for_wide_action_sets():
    """The wide route does not go through the on-demand planner: it still has no plan for 17..64 actions."""
    assert _jit.plan(18, 8, 21, 50) is None
    assert _jit.plan(64, 8, 21, 50) is None


def test_built_library_exports_the_wide_entry_points():
    lib = _lib.load(build_if_missing=True)
    assert lib.mzs_mlp_allow_wide and lib.mzs_mlp_wide_plan
    assert lib.mzs_abi_version() == 1
    assert lib.mzs_mlp_allow_wide(None, 1) == _lib.MZS_E_INVALID  # no handle: refused, nothing touched


def _plan_by_formula(A, E, F, S):
    """The budget of include/mzsearch.h, restated: words per workgroup and per root, blocks rounded to 16 bytes; the
    workgroup size 1..4 with most resident roots in 160 KiB (at most 32 wavefronts per CU), embeddings in LDS unless
    leaving them in HBM keeps more roots, ties to the smaller workgroup."""
    if not (17 <= A <= 64 and 1 <= E <= 64 and 17 <= F <= 63 and 1 <= S <= 255):
        return None
    r4 = lambda w: (w + 3) // 4 * 4  # noqa: E731
    H, X, N = 16, E + A, S + 1
    weights = (E * H + H + H * F + F) + (E * H + H + H * A + A) + (X * H + H + H * F + F) + (X * H + H + H * E + E)
    wg = r4(weights) + r4(S + 2)
    best = None
    for emb in (True, False):
        for waves in (1, 2, 3, 4):
            root = r4(N * (4 + 4 * A) + N + (N * E if emb else 0))
            nbytes = 4 * (wg + waves * root)
            if nbytes > 160 * 1024:
                continue
            roots = min(160 * 1024 // nbytes * waves, 32)
            if best is None or roots > best["roots_per_cu"]:
                best = dict(waves=waves, lds_bytes=nbytes, roots_per_cu=roots, emb_lds=emb)
    return best


def test_lds_plan_follows_its_formula():
    shapes = [(18, 8, 10, 50), (32, 8, 10, 50), (64, 8, 10, 50), (64, 64, 10, 50), (64, 64, 20, 120), (17, 1, 8, 1),
              (64, 8, 10, 255), (18, 8, 10, 255), (33, 20, 31, 100), (48, 64, 10, 200)]
    for A, E, support, S in shapes:
        assert wide_plan(A, E, support, S) == _plan_by_formula(A, E, 2 * support + 1, S), (A, E, support, S)
    # the Atari action set at the metric's search length: several roots per workgroup, more than one workgroup per CU
    p = wide_plan(18, 8, 10, 50)
    assert p["emb_lds"] and p["roots_per_cu"] >= 8 and p["lds_bytes"] * (p["roots_per_cu"] // p["waves"]) <= 160 * 1024
    # 64 actions: a root is tens of KB, still two to a CU; at 255 simulations one root is beyond a CU's LDS
    assert wide_plan(64, 8, 10, 50)["roots_per_cu"] >= 2
    assert wide_plan(64, 8, 10, 255) is None
    # what the kernel declines whatever the LDS: 16 actions and fewer, more than 64, support_size outside 8..31, S > 255
    for A, E, support, S in [(16, 8, 10, 50), (65, 8, 10, 50), (18, 8, 7, 50), (18, 8, 32, 50), (18, 8, 10, 256), (18, 65, 10, 50)]:
        assert wide_plan(A, E, support, S) is None, (A, E, support, S)
