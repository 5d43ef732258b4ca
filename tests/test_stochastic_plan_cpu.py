"""The LDS plan of the one-launch stochastic search (mzs_mlp_stochastic_plan / search.stochastic_plan): host arithmetic,
no device."""
import pytest

from muax_amd import search

LDS_PER_CU = 160 * 1024
SHAPES = [(4, 32, 16, 10), (4, 3, 5, 8), (18, 40, 64, 31), (2, 62, 8, 8), (1, 1, 1, 8), (3, 5, 64, 10)]


@pytest.mark.parametrize("A,C,E,support", SHAPES)
def test_plan_arithmetic(A, C, E, support):
    last = None
    for S in (1, 2, 7, 20, 50, 51, 100, 200, 255):
        pl = search.stochastic_plan(A, C, E, support, S)
        if pl is None:  # (once one root's tree is too large it stays so)
            last = 0
            continue
        assert set(pl) == {"waves", "lds_bytes", "roots_per_cu", "emb_lds"}
        assert 0 < pl["lds_bytes"] <= LDS_PER_CU and pl["lds_bytes"] % 16 == 0
        assert 1 <= pl["waves"] <= 4
        assert pl["waves"] <= pl["roots_per_cu"] == min(32, LDS_PER_CU // pl["lds_bytes"] * pl["waves"])
        assert last is None or pl["roots_per_cu"] <= last, "resident roots grew with num_simulations"
        last = pl["roots_per_cu"]


def test_plan_admits_and_declines():
    assert search.stochastic_plan(4, 32, 16, 10, 50) is not None
    assert search.stochastic_plan(1, 1, 1, 8, 1) is not None
    assert search.stochastic_plan(4, 61, 16, 10, 50) is None and search.stochastic_plan(33, 32, 16, 10, 50) is None  # A + C = 65
    assert search.stochastic_plan(4, 60, 16, 10, 50) is not None                                                    # A + C = 64
    assert search.stochastic_plan(4, 32, 65, 10, 50) is None and search.stochastic_plan(4, 32, 64, 10, 50) is not None
    assert search.stochastic_plan(4, 32, 16, 7, 50) is None and search.stochastic_plan(4, 32, 16, 32, 50) is None
    assert search.stochastic_plan(4, 32, 16, 8, 50) is not None and search.stochastic_plan(4, 32, 16, 31, 50) is not None
    assert search.stochastic_plan(4, 3, 5, 8, 256) is None and search.stochastic_plan(4, 3, 5, 8, 255) is not None
    assert search.stochastic_plan(4, 3, 5, 8, 0) is None and search.stochastic_plan(0, 3, 5, 8, 4) is None


def test_2048_shape_shares_a_workgroup():
    """4 + 32 slots, E = 16, F = 21, 50 simulations: about 21 KB of weights and 34 KB per root -- several roots share
    one copy of the weights, the embeddings stay in LDS."""
    A, C, E, F, S, H = 4, 32, 16, 21, 50, 16
    pl = search.stochastic_plan(A, C, E, 10, S)
    assert pl["waves"] in (3, 4) and pl["emb_lds"] and pl["roots_per_cu"] >= pl["waves"]
    r4 = lambda w: (w + 3) // 4 * 4  # noqa: E731
    head = lambda i, o: i * H + H + H * o + o  # noqa: E731
    weights = head(E + A, E) + head(E, F) + head(E, C) + head(E + C, F) + head(E + C, E) + head(E, F) + head(E, A)
    root = (S + 1) * (4 + 4 * (A + C)) + (S + 1) + (S + 1) * E  # records, path, embeddings
    assert 20_000 < 4 * weights < 22_000 and 33_000 < 4 * root < 35_000
    assert pl["lds_bytes"] == 4 * (r4(weights) + r4(S + 2) + pl["waves"] * r4(root))


def test_largest_tree_of_the_widest_shape():
    """All 64 slots, E = 64, F = 63: the weights leave room for fewer than 255 simulations of one root."""
    admitted = [S for S in range(1, 256) if search.stochastic_plan(2, 62, 64, 31, S) is not None]
    assert admitted and admitted == list(range(1, admitted[-1] + 1))
    assert admitted[-1] < 255
    assert search.stochastic_plan(2, 62, 64, 31, admitted[-1] + 1) is None
    assert search.stochastic_plan(2, 62, 64, 31, admitted[-1])["waves"] == 1


def test_binding_declares_the_entries():
    """(That ENTRIES is the header's list, `int` returns included: tests/test_abi_cpu.py.)"""
    import ctypes as C
    from muax_amd import _lib
    for name in ("mzs_mlp_stochastic_plan", "mzs_mlp_stochastic_search", "mzs_stochastic_search_block"):
        assert _lib.ENTRIES[name][0] is C.c_int
    assert C.sizeof(_lib.MzsStochasticSearchArgs) == 8 + 6 * 8 + 16 + 5 * 8
