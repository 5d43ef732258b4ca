"""The fused act() kernel's backup when a path has more than 15 edges, against the CPU oracle (every output and every
tree array ==).

Lane e of a 16-lane row owns path entry e, so such a path overflows its row.  Plain-record instances then lay the
wave's four paths end to end over the 64 lanes and back them up in ONE pass -- when the four entry counts (depth + 1)
sum to at most 64; otherwise (and in every other instance) the 16-entry chunk loop runs.  A moderate bias on the policy
head makes the roots of one wave differ in depth, so that both routes and the gate between them are met; each test
re-derives from the ORACLE's parents that the wave-simulations it exists for occur (four consecutive roots share a
wave; rows past the end of the batch shadow the last root).
"""
import numpy as np
import pytest
import torch

from helpers import make_case
from test_gpu_parity import _compare, _fused, _gumbel_oracle_act, _oracle

pytestmark = pytest.mark.gpu

S = 50
SEED = 43


def _case(oracle, B, A, bias):
    case = make_case(oracle, SEED, B, 4, 8, A, S)
    b2 = np.full(A, -bias, np.float32)
    b2[0] = bias
    case["w"]["pp_b2"] = b2
    return case


def _sim_depths(parents, max_depth=0):
    """Edges of every simulation's path, [B, S]: simulation s expands node s + 1 at the end of its path, except where
    the max_depth cut re-expands an existing node (node s + 1 then stays unused, parent -1) at depth max_depth."""
    B = parents.shape[0]
    node_depth = np.zeros((B, S + 1), np.int64)
    dep = np.zeros((B, S), np.int64)
    for k in range(1, S + 1):
        fresh = parents[:, k] >= 0
        node_depth[:, k] = np.where(fresh, node_depth[np.arange(B), np.maximum(parents[:, k], 0)] + 1, 0)
        dep[:, k - 1] = np.where(fresh, node_depth[:, k], max_depth)
        assert fresh.all() or max_depth > 0
    return dep


def _waves(dep):
    """Per wave-simulation: the rows' depths [W, 4, S], and which of them take the wide pass / the chunk loop while
    deep."""
    B = dep.shape[0]
    rows = np.minimum(np.arange(4 * ((B + 3) // 4)), B - 1).reshape(-1, 4)
    d = dep[rows]
    deep = d.max(1) >= 16
    fits = (d + 1).sum(1) <= 64
    return d, deep & fits, deep & ~fits


def _assert_both_routes(dep):
    """A deep wave-simulation that fits 64 lanes with a segment across a 16-lane boundary; one that does not fit; rows
    of exactly 15, 16 and 17 edges on the wide route; all four rows deep."""
    d, wide, loop = _waves(dep)
    assert wide.any() and loop.any()
    off = np.cumsum(d + 1, axis=1) - (d + 1)  # first lane of each row's segment
    crosses = (off // 16 != (off + d) // 16) & (off > 0)  # ... a segment that does not start at lane 0
    assert (crosses.any(1) & wide).any()
    for k in (15, 16, 17):
        assert ((d == k).any(1) & wide).any(), k
    assert (d >= 16).all(1).any()


@pytest.mark.parametrize("tiebreak", [False, True])
@pytest.mark.parametrize("B", [5, 24, 67])
def test_deep_paths_muzero(oracle, B, tiebreak):
    case = _case(oracle, B, 2, 0.3)
    key = [3, 1]
    s, out = _fused(case, tiebreak, key)
    ref = _oracle(oracle, case, tiebreak, key)
    dep = _sim_depths(ref["tree"].parents)
    d, wide, loop = _waves(dep)
    if B == 5:
        # the last wave is root 4 four times over: a deep row there (4 x 17 entries never fit: the chunk loop), and the
        # first wave takes both routes
        assert loop[-1].any() and wide[0].any() and loop[0].any()
    else:
        _assert_both_routes(dep)
    if B == 67:
        assert wide[-1].any()  # roots 64, 65, 66, 66: the wide pass with a shadow row
    _compare(ref, s, out)


@pytest.mark.parametrize("qt,bias", [("qtransform_by_parent_and_siblings", 1.4), ("qtransform_completed_by_mix_value", 0.3)])
def test_deep_paths_gumbel(oracle, qt, bias):
    from muax_amd import MuZeroSearch, SearchConfig
    B = 24
    kind = 1 if qt.endswith("mix_value") else 0
    case = _case(oracle, B, 2, bias)
    key = [21, 22]
    ref = _gumbel_oracle_act(oracle, case, key, kind, 16)
    _assert_both_routes(_sim_depths(ref["tree"].parents))
    s = MuZeroSearch(B, SearchConfig(2, S, 8, policy="gumbel", qtransform=qt, max_num_considered_actions=16, tiebreak=False))
    s.set_mlp_weights({k: torch.from_numpy(v) for k, v in case["w"].items()}, case["obs_dim"], 10, 0.99)
    out = s.act_mlp(torch.from_numpy(case["obs"]), key, with_tree=True)
    torch.cuda.synchronize()
    _compare(ref, s, out)


@pytest.mark.parametrize("tiebreak", [False, True])
def test_deep_paths_four_actions(oracle, tiebreak):
    case = _case(oracle, 24, 4, 0.3)
    key = [3, 1]
    ref = _oracle(oracle, case, tiebreak, key)
    _assert_both_routes(_sim_depths(ref["tree"].parents))
    s, out = _fused(case, tiebreak, key)
    _compare(ref, s, out)


def test_deep_paths_cut_at_max_depth_20(oracle):
    """The cut hands the backup (parent, action, depth, next) of level max_depth - 1 instead of the cached end point:
    rows of exactly 20 edges from re-expanded nodes beside shallower rows, on both routes."""
    case = _case(oracle, 24, 2, 0.3)
    key = [3, 1]
    ref = _oracle(oracle, case, True, key, max_depth=20)
    par = ref["tree"].parents
    assert (par[:, 1:] < 0).any()  # simulations that were cut
    dep = _sim_depths(par, 20)
    assert dep.max() == 20
    _assert_both_routes(dep)
    d, wide, loop = _waves(dep)
    cut = (par[:, 1:] < 0)[np.minimum(np.arange(24), 23).reshape(-1, 4)]
    assert (cut.any(1) & wide).any() and (cut.any(1) & loop).any()
    s, out = _fused(case, True, key, max_depth=20)
    _compare(ref, s, out)


def test_deep_paths_without_tree_export(oracle):
    """The same search with no export requested (the caller's tree arrays are not there to write)."""
    from muax_amd import MuZeroSearch, SearchConfig
    B = 67
    case = _case(oracle, B, 2, 0.3)
    key = [3, 1]
    ref = _oracle(oracle, case, True, key)
    _assert_both_routes(_sim_depths(ref["tree"].parents))
    s = MuZeroSearch(B, SearchConfig(2, S, 8, tiebreak=True))
    s.set_mlp_weights({k: torch.from_numpy(v) for k, v in case["w"].items()}, case["obs_dim"], case["support"], 0.99, "child")
    out = s.act_mlp(torch.from_numpy(case["obs"]), key, dirichlet_noise=torch.from_numpy(case["noise"]),
                    gumbel=torch.from_numpy(case["gumbel"]))
    torch.cuda.synchronize()
    assert np.array_equal(ref["action"], out.action.cpu().numpy())
    assert np.array_equal(ref["action_weights"], out.action_weights.cpu().numpy())
    assert np.array_equal(ref["root_value"], s.root_value.cpu().numpy())
    assert np.array_equal(ref["depth_sum"], s.depth_sum.cpu().numpy().astype(np.int64))
    assert np.array_equal(ref["tree"].node_values[:, 0], s.search_value.cpu().numpy())
