"""The step-wise kernels (mz_step_kernels.cuh: the walking and the cached-decision set, both built from the per-node rules
of mz_step.cuh, the second through the bodies of mz_step_jump.cuh; launched by mz_stepwise.hip) against the C oracle, both fed the same
*script* instead of a net (tests/scripted_search.py): per-edge discounts with exact 0s and 1s, re-expansions that write
other numbers than the first expansion, exact ties, logits of -1e9 and +-80, rewards in the thousands next to 1e-3, one
line 130 levels deep.  The bar is the project's: the selected action and the parent embedding at every simulation, the
final action and action weights, every tree array bit for bit, depth_sum -- and, independently of the oracle, the exported
tree holds for every edge and node the script row of the LAST simulation that expanded it.  The references are checked on
the CPU in tests/test_scripted_search_cpu.py."""
import numpy as np
import pytest
import torch

import scripted_search as ss

pytestmark = pytest.mark.gpu

PAS, MIX = "qtransform_by_parent_and_siblings", "qtransform_completed_by_mix_value"
# (A, B, S): the 16-lane action slots (1, 2, 16 | 17, 64 = the step-wise maximum) against batches ragged against the rows
# per workgroup; S >= 28 = 4 x the deepest max_depth cut.  Shapes with 16 and more actions draw invalid root actions (and,
# where B > 1, one all-invalid root).
SHAPES = [(1, 7, 29), (2, 33, 40), (16, 1, 33), (17, 7, 36), (64, 33, 40)]
# (A, B, S, max_depth) of the re-expansion family: at most S / 2 nodes exist within the cut (7, 2 + 4 + 8 = 14, 16, 17, 2),
# so in every root at least half of the simulations re-expand -- asserted in every case.  (64 actions cannot within 40
# simulations; the other families cover them.)
REEXPANSION_SHAPES = [(1, 7, 29, 7), (2, 33, 40, 3), (16, 1, 33, 1), (17, 7, 36, 1), (2, 33, 40, 1)]
E = 8
MUZERO_FAMILIES = ["discounts", "generic", "reexpansion", "ties", "extreme_logits", "large"]
GUMBEL_FAMILIES = ["discounts", "reexpansion", "ties", "extreme_logits"]


def _two_shapes(k, family):
    """Two (A, B, S, max_depth) for the k-th combination of a family: over a family's combinations -- and over those of
    either set of tree kernels alone -- every shape of the list comes up."""
    shapes = REEXPANSION_SHAPES if family == "reexpansion" else [s + (None,) for s in SHAPES]
    return [shapes[k % 5], shapes[(k + 2) % 5]]


class _TreeArrays:
    """The exported tree's integer arrays as NumPy attributes (for scripted_search.check_structure)."""

    def __init__(self, t):
        for k in ("node_visits", "children_visits", "children_index", "parents", "action_from_parent"):
            setattr(self, k, getattr(t, k).cpu().numpy())


def _check_against_script(sc, res, max_depth):
    """What the script itself says the exported tree holds (plain array comparisons, no oracle), and depth_sum."""
    t = res["out"].search_tree
    want = ss.expected_last_writes(sc, res["actions"], res["parent_emb"])
    got = {k: getattr(t, k).cpu().numpy() for k in ("children_rewards", "children_discounts", "raw_values",
                                                     "children_prior_logits", "embeddings")}
    for k in ("children_rewards", "children_discounts", "raw_values", "embeddings"):
        assert np.array_equal(want[k], got[k]), k
    assert np.array_equal(want["children_prior_logits"][:, 1:], got["children_prior_logits"][:, 1:])
    nv, cv = t.node_visits.cpu().numpy(), t.children_visits.cpu().numpy()
    assert np.array_equal(want["expanded"][:, 1:], nv[:, 1:] - cv[:, 1:].sum(-1))  # every re-expansion counted
    if max_depth:
        share = ss.reexpansion_share(nv, sc.S)
        assert want["reexpanded"] and share.min() >= 0.5, share  # most simulations overwrite an existing node
    else:
        assert not want["reexpanded"]
        depth = ss.node_depths(t.parents.cpu().numpy())
        assert np.array_equal(depth.sum(1), res["handle"].depth_sum.cpu().numpy())
    ss.check_structure(_TreeArrays(t), sc.S, sc.invalid, reexpansion=bool(max_depth))


def _run(oracle, family, A, B, S, seed, max_depth=None, e=E, **kw):
    sc = ss.make_script(family, seed, B, A, e, S, invalid=A >= 16, max_depth=max_depth)
    res = ss.drive_hip_script(oracle, sc, **kw)
    _check_against_script(sc, res, max_depth)
    res["handle"].close()
    return res


@pytest.mark.parametrize("tiebreak", [False, True])
@pytest.mark.parametrize("walk,fused_select", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("family", MUZERO_FAMILIES)
def test_muzero_scripted_matches_oracle(oracle, family, walk, fused_select, tiebreak, monkeypatch):
    """Every family on both sets of tree kernels (cached decisions / MZS_STEP_WALK=1) and both call shapes (mzs_select +
    mzs_expand_backup / mzs_expand_backup_select), tie-break noise off and on."""
    if walk:
        monkeypatch.setenv("MZS_STEP_WALK", "1")
    k = 4 * walk + 2 * fused_select + tiebreak
    for A, B, S, max_depth in _two_shapes(k + MUZERO_FAMILIES.index(family), family):
        res = _run(oracle, family, A, B, S, 10 + k, max_depth, tiebreak=tiebreak, fused_select=fused_select)
        if family == "discounts" and B >= 3:
            d = res["out"].search_tree.children_discounts.cpu().numpy()
            ci = res["out"].search_tree.children_index.cpu().numpy()
            assert (d[B - 1] == 0).all() and (d[B - 2][ci[B - 2] >= 0] == 1).all()


@pytest.mark.parametrize("max_considered", [2, 16])
@pytest.mark.parametrize("walk", [False, True])
@pytest.mark.parametrize("qt", [MIX, PAS])
@pytest.mark.parametrize("family", GUMBEL_FAMILIES)
def test_gumbel_scripted_matches_oracle(oracle, family, qt, walk, max_considered, monkeypatch):
    """Gumbel MuZero (sequential halving at the root, deterministic interior selection), both qtransforms: q = reward +
    discount * value of the two qtransforms on per-edge discounts, their degenerate min-max normalisation on ties."""
    if walk:
        monkeypatch.setenv("MZS_STEP_WALK", "1")
    k = 4 * (qt == PAS) + 2 * walk + (max_considered == 16)
    for A, B, S, max_depth in _two_shapes(k + GUMBEL_FAMILIES.index(family), family):
        _run(oracle, family, A, B, S, 40 + k, max_depth, policy="gumbel", qtransform=qt, max_considered=max_considered)


@pytest.mark.parametrize("tiebreak", [False, True])
@pytest.mark.parametrize("walk,fused_select", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("S", [17, 65, 130])
def test_single_deep_line_with_varying_discounts(oracle, S, walk, fused_select, tiebreak, monkeypatch):
    """+20 on action 0 at every node: simulation k walks a path of length k + 1, so the deepest paths are 15, 16, 17 /
    63, 64, 65 / 126 .. 130 levels -- either side of the walk's 16-entry chunks and of return_chain's 63-level chunks --
    with another reward and discount (0s and 1s among them) on every edge of the line."""
    if walk:
        monkeypatch.setenv("MZS_STEP_WALK", "1")
    res = _run(oracle, "deep_line", 2, 7, S, S, tiebreak=tiebreak, fused_select=fused_select)
    t = res["out"].search_tree
    assert (res["actions"] == 0).all()
    assert np.array_equal(t.parents.cpu().numpy()[:, 1:], np.tile(np.arange(S), (7, 1)))  # one chain of depth S
    d = t.children_discounts.cpu().numpy()[:5, :S, 0]
    assert (d == 0).any() and (d == 1).any() and len(np.unique(d)) > 5


@pytest.mark.parametrize("walk,fused_select", [(False, False), (True, False), (False, True), (True, True)])
def test_wide_embedding_rows(oracle, walk, fused_select, monkeypatch):
    """E >= 256: the wide-row transfer of parent and next embeddings, on a generic script."""
    if walk:
        monkeypatch.setenv("MZS_STEP_WALK", "1")
    _run(oracle, "generic", 17, 7, 12, 70, e=260, tiebreak=True, fused_select=fused_select)


@pytest.mark.parametrize("fused_select", [False, True])
@pytest.mark.parametrize("S", [1023, 1024])
def test_tree_size_where_the_walking_kernels_take_over(oracle, S, fused_select, monkeypatch):
    """No MZS_STEP_WALK: S = 1023 (1024 nodes, kJumpMaxNodes) is the largest tree of the cached-decision kernels (their
    LDS at 15 x 1025 words), S = 1024 the smallest one the walking kernels get by size alone.  Which set ran is read off
    mzs_resnet_search, whose first question is whether the handle's tree has cached decisions: without them it answers
    MZS_E_UNSUPPORTED, with them it goes on to reject its (null) arguments."""
    from muax_amd import _lib
    monkeypatch.delenv("MZS_STEP_WALK", raising=False)
    monkeypatch.delenv("MZS_JUMP_BUDGET_MB", raising=False)
    for family in ("generic", "deep_line"):
        sc = ss.make_script(family, S, 3, 2, E, S)
        res = ss.drive_hip_script(oracle, sc, tiebreak=True, fused_select=fused_select)
        _check_against_script(sc, res, None)
        h = res["handle"]
        rc = _lib.load().mzs_resnet_search(h._h, None, 1.0, 0, 1, None)
        msg = _lib.load().mzs_last_error(h._h).decode()
        if S + 1 <= 1024:
            assert rc == _lib.MZS_E_INVALID and "cached decisions" not in msg, (rc, msg)
        else:
            assert rc == _lib.MZS_E_UNSUPPORTED and "cached decisions" in msg, (rc, msg)
        h.close()


@pytest.mark.parametrize("policy", ["muzero", "gumbel"])
def test_search_convenience_loop_with_a_script_as_recurrent_fn(oracle, policy):
    """MuZeroSearch.search() (eager, graph=False) with the script as its recurrent_fn: the convenience loop gives the tree
    the C oracle builds from the same script."""
    from helpers import assert_trees_equal
    from muax_amd import MuZeroSearch, SearchConfig
    A, B, S, key = 2, 33, 30, [6, 7]  # 2 + 4 + 8 = 14 nodes within the cut: most simulations re-expand
    sc = ss.make_script("reexpansion", 80, B, A, E, S, invalid=True, max_depth=3)
    kw = dict(policy="gumbel", qtransform=MIX, max_considered=4) if policy == "gumbel" else dict(policy="muzero", tiebreak=True)
    ref = ss.run_oracle(oracle, sc, key=key, **kw)
    s = MuZeroSearch(B, SearchConfig(A, S, E, max_depth=3, tiebreak=True, policy=policy, qtransform=kw.get("qtransform", PAS),
                                     max_num_considered_actions=4))
    root_out, rec = ss.script_root_and_rec(sc)
    out = s.search(root_out, rec.counting(), key, torch.from_numpy(sc.invalid),
                   dirichlet_noise=torch.from_numpy(sc.noise), gumbel=torch.from_numpy(sc.gumbel) if policy == "gumbel" else None,
                   with_tree=True, graph=False)
    assert np.array_equal(ref["action"], out.action.cpu().numpy())
    assert np.array_equal(ref["action_weights"], out.action_weights.cpu().numpy())
    assert np.array_equal(ref["depth_sum"], s.depth_sum.cpu().numpy().astype(np.int64))
    assert_trees_equal(ref["tree"], out.search_tree, exact_floats=True)
    assert ss.reexpansion_share(ref["tree"].node_visits, S).min() >= 0.5
    s.close()
