"""Two-action value scores of the fused act() kernel against the C oracle, at the smallest shapes where they can go wrong.

A node with two children is where the fused kernel may carry the per-action values (prior, value, reward, q, score) as
one packed pair; a packed f32 op rounds each half like the scalar op, so every exported array must stay EQUAL (==) to
the oracle's.  Shapes: 5 roots (one wavefront, its fourth row shadowing the last root) and 17 roots (two workgroups);
one simulation (the root's initial scores only), two (the first backup, depth 1), fifty with and without a depth limit;
masked root actions; networks whose q values coincide (span below the normalisation's epsilon), whose numerators fall
into the IEEE-division branch, and three / four actions, which keep the per-action code.
"""
import numpy as np
import pytest
import torch

from helpers import assert_trees_equal, make_case

pytestmark = pytest.mark.gpu

F32 = np.float32
DISCOUNT = 0.99


def _fused(case, tiebreak, key, max_depth=None, discount=DISCOUNT):
    from muax_amd import MuZeroSearch, SearchConfig
    cfg = SearchConfig(case["A"], case["S"], case["E"], max_depth=max_depth, tiebreak=tiebreak)
    s = MuZeroSearch(case["B"], cfg)
    s.set_mlp_weights({k: torch.from_numpy(v) for k, v in case["w"].items()}, case["obs_dim"], case["support"], discount,
                      "child")
    out = s.act_mlp(torch.from_numpy(case["obs"]), key, dirichlet_noise=torch.from_numpy(case["noise"]),
                    invalid_actions=None if case["invalid"] is None else torch.from_numpy(case["invalid"]),
                    temperature=1.0, gumbel=torch.from_numpy(case["gumbel"]), with_tree=True)
    torch.cuda.synchronize()
    return s, out


def _oracle(oracle, case, tiebreak, key, max_depth=0, discount=DISCOUNT):
    mlp = oracle.Mlp(case["w"], case["obs_dim"], case["E"], case["A"], case["F"], support_size=case["support"],
                     recurrent_pred_on=0, discount=discount)
    cfg = oracle.SearchCfg(case["S"], max_depth=max_depth or 0, tiebreak=int(tiebreak))
    return oracle.act_mlp(mlp, cfg, case["obs"], key, case["noise"], 0.25, case["invalid"], 1.0, case["gumbel"])


def _check(oracle, case, tiebreak, key, max_depth=0, discount=DISCOUNT):
    ref = _oracle(oracle, case, tiebreak, key, max_depth, discount)
    s, out = _fused(case, tiebreak, key, max_depth or None, discount)
    assert np.array_equal(ref["action"], out.action.cpu().numpy())
    assert np.array_equal(ref["action_weights"], out.action_weights.cpu().numpy())
    assert np.array_equal(ref["root_value"], s.root_value.cpu().numpy())
    assert np.array_equal(ref["tree"].node_values[:, 0], s.search_value.cpu().numpy())
    assert_trees_equal(ref["tree"], out.search_tree, exact_floats=True)
    return ref


def _spans(tree, discount):
    """max - min of {node value, q of the visited children} for every node with a visited child (what the value
    scores are normalised by), recomputed in float32 from the final tree."""
    vis = tree.children_visits > 0
    q = (tree.children_rewards + F32(discount) * tree.children_values).astype(F32)
    nv = tree.node_values[..., None]
    lo = np.minimum(np.where(vis, q, nv).min(-1), tree.node_values)
    hi = np.maximum(np.where(vis, q, nv).max(-1), tree.node_values)
    return (hi - lo)[vis.any(-1)]


@pytest.mark.parametrize("tiebreak", [False, True])
@pytest.mark.parametrize("B", [5, 17])
@pytest.mark.parametrize("S,max_depth", [(1, 0), (2, 0), (50, 0), (50, 3)])
def test_two_actions_match_oracle(oracle, B, S, max_depth, tiebreak):
    case = make_case(oracle, 40 + S, B, 4, 8, 2, S)
    ref = _check(oracle, case, tiebreak, [S, 7 + B], max_depth)
    if S == 50 and max_depth == 0 and B == 17:
        assert ref["depth_sum"].max() / S > 4  # (paths long enough for every lane role of a backup pass)


@pytest.mark.parametrize("tiebreak", [False, True])
def test_two_actions_masked_root_actions(oracle, tiebreak):
    case = make_case(oracle, 51, 17, 4, 8, 2, 20, invalid_frac=0.4)
    inv = case["invalid"]
    assert 0 < inv[1:].sum() < inv[1:].size and (inv[1:].sum(1) == 1).any()  # some roots with exactly one masked action
    ref = _check(oracle, case, tiebreak, [3, 1])
    one = inv.sum(1) == 1
    assert (inv[np.arange(17), ref["action"]][one] == 0).all()


@pytest.mark.parametrize("tiebreak", [False, True])
@pytest.mark.parametrize("scale", [200.0, 1e-8])
def test_two_actions_extreme_weight_scales(oracle, scale, tiebreak):
    """Weights x 200: the decodes saturate at the ends of the support (one-hot distributions, q spans above 100).
    Scaling up does not reach the span's 1e-8 floor (the oracle's spans of this case stay above it); weights x 1e-8 do:
    priors that differ in their last bits, values and rewards that decode to exact zeros, every span below the floor."""
    case = make_case(oracle, 52, 17, 4, 8, 2, 30)
    case["w"] = {k: (v * scale).astype(F32) for k, v in case["w"].items()}
    ref = _check(oracle, case, tiebreak, [5, 2])
    sp = _spans(ref["tree"], DISCOUNT)
    assert sp.max() > 100 if scale > 1 else (sp < 1e-8).all()


@pytest.mark.parametrize("B", [5, 17])
def test_two_actions_all_zero_weights_every_decision_a_tie(oracle, B):
    case = make_case(oracle, 53, B, 4, 8, 2, 30)
    case["w"] = {k: np.zeros_like(v) for k, v in case["w"].items()}
    for tiebreak in (False, True):
        ref = _check(oracle, case, tiebreak, [6, 3])
        assert (_spans(ref["tree"], DISCOUNT) == 0).all()


def test_two_actions_ieee_division_fallback(oracle):
    """The network of test_fused_rare_division_paths: an all-zero reward head and a discount of 1e-30 or 3e-33, so the
    value-score numerators q - min q lie in (0, 2^-100), where the shared reciprocal hands over to the IEEE division."""
    case = make_case(oracle, 902, 17, 4, 8, 2, 40)
    w = dict(case["w"])
    for k in ("dr_w1", "dr_b1", "dr_w2", "dr_b2"):
        w[k] = np.zeros_like(w[k])
    flat = dict(case, w=w)
    for disc in (1e-30, 3e-33):
        ref = _check(oracle, flat, False, [2, 9], discount=disc)
        tree = ref["tree"]
        vis = tree.children_visits > 0
        q = (tree.children_rewards + F32(disc) * tree.children_values).astype(F32)
        lo = np.minimum(np.where(vis, q, tree.node_values[..., None]).min(-1), tree.node_values)
        num = (q - lo[..., None])[vis]
        assert ((num > 0) & (num < 2.0 ** -100)).any()


@pytest.mark.parametrize("tiebreak", [False, True])
@pytest.mark.parametrize("A,E,obs_dim", [(3, 8, 4), (4, 32, 8)])
def test_more_actions_keep_the_per_action_path(oracle, A, E, obs_dim, tiebreak):
    case = make_case(oracle, 60 + A, 17, obs_dim, E, A, 10)
    _check(oracle, case, tiebreak, [A, E])
