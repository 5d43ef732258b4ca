"""The reference of the stochastic step-wise tests (tests/stochastic_search.py: the stepper built from the C oracle's
primitives) checked on the CPU before the kernels are compared with it (tests/test_gpu_stochastic_search.py): against a
NumPy restatement of the same search written here, and by what the two kinds of node must look like in its trees."""
import numpy as np
import pytest

import scripted_search as ss
import stochastic_search as st

F32 = np.float32
B, A, C, ES, EA, S = 4, 4, 6, 8, 5, 30
# (family, max_depth, actions, outcomes, seed).  The seeds are ones for which NO root has a selection decided by less than
# 1e-4 in the reference (asserted): the comparison then covers every root.  Re-expansion: 2 actions and 2 outcomes put
# 2, 2 + 4 = 6 and 6 + 8 = 14 nodes within a cut of 1, 2 and 3 levels -- at most S / 2, so that in every root at least half
# of the simulations re-expand; the cut lands on a chance node (1, 3) and on a decision node (2).
# (Root 0 of every script has all its actions invalid; a selection at a chance node is decided by p_i / (n_i + 1) against
# p_j / (n_j + 1), which come within 1e-4 of each other often: about one seed in ten leaves all of 4 roots clear, hence the
# small batch and two seeds per case.)
CROSS = [("generic", None, A, C, 6), ("generic", None, A, C, 8), ("discounts", None, A, C, 2), ("discounts", None, A, C, 4),
         ("reexpansion", 1, 2, 2, 1), ("reexpansion", 1, 2, 2, 2), ("reexpansion", 2, 2, 2, 1), ("reexpansion", 2, 2, 2, 3),
         ("reexpansion", 3, 2, 2, 1), ("reexpansion", 3, 2, 2, 3)]


def run_numpy(sc):
    """mctx.stochastic_muzero_policy's search restated on oracle/mz_numpy.py: its Tree and its muzero_action_selection
    (_select) at even depth, p / (visits + 1) at odd depth, the expansion merged by the parent's kind, mctx's backward."""
    from oracle import mz_numpy as mn
    n, AC, E = sc.B, sc.A + sc.C, sc.E
    max_depth = sc.max_depth or sc.S
    t = mn.Tree(n, sc.S + 1, AC, E)
    t.raw_values[:, 0] = t.node_values[:, 0] = sc.root_value
    t.node_visits[:, 0] = 1
    t.embeddings[:, 0, :sc.Es] = sc.root_embedding
    t.root_invalid_actions[:] = 1
    t.root_invalid_actions[:, :sc.A] = 0 if sc.invalid is None else sc.invalid
    t.children_prior_logits[:, 0] = -np.inf
    t.children_prior_logits[:, 0, :sc.A] = mn.root_prior(sc.root_logits, sc.noise, 0.25, sc.invalid)
    br = np.arange(n)
    depth_sum, min_margin = np.zeros(n, np.int64), np.full(n, np.inf)
    for sim in range(sc.S):
        node, parent, action = (np.zeros(n, np.int32) for _ in range(3))
        depth, cont = np.zeros(n, np.int32), np.ones(n, bool)
        level = 0
        while cont.any():
            rows = br[cont]
            if level % 2 == 0:
                a, m = mn._select(t, node[rows], depth, 1.25, 19652.0, None, rows)
            else:
                p = mn.softmax(t.children_prior_logits[rows, node[rows]])
                score = (p / (t.children_visits[rows, node[rows]] + 1).astype(F32)).astype(F32)
                a, srt = score.argmax(-1).astype(np.int32), np.sort(score, -1)
                m = srt[:, -1] - srt[:, -2]
            min_margin[rows] = np.minimum(min_margin[rows], np.where(np.isnan(m), np.inf, m))
            parent[rows], action[rows] = node[rows], a
            nxt = t.children_index[rows, node[rows], a]
            depth[rows] += 1
            go = (nxt != -1) & (depth[rows] < max_depth)
            node[rows[go]] = nxt[go]
            cont[rows[~go]] = False
            level += 1
        depth_sum += depth
        nxt = t.children_index[br, parent, action]
        nxt = np.where(nxt == -1, sim + 1, nxt).astype(np.int32)
        r, d, pl, v, ne = st.merged_row(sc.A, sc.C, E, (depth - 1) % 2 == 0, sc.row(sim))
        t.children_prior_logits[br, nxt] = pl
        t.raw_values[br, nxt] = t.node_values[br, nxt] = v
        t.node_visits[br, nxt] += 1
        t.embeddings[br, nxt] = ne
        t.children_index[br, parent, action] = nxt
        t.children_rewards[br, parent, action], t.children_discounts[br, parent, action] = r, d
        t.parents[br, nxt], t.action_from_parent[br, nxt] = parent, action
        leaf, idx = t.node_values[br, nxt].copy(), nxt.copy()
        while (idx != 0).any():
            rows = br[idx != 0]
            i = idx[rows]
            p, a = t.parents[rows, i], t.action_from_parent[rows, i]
            cnt = t.node_visits[rows, p]
            lv = t.children_rewards[rows, p, a] + t.children_discounts[rows, p, a] * leaf[rows]
            leaf[rows] = lv
            t.node_values[rows, p] = (t.node_values[rows, p] * cnt + lv) / (cnt + F32(1.0))
            t.node_visits[rows, p] = cnt + 1
            t.children_values[rows, p, a] = t.node_values[rows, i]
            t.children_visits[rows, p, a] += 1
            idx[rows] = p
    return dict(tree=t, depth_sum=depth_sum, min_margin=min_margin)


@pytest.mark.parametrize("family,max_depth,acts,outcomes,seed", CROSS)
def test_stepper_and_numpy_restatement_agree(oracle, family, max_depth, acts, outcomes, seed):
    """Integer arrays exactly, floats to 1e-5 max(1, |x|) (the -inf of the padded prior rows in the same places), on EVERY
    root: the seeds are chosen so that the reference decides no selection by less than 1e-4."""
    sc = st.make_script(family, seed, B, acts, outcomes, ES, EA, S, invalid=True, max_depth=max_depth)
    rc = st.run_stepper(oracle, sc, tiebreak=False)
    margin = rc["min_margin"][sc.invalid.sum(1) < acts]  # (an all-invalid root: every score -inf, no margin)
    assert (margin > 1e-4).all(), f"{family}: the reference itself has near ties ({np.sort(margin)[:3]}); choose another seed"
    rn = run_numpy(sc)
    tn = rn["tree"].arrays()
    for k, a in rc["tree"].arrays().items():
        if a.dtype == np.int32:
            assert np.array_equal(a, tn[k]), k
        else:
            fin = np.isfinite(a)
            assert np.array_equal(fin, np.isfinite(tn[k])) and np.array_equal(a[~fin], tn[k][~fin]), k
            ref = tn[k][fin].astype(np.float64)
            err = np.abs(a[fin].astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
            assert err.max() <= 1e-5, (k, float(err.max()))
    assert np.array_equal(rc["depth_sum"], rn["depth_sum"])
    if max_depth:
        assert ss.reexpansion_share(rc["tree"].node_visits, S).min() >= 0.5


@pytest.mark.parametrize("tiebreak", [False, True])
@pytest.mark.parametrize("family,max_depth", [("generic", None), ("discounts", None), ("equal_chance", None),
                                              ("extreme_logits", None), ("reexpansion", 2), ("reexpansion", 3)])
def test_structure_of_the_steppers_tree(oracle, family, max_depth, tiebreak):
    """Chance nodes visit chance slots only and decision nodes action slots only, chance edges carry reward 0 and discount
    1, every chance node's child visits are the D'Hondt apportionment by its stored prior, scripted_search's
    check_structure holds; the finish is over the A actions."""
    acts, outcomes = (2, 2) if max_depth else (3, 5)  # (re-expansion: at most S / 2 nodes within the cut, see CROSS)
    sc = st.make_script(family, 2, 9, acts, outcomes, EA, ES, S, invalid=True, max_depth=max_depth)
    rc = st.run_stepper(oracle, sc, tiebreak=tiebreak)
    t = rc["tree"]
    inv = np.concatenate([sc.invalid, np.ones((sc.B, sc.C), np.uint8)], 1)
    ss.check_structure(t, S, inv, reexpansion=bool(max_depth))
    st.check_kinds(oracle, t, sc.A, reexpansion=bool(max_depth))
    assert rc["action_weights"].shape == (sc.B, sc.A) and np.allclose(rc["action_weights"].sum(1), 1, atol=1e-5)
    assert np.array_equal(rc["search_value"], t.node_values[:, 0])
    assert not np.isnan(np.concatenate([v.ravel() for v in t.arrays().values() if v.dtype == F32])).any()
    # the parent-kind flag is the parity of the selection's depth
    depth = ss.node_depths(t.parents)
    assert np.array_equal(rc["kinds"], 1 - depth[np.arange(sc.B)[None, :], rc["parents"]] % 2)
    if family == "equal_chance":  # equal logits: every chance node deals its visits round-robin, the first outcome first
        cv = t.children_visits[depth % 2 == 1][:, sc.A:]
        assert (cv.max(1) - cv.min(1) <= 1).all() and (np.diff(cv, axis=1) <= 0).all()
    if family == "discounts":
        d = t.children_discounts[t.children_index >= 0]
        assert (d == 0).any() and (d == 1).any()
    if max_depth:
        assert ss.reexpansion_share(t.node_visits, S).min() >= 0.5


def test_chance_apportionment_is_dhondt():
    assert np.array_equal(st.chance_apportionment([0, 0, 0.5, 0.3, 0.2], 10), [0, 0, 5, 3, 2])
    assert np.array_equal(st.chance_apportionment([0.25] * 4, 6), [2, 2, 1, 1])  # ties: the first index
