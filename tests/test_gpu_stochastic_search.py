"""The stochastic step-wise kernels (chance_decide of mz_step.cuh; the root, walking select, merged expand + backward and
finish kernels of mz_step_kernels.cuh, launched by mz_stepwise.hip's mzs_*_stochastic entries) in lock-step with the
reference stepper of tests/stochastic_search.py, both fed the same script.  The bar is bit for bit: the selected slot, the
parent-kind flag and the parent embedding at every simulation; the final action, action weights, search value and
depth_sum; every array of the exported A'-wide tree.  The stepper itself is checked on the CPU
(tests/test_stochastic_search_cpu.py)."""
import numpy as np
import pytest
import torch

import scripted_search as ss
import stochastic_search as st

pytestmark = pytest.mark.gpu

# (A, C, B, S): the smallest tree of all; 2048's shape (3 lane slots); A' = 16, a full slot, with B ragged against the 16
# roots of a 256-thread workgroup and the 4 of a wavefront; A' = 17; A itself across a slot; A' = 64, the maximum
SHAPES = [(1, 1, 1, 29), (4, 32, 7, 36), (15, 1, 33, 40), (16, 1, 7, 33), (17, 3, 33, 40), (16, 48, 1, 33)]
# (A, C, B, S, max_depth): at most S / 2 nodes exist within the cut (3; 2 + 4 = 6; 6 + 8 = 14; 4; 16; 17), so in every root
# at least half of the simulations re-expand (asserted).  A cut of 1 or 3 levels lands on a chance node, of 2 on a
# decision node.
REEXPANSION_SHAPES = [(1, 1, 1, 29, 3), (2, 2, 33, 40, 2), (2, 2, 33, 40, 3), (4, 32, 7, 36, 1), (16, 1, 7, 33, 1),
                      (17, 3, 33, 40, 1)]
FAMILIES = ["generic", "discounts", "equal_chance", "extreme_logits", "invalid", "reexpansion"]


class _TreeArrays:
    """The exported tree as NumPy attributes (for check_structure / check_kinds)."""

    def __init__(self, t):
        for k in t._fields:
            setattr(self, k, getattr(t, k).cpu().numpy())


def _run(oracle, family, shape, seed, widths, tiebreak):
    A, C, B, S = shape[:4]
    max_depth = shape[4] if len(shape) > 4 else None
    sc = st.make_script("generic" if family == "invalid" else family, seed, B, A, C, *widths, S,
                        invalid=(family == "invalid"), max_depth=max_depth)
    res = st.drive_hip(oracle, sc, tiebreak=tiebreak)
    t = _TreeArrays(res["out"].search_tree)
    assert t.children_visits.shape == (B, S + 1, A + C) and t.embeddings.shape == (B, S + 1, max(widths))
    inv = np.ones((B, A + C), np.uint8)
    inv[:, :A] = 0 if sc.invalid is None else sc.invalid
    ss.check_structure(t, S, inv, reexpansion=bool(max_depth))
    st.check_kinds(oracle, t, A, reexpansion=bool(max_depth))
    if max_depth:
        share = ss.reexpansion_share(t.node_visits, S)
        assert share.min() >= 0.5, share
    res["handle"].close()
    return sc, t


@pytest.mark.parametrize("tiebreak", [False, True])
@pytest.mark.parametrize("family", FAMILIES)
def test_stochastic_scripted_matches_stepper(oracle, family, tiebreak):
    """Every family on every shape of its list with tie-break noise off and on, the state embedding wider than the
    afterstate embedding (8, 5) and narrower (5, 8) in turn."""
    k = FAMILIES.index(family)
    shapes = REEXPANSION_SHAPES if family == "reexpansion" else SHAPES
    for i, shape in enumerate(shapes):
        widths = (8, 5) if (i + tiebreak + k) % 2 == 0 else (5, 8)
        sc, t = _run(oracle, family, shape, 10 + 2 * k + tiebreak, widths, tiebreak)
        depth = ss.node_depths(t.parents)
        chance = (depth % 2 == 1) & (t.node_visits > 0)
        if family == "discounts" and sc.B >= 3:  # the edges out of chance nodes carry the script's discounts, exact 0 and 1
            d = t.children_discounts[chance][:, sc.A:][t.children_index[chance][:, sc.A:] >= 0]  # among them (the edges
            assert (d == 0).any() and (d == 1).any()  # into chance nodes: reward 0, discount 1 -- check_kinds)
        if family == "equal_chance" and sc.C > 1:  # round-robin over the outcomes, the first index first
            cv = t.children_visits[chance][:, sc.A:]
            assert (cv.max(1) - cv.min(1) <= 1).all() and (np.diff(cv, axis=1) <= 0).all()
        if family == "invalid" and sc.invalid is not None and sc.B > 1:
            assert sc.invalid[0].all() and t.children_visits[0, 0, 0] == sc.S  # all invalid: the argmax over -inf is slot 0


def _nets(A, C, Es, Ea, seed, device):
    """Small torch decision and chance functions (one hidden layer of 16 on [embedding, one-hot]) in mctx's calling
    convention, params = a dict of weight tensors."""
    g = torch.Generator().manual_seed(seed)
    w = lambda *s: (torch.randn(*s, generator=g) / s[0] ** 0.5).to(device)  # noqa: E731
    params = dict(d1=w(Es + A, 16), dl=w(16, C), dv=w(16, 1), de=w(16, Ea), c1=w(Ea + C, 16), cl=w(16, A), cv=w(16, 1),
                  cr=w(16, 1), ce=w(16, Es))
    from muax_amd import ChanceRecurrentFnOutput, DecisionRecurrentFnOutput

    def decision(p, key, action, emb):
        h = torch.tanh(emb @ p["d1"][:Es] + p["d1"][Es:][action.long()])  # [embedding, one-hot action] @ d1
        return DecisionRecurrentFnOutput(h @ p["dl"], (h @ p["dv"])[:, 0]), torch.tanh(h @ p["de"])

    def chance(p, key, outcome, emb):
        h = torch.tanh(emb @ p["c1"][:Ea] + p["c1"][Ea:][outcome.long()])
        out = ChanceRecurrentFnOutput(h @ p["cl"], (h @ p["cv"])[:, 0], (h @ p["cr"])[:, 0],
                                      torch.full((emb.shape[0],), 0.97, device=emb.device))
        return out, torch.tanh(h @ p["ce"])

    return params, decision, chance


def test_policy_adapter_with_torch_nets_eager_and_graph(oracle):
    """StochasticMuZeroPolicy.__call__ with small torch nets, eager and as a captured hipGraph: action and weights == the
    stepper's, driven with the same nets on the rows the search hands out; the returned tree is the decision slice."""
    import muax_amd as mx
    A, C, B, S, Es, Ea, key = 4, 6, 7, 20, 8, 5, [8, 9]
    dev = torch.device("cuda")
    params, decision, chance = _nets(A, C, Es, Ea, 3, dev)
    rng = np.random.default_rng(5)
    root = tuple(torch.from_numpy(x).to(dev) for x in (rng.standard_normal((B, A)).astype(np.float32),
                                                       rng.uniform(-1, 1, B).astype(np.float32),
                                                       rng.uniform(-1, 1, (B, Es)).astype(np.float32)))
    invalid = ss.draw_invalid(rng, B, A, all_invalid_root=False)
    noise = rng.dirichlet([0.3] * A, B).astype(np.float32)
    # the stepper, with the nets evaluated on what it hands out (both functions on all rows, as the search does)
    ref = st.StochasticStepper(oracle, B, A, C, max(Es, Ea), S, *(x.cpu().numpy() for x in root), tiebreak=True, key=key,
                               invalid=invalid, noise=noise)
    with torch.no_grad():
        for sim in range(S):
            p, slot, _ = ref.select(sim)
            pemb = torch.from_numpy(ref.parent_embedding(p)).to(dev)
            ts = torch.from_numpy(slot).to(dev)
            d_out, after = decision(params, None, ts.clamp(0, A - 1), pemb[:, :Es])
            c_out, state = chance(params, None, (ts - A).clamp(0, C - 1), pemb[:, :Ea])
            n = lambda x: x.cpu().numpy()  # noqa: E731
            ref.expand_backup(sim, p, slot, ((n(d_out[0]), n(d_out[1])), n(after), tuple(n(x) for x in c_out), n(state)))
    a_ref, w_ref, _ = ref.finish()
    policy = mx.StochasticMuZeroPolicy()
    for graph in (False, True, True):  # (the second graph call replays the capture)
        with torch.no_grad():
            out = policy(params, key, root, decision_recurrent_fn=decision, chance_recurrent_fn=chance, num_simulations=S,
                         invalid_actions=torch.from_numpy(invalid), dirichlet_noise=torch.from_numpy(noise),
                         with_tree=True, graph=graph)
        assert np.array_equal(a_ref, out.action.cpu().numpy()), graph
        assert np.array_equal(w_ref, out.action_weights.cpu().numpy()), graph
        t = out.search_tree
        assert t.children_visits.shape == (B, S + 1, A) and t.children_index.shape == (B, S + 1, A)
        assert np.array_equal(ref.tree.children_visits[..., :A], t.children_visits.cpu().numpy())
        assert np.array_equal(ref.tree.node_values, t.node_values.cpu().numpy())
    with pytest.raises(ValueError, match="qtransform_by_parent_and_siblings"):
        policy(params, key, root, decision_recurrent_fn=decision, chance_recurrent_fn=chance,
               qtransform="qtransform_completed_by_mix_value")


def test_entries_refuse_the_other_kind_of_handle_and_wide_embeddings():
    from muax_amd import MuZeroSearch, SearchConfig
    B, A, C, E = 3, 2, 2, 4
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    s = MuZeroSearch(B, SearchConfig(A, 5, E, policy="stochastic", num_chance_outcomes=C))
    with pytest.raises(ValueError, match="mzs_root_stochastic"):
        s.root(z(B, A), z(B), z(B, E))
    s.root_stochastic(z(B, A), z(B), z(B, E))
    for call in (lambda: s.select(0), lambda: s.expand_backup(0, z(B), z(B), z(B, A), z(B), z(B, E)), lambda: s.finish()):
        with pytest.raises(ValueError, match="stochastic"):
            call()
    s.close()
    d = MuZeroSearch(B, SearchConfig(A, 5, E, policy="muzero"))
    d.root(z(B, A), z(B), z(B, E))
    for call in (lambda: d.root_stochastic(z(B, A), z(B), z(B, E)), lambda: d.select_stochastic(0),
                 lambda: d.finish_stochastic()):
        with pytest.raises(ValueError, match="does not run the stochastic policy"):
            call()
    d.close()
    with pytest.raises(ValueError, match="narrower than 256"):
        MuZeroSearch(B, SearchConfig(A, 5, 256, policy="stochastic", num_chance_outcomes=C))
    with pytest.raises(ValueError, match="> 64"):
        MuZeroSearch(B, SearchConfig(32, 5, E, policy="stochastic", num_chance_outcomes=33))
    MuZeroSearch(B, SearchConfig(A, 5, 255, policy="stochastic", num_chance_outcomes=C)).close()
