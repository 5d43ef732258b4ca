"""Stochastic MuZero search (chance nodes) for the step-wise kernels: scripts, a reference stepper and the lock-step
driver (helper, no test functions).

The search is mctx.stochastic_muzero_policy as include/mzsearch.h states it: the MuZero search over A' = A + C slots per
node (A actions, then C chance outcomes), decision nodes at even depth, chance nodes at odd depth.  `StochasticStepper`
is built from the C oracle's primitives only -- root_prior, tree_init, action_scores, softmax, the split / uniform / gumbel
streams, step_expand_backup, summary_sample -- with the walk itself in Python, so the bar of the GPU tests stays bit for
bit.  A *script* fixes both functions' outputs per simulation (scripted_search.py): row `sim` whatever was selected.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np

import scripted_search as ss

F32 = np.float32
FAMILIES = ("generic", "discounts", "equal_chance", "extreme_logits", "reexpansion")
NEG_INF = F32(-np.inf)


@dataclass
class StochasticScript:
    chance_logits: np.ndarray         # [S, B, C]   decision function
    afterstate_value: np.ndarray      # [S, B]
    afterstate_embedding: np.ndarray  # [S, B, Ea]; component 0 is sim + 1 + b / 1024
    action_logits: np.ndarray         # [S, B, A]   chance function
    value: np.ndarray                 # [S, B]
    reward: np.ndarray                # [S, B]
    discount: np.ndarray              # [S, B]
    state_embedding: np.ndarray       # [S, B, Es]; component 0 is sim + 1 + b / 1024
    root_logits: np.ndarray           # [B, A]
    root_value: np.ndarray            # [B]
    root_embedding: np.ndarray        # [B, Es]
    invalid: Optional[np.ndarray] = None  # [B, A] uint8
    noise: Optional[np.ndarray] = None    # [B, A] Dirichlet noise of the root (fraction 0.25)
    max_depth: Optional[int] = None

    @property
    def S(self):
        return self.reward.shape[0]

    @property
    def B(self):
        return self.reward.shape[1]

    @property
    def A(self):
        return self.action_logits.shape[2]

    @property
    def C(self):
        return self.chance_logits.shape[2]

    @property
    def Es(self):
        return self.state_embedding.shape[2]

    @property
    def Ea(self):
        return self.afterstate_embedding.shape[2]

    @property
    def E(self):
        return max(self.Es, self.Ea)

    def row(self, sim):
        """(decision outputs, afterstate embedding, chance outputs, state embedding) of simulation `sim`: the argument
        order of expand_backup_stochastic."""
        return ((self.chance_logits[sim], self.afterstate_value[sim]), self.afterstate_embedding[sim],
                (self.action_logits[sim], self.value[sim], self.reward[sim], self.discount[sim]), self.state_embedding[sim])


def make_script(family, seed, B, A, C, Es, Ea, S, invalid=False, max_depth=None):
    """A seeded script.  generic: rewards, values of mixed sign and size; discounts: per-edge discounts with exact 0 and 1
    (scripted_search.draw_discounts; chance edges carry reward 0 and discount 1 whatever the script says); equal_chance:
    all chance logits equal (round-robin over the outcomes, the first index first); extreme_logits: rows with +-80 and
    -1e9 in both functions' logits; reexpansion: generic numbers for a max_depth cut.  `invalid`: invalid root actions,
    one all-invalid root where B > 1."""
    assert family in FAMILIES, family
    rng = np.random.default_rng([seed, FAMILIES.index(family), B, A, C, Es, Ea, S])
    ae, _ = ss._embeddings(rng, S, B, Ea)
    se, re = ss._embeddings(rng, S, B, Es)
    chance_logits = rng.standard_normal((S, B, C)).astype(F32)
    action_logits = rng.standard_normal((S, B, A)).astype(F32)
    root_logits = rng.standard_normal((B, A)).astype(F32)
    discount = ss.draw_discounts(rng, S, B)
    noise = rng.dirichlet([0.3] * A, B).astype(F32)
    if family == "discounts":
        reward, value, av, root_value = (rng.uniform(-1, 1, s).astype(F32) for s in ((S, B), (S, B), (S, B), (B,)))
    else:
        reward = rng.uniform(-2, 3, (S, B)).astype(F32)
        value, av = rng.uniform(-30, 60, (S, B)).astype(F32), rng.uniform(-30, 60, (S, B)).astype(F32)
        root_value = rng.uniform(-30, 60, B).astype(F32)
        if family == "reexpansion":
            assert max_depth and S >= 4 * max_depth
        if family == "equal_chance":
            chance_logits[:] = F32(0.25)
        if family == "extreme_logits":
            chance_logits, action_logits = ss._extreme_rows(rng, (S, B, C)), ss._extreme_rows(rng, (S, B, A))
            root_logits = ss._extreme_rows(rng, (B, A))
    inv = ss.draw_invalid(rng, B, A) if invalid and A > 1 else None
    c = np.ascontiguousarray
    return StochasticScript(c(chance_logits, F32), c(av, F32), ae, c(action_logits, F32), c(value, F32), c(reward, F32),
                            discount, se, c(root_logits, F32), c(root_value, F32), re, inv, noise, max_depth)


def pad_rows(x, width):
    out = np.zeros(x.shape[:-1] + (width,), F32)
    out[..., :x.shape[-1]] = x
    return out


def merged_row(A, C, E, decision_parent, outs):
    """The expansion's inputs per root, merged by the parent's kind: (reward, discount, prior row [B, A + C], value,
    embedding [B, E]).  decision_parent [B] bool; outs as StochasticScript.row."""
    (cl, av), ae, (al, v, r, d), se = outs
    B = len(decision_parent)
    dp = np.asarray(decision_parent, bool)
    prior = np.full((B, A + C), NEG_INF, F32)
    prior[dp, A:] = cl[dp]
    prior[~dp, :A] = al[~dp]
    reward = np.where(dp, F32(0), r).astype(F32)
    discount = np.where(dp, F32(1), d).astype(F32)
    value = np.where(dp, av, v).astype(F32)
    emb = np.where(dp[:, None], pad_rows(ae, E), pad_rows(se, E)).astype(F32)
    return reward, discount, prior, value, emb


class StochasticStepper:
    """The reference: an A'-wide oracle.Tree, a Python walk over oracle.action_scores (even depth) and oracle.softmax
    (odd depth), step_expand_backup with the merged row, summary_sample on an A-wide copy of the tree.  `min_margin` [B]:
    the smallest gap between the best and the second-best score of any selection (either kind of node)."""

    def __init__(self, oracle, B, A, C, E, S, root_logits, root_value, root_embedding, *, tiebreak=False, max_depth=None,
                 key=(4, 5), invalid=None, noise=None):
        self.o, self.B, self.A, self.C, self.E, self.S = oracle, B, A, C, E, S
        self.tiebreak, self.max_depth = bool(tiebreak), (max_depth if max_depth and max_depth > 0 else S)
        self.tree = oracle.Tree(B, S + 1, A + C, E)
        self.cfg = oracle.SearchCfg(S, tiebreak=int(tiebreak), max_depth=max_depth or 0)
        self.k_sample, _, self.sim_keys = oracle.sim_keys_from_act_key(list(key), S)
        prior = oracle.root_prior(root_logits, noise, 0.25 if noise is not None else 0.0, invalid)
        prior = np.concatenate([prior, np.full((B, C), NEG_INF, F32)], axis=1)
        inv = np.ones((B, A + C), np.uint8)
        inv[:, :A] = 0 if invalid is None else invalid
        oracle.tree_init(self.tree, prior, root_value, pad_rows(np.asarray(root_embedding, F32), E), inv)
        self.depth_sum = np.zeros(B, np.int64)
        self.min_margin = np.full(B, np.inf)
        self.sel_depth = np.zeros(B, np.int32)

    def _scores(self, b, node, depth, sel_key):
        t = self.tree
        if depth % 2 == 0:
            vs, ps = self.o.action_scores(t, self.cfg, b, node)
            score = (vs + ps).astype(F32)
            if self.tiebreak:
                score = (score + F32(1e-7) * self.o.uniform(sel_key, self.A + self.C)).astype(F32)
            if depth == 0:
                score = np.where(t.root_invalid_actions[b] != 0, NEG_INF, score)
            return score
        p = self.o.softmax(t.children_prior_logits[b, node])
        return (p / (t.children_visits[b, node] + 1).astype(F32)).astype(F32)

    def select(self, sim):
        """-> (parent [B], slot [B], parent_is_decision [B])"""
        B, t = self.B, self.tree
        parent, slot = np.zeros(B, np.int32), np.zeros(B, np.int32)
        for b in range(B):
            key = self.o.split(self.sim_keys[sim], B)[b] if self.tiebreak else None
            node, depth = 0, 0
            while True:
                sel = None
                if self.tiebreak:  # one split per level, whether the level uses its key or not
                    key, sel = self.o.split(key, 2)
                score = self._scores(b, node, depth, sel)
                best = int(np.argmax(score))  # the first maximum
                top = np.sort(score)[::-1]
                if len(top) > 1 and np.isfinite(top[1]):
                    self.min_margin[b] = min(self.min_margin[b], float(top[0]) - float(top[1]))
                parent[b], slot[b] = node, best
                depth += 1
                child = t.children_index[b, node, best]
                if child == -1 or depth >= self.max_depth:
                    break
                node = child
            self.sel_depth[b] = depth
        self.depth_sum += self.sel_depth
        return parent, slot, ((self.sel_depth - 1) % 2 == 0).astype(np.int32)

    def parent_embedding(self, parent):
        return self.tree.embeddings[np.arange(self.B), parent]

    def expand_backup(self, sim, parent, slot, outs):
        row = merged_row(self.A, self.C, self.E, (self.sel_depth - 1) % 2 == 0, outs)
        self.o.step_expand_backup(self.tree, sim, parent, slot, *row)

    def decision_tree(self):
        """The A-wide copy of the tree (mctx _mask_tree(tree, num_actions, 'decision'))."""
        t, A = self.tree, self.A
        d = self.o.Tree(t.B, t.N, A, t.E)
        for k, v in t.arrays().items():
            getattr(d, k)[...] = v[..., :A] if k.startswith("children_") else v
        return d

    def finish(self):
        """-> (action [B], action_weights [B, A], search_value [B])"""
        g = self.o.gumbel(self.k_sample, self.B * self.A).reshape(self.B, self.A)
        action, weights = self.o.summary_sample(self.decision_tree(), 1.0, g)
        return action, weights, self.tree.node_values[:, 0].copy()


def script_stepper(oracle, sc, **kw):
    kw.setdefault("max_depth", sc.max_depth)
    return StochasticStepper(oracle, sc.B, sc.A, sc.C, sc.E, sc.S, sc.root_logits, sc.root_value, sc.root_embedding,
                             invalid=sc.invalid, noise=sc.noise, **kw)


def run_stepper(oracle, sc, **kw):
    """The stepper through a script.  Returns dict(tree, action, action_weights, search_value, depth_sum, min_margin,
    slots [S, B], parents [S, B], kinds [S, B])."""
    st = script_stepper(oracle, sc, **kw)
    slots, parents, kinds = (np.zeros((sc.S, sc.B), np.int32) for _ in range(3))
    for sim in range(sc.S):
        parents[sim], slots[sim], kinds[sim] = st.select(sim)
        st.expand_backup(sim, parents[sim], slots[sim], sc.row(sim))
    action, weights, value = st.finish()
    return dict(tree=st.tree, action=action, action_weights=weights, search_value=value, depth_sum=st.depth_sum,
                min_margin=st.min_margin, slots=slots, parents=parents, kinds=kinds)


def chance_apportionment(prob, n):
    """D'Hondt: n visits handed out one at a time to the slot with the largest prob / (visits + 1) in fp32, first index on
    ties -- what a chance node's selections amount to."""
    prob = np.asarray(prob, F32)
    visits = np.zeros(len(prob), np.int32)
    for _ in range(int(n)):
        visits[int(np.argmax((prob / (visits + 1).astype(F32)).astype(F32)))] += 1
    return visits


def check_kinds(oracle, tree, A, reexpansion=False):
    """What the two kinds of node look like in a finished A'-wide tree: odd-depth (chance) nodes have visits and children
    on slots >= A only, even-depth nodes other than the root on slots < A only (the root: its chance slots are masked);
    an edge into a chance node carries reward 0 and discount 1; the child visits of every chance node are the D'Hondt
    apportionment of their sum by the node's stored prior."""
    depth = ss.node_depths(tree.parents)
    nv, cv, ci = tree.node_visits, tree.children_visits, tree.children_index
    for b, n in zip(*np.nonzero(nv > 0)):
        if depth[b, n] % 2 == 1:
            assert (cv[b, n, :A] == 0).all() and (ci[b, n, :A] == -1).all()
            p, a = tree.parents[b, n], tree.action_from_parent[b, n]
            assert a < A and tree.children_rewards[b, p, a] == 0 and tree.children_discounts[b, p, a] == 1
            prob = oracle.softmax(tree.children_prior_logits[b, n])
            assert (prob[:A] == 0).all()
            if not reexpansion:  # (a re-expansion rewrites the prior the earlier visits were dealt by)
                assert np.array_equal(cv[b, n], chance_apportionment(prob, cv[b, n].sum())), (b, n)
        else:
            assert (cv[b, n, A:] == 0).all() and (ci[b, n, A:] == -1).all()
            if n > 0:
                assert tree.action_from_parent[b, n] >= A


# ---------------------------------------------------------------- HIP against the stepper, lock-step

def drive_hip(oracle, sc, *, tiebreak=False, key=(4, 5)):
    """The stochastic step-wise kernels and the stepper driven with the same script, compared as they go (slot, parent
    kind, parent embedding: ==) and at the end (action, action weights, search value, depth_sum, every array of the
    A'-wide tree: ==).  Returns dict(handle, out, ref (the stepper), slots [S, B])."""
    import torch

    from helpers import assert_trees_equal
    from muax_amd import MuZeroSearch, SearchConfig
    dev = "cuda"
    s = MuZeroSearch(sc.B, SearchConfig(sc.A, sc.S, sc.E, tiebreak=tiebreak, max_depth=sc.max_depth, policy="stochastic",
                                        num_chance_outcomes=sc.C, state_embed_dim=sc.Es, afterstate_embed_dim=sc.Ea))
    tt = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    s.root_stochastic(tt(sc.root_logits), tt(sc.root_value), tt(sc.root_embedding), list(key), tt(sc.invalid),
                      tt(sc.noise), 0.25)
    st = script_stepper(oracle, sc, tiebreak=tiebreak, key=key)
    slots = np.zeros((sc.S, sc.B), np.int32)
    for sim in range(sc.S):
        slot, kind, pemb = s.select_stochastic(sim)
        p_ref, s_ref, k_ref = st.select(sim)
        slots[sim] = slot.cpu().numpy()
        bad = np.flatnonzero(s_ref != slots[sim])
        assert bad.size == 0, f"first diverging decision: simulation {sim}, root {bad[:1]}: stepper {s_ref[bad[:1]]} " \
                              f"(from node {p_ref[bad[:1]]}), kernel {slots[sim][bad[:1]]}"
        assert np.array_equal(k_ref, kind.cpu().numpy()), f"parent kind, simulation {sim}"
        assert np.array_equal(st.parent_embedding(p_ref), pemb.cpu().numpy()), f"parent embedding, simulation {sim}"
        (cl, av), ae, (al, v, r, d), se = sc.row(sim)
        s.expand_backup_stochastic(sim, (tt(cl), tt(av)), tt(ae), (tt(al), tt(v), tt(r), tt(d)), tt(se))
        st.expand_backup(sim, p_ref, s_ref, sc.row(sim))
    out = s.finish_stochastic(1.0, None, with_tree=True)
    a_ref, w_ref, v_ref = st.finish()
    assert out.action_weights.shape == (sc.B, sc.A)
    assert np.array_equal(a_ref, out.action.cpu().numpy())
    assert np.array_equal(w_ref, out.action_weights.cpu().numpy())
    assert np.array_equal(v_ref, s.search_value.cpu().numpy())
    assert np.array_equal(st.depth_sum, s.depth_sum.cpu().numpy().astype(np.int64))
    assert_trees_equal(st.tree, out.search_tree, exact_floats=True)
    return dict(handle=s, out=out, ref=st, slots=slots)
