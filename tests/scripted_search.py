"""Scripted recurrent outputs for the step-wise search (helper, no test functions).

The step-wise C-ABI (mzs_root[_gumbel], mzs_select, mzs_expand_backup[_select], mzs_finish, mzs_tree_export) takes the
caller's net outputs where mctx calls recurrent_fn.  A *script* is those outputs fixed before the search starts and
indexed by simulation: recurrent_fn of simulation `sim` returns row `sim` whatever action was selected.  That allows what
a deterministic net cannot produce: per-edge discounts (0 and 1 included), a re-expanded node that receives other numbers
than at its first expansion, exact ties, logits of -1e9, rewards in the thousands.

Three drivers consume one script -- the HIP handle (`drive_hip`, lock-step with the C oracle), the C oracle alone
(`run_oracle`) and the NumPy restatement (`run_numpy`) -- and `expected_last_writes` replays a run's own decisions on the
host to say which script row every edge and node must hold at the end, independently of the oracle.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np

F32 = np.float32
FAMILIES = ("discounts", "generic", "reexpansion", "ties", "extreme_logits", "large", "deep_line")
QT_KIND = {"qtransform_by_parent_and_siblings": 0, "qtransform_completed_by_mix_value": 1}


@dataclass
class Script:
    reward: np.ndarray          # [S, B]
    discount: np.ndarray        # [S, B]
    prior_logits: np.ndarray    # [S, B, A]
    value: np.ndarray           # [S, B]
    next_embedding: np.ndarray  # [S, B, E]; component 0 is sim + 1 + b / 1024: distinct per (sim, root)
    root_logits: np.ndarray     # [B, A]
    root_value: np.ndarray      # [B]
    root_embedding: np.ndarray  # [B, E]; component 0 is b / 1024
    invalid: Optional[np.ndarray] = None  # [B, A] uint8
    noise: Optional[np.ndarray] = None    # [B, A] Dirichlet noise of the MuZero root (fraction 0.25), None: no noise
    gumbel: Optional[np.ndarray] = None   # [B, A] root Gumbel of the Gumbel policy
    max_depth: Optional[int] = None       # the search cut the script was written for (re-expansion family)

    @property
    def S(self):
        return self.reward.shape[0]

    @property
    def B(self):
        return self.reward.shape[1]

    @property
    def A(self):
        return self.prior_logits.shape[2]

    @property
    def E(self):
        return self.next_embedding.shape[2]

    def row(self, sim):
        """RecurrentFnOutput + next embedding of simulation `sim`, the argument order of expand_backup."""
        return (self.reward[sim], self.discount[sim], self.prior_logits[sim], self.value[sim], self.next_embedding[sim])


# ---------------------------------------------------------------- generators

def draw_discounts(rng, S, B):
    """Per (sim, root) one of {0, 1, 0.99, 0.5, uniform[0, 1)} with equal chance (one edge in five exactly 0); the last
    root's are all 0 (every edge terminal) and the one before it all 1, where the batch has that many roots."""
    kind = rng.integers(0, 5, (S, B))
    d = np.choose(kind, [np.zeros((S, B)), np.ones((S, B)), np.full((S, B), 0.99), np.full((S, B), 0.5),
                         rng.uniform(0, 1, (S, B))]).astype(F32)
    if B >= 2:
        d[:, B - 1] = 0.0
    if B >= 3:
        d[:, B - 2] = 1.0
    return d


def draw_invalid(rng, B, A, frac=0.3, all_invalid_root=True):
    """Invalid root actions: each with chance `frac`, one valid action kept per root, and (B > 1) root 0 all invalid."""
    invalid = (rng.uniform(size=(B, A)) < frac).astype(np.uint8)
    invalid[np.arange(B), rng.integers(0, A, B)] = 0
    if all_invalid_root and B > 1:
        invalid[0, :] = 1
    return invalid


def _embeddings(rng, S, B, E):
    ne = rng.uniform(-1, 1, (S, B, E)).astype(F32)
    ne[:, :, 0] = (np.arange(S)[:, None] + 1 + np.arange(B)[None, :] / 1024).astype(F32)
    re = rng.uniform(-1, 1, (B, E)).astype(F32)
    re[:, 0] = (np.arange(B) / 1024).astype(F32)
    return ne, re


def _extreme_rows(rng, shape):
    """Logit rows of four kinds in turn: N(0, 1) with one logit at -1e9 ("masked"); a spread of +-80 with both ends
    present (softmax underflows to exact 0); all -1e9; plain N(0, 1)."""
    A = shape[-1]
    x = rng.standard_normal(shape).astype(F32)
    flat = x.reshape(-1, A)
    for i, row in enumerate(flat):
        k = i % 4
        if k == 0:
            row[rng.integers(0, A)] = -1e9
        elif k == 1:
            row[:] = rng.uniform(-80, 80, A)
            row[rng.integers(0, A)] = 80.0
            if A > 1:
                row[(int(np.argmax(row)) + 1 + rng.integers(0, A - 1)) % A] = -80.0
        elif k == 2:
            row[:] = -1e9
    return flat.reshape(shape)


def make_script(family, seed, B, A, E, S, invalid=False, max_depth=None):
    """A seeded script of one of FAMILIES (all finite float32).  `invalid`: draw invalid root actions (draw_invalid)."""
    assert family in FAMILIES, family
    rng = np.random.default_rng([seed, FAMILIES.index(family), B, A, E, S])
    ne, re = _embeddings(rng, S, B, E)
    logits = rng.standard_normal((S, B, A)).astype(F32)
    root_logits = rng.standard_normal((B, A)).astype(F32)
    discount = draw_discounts(rng, S, B)
    noise = rng.dirichlet([0.3] * A, B).astype(F32)
    gumbel = rng.gumbel(size=(B, A)).astype(F32)
    if family == "discounts":  # order-1 rewards and values: the discounts are what varies
        reward, value, root_value = (rng.uniform(-1, 1, s).astype(F32) for s in ((S, B), (S, B), (B,)))
    elif family in ("generic", "reexpansion", "extreme_logits"):
        reward = rng.uniform(-2, 3, (S, B)).astype(F32)
        value = rng.uniform(-30, 60, (S, B)).astype(F32)
        root_value = rng.uniform(-30, 60, B).astype(F32)
        if family == "reexpansion":
            assert max_depth and S >= 4 * max_depth, "most simulations must re-expand"
        if family == "extreme_logits":
            logits, root_logits = _extreme_rows(rng, (S, B, A)), _extreme_rows(rng, (B, A))
    elif family == "ties":
        # even roots: every reward and value 0; odd roots: every one 0.75.  All logits equal, one discount, no root noise,
        # one constant root-Gumbel row: every sibling comparison of the search is an exact tie.
        c = np.where(np.arange(B) % 2 == 0, 0.0, 0.75).astype(F32)
        reward, value, root_value = np.tile(c, (S, 1)), np.tile(c, (S, 1)), c.copy()
        logits[:], root_logits[:], discount[:] = 0.0, 0.0, 0.5
        noise, gumbel = None, np.full((B, A), 0.25, F32)
    elif family == "large":
        # even roots of order 1e3 .. 1e4 with mixed signs, odd roots of order 1e-3, side by side in one batch
        scale = np.where(np.arange(B) % 2 == 0, 10.0 ** rng.uniform(3, 4, B), 1e-3)
        reward, value = ((scale * rng.uniform(-1, 1, (S, B))).astype(F32) for _ in range(2))
        root_value = (scale * rng.uniform(-1, 1, B)).astype(F32)
    else:  # deep_line: +20 on action 0 at every node, the search digs one line; rewards and discounts vary along it
        reward = rng.uniform(-2, 3, (S, B)).astype(F32)
        value, root_value = rng.uniform(-5, 5, (S, B)).astype(F32), rng.uniform(-5, 5, B).astype(F32)
        logits[..., 0], root_logits[..., 0] = logits[..., 0] * F32(0.1) + F32(20), root_logits[..., 0] * F32(0.1) + F32(20)
        noise = None
    inv = draw_invalid(rng, B, A) if invalid and A > 1 and family != "deep_line" else None
    return Script(np.ascontiguousarray(reward, F32), discount, np.ascontiguousarray(logits, F32),
                  np.ascontiguousarray(value, F32), ne, np.ascontiguousarray(root_logits, F32),
                  np.ascontiguousarray(root_value, F32), re, inv, noise, gumbel, max_depth)


# ---------------------------------------------------------------- the C oracle, stepped

class OracleStepper:
    """tree_init, then per simulation step_select / gumbel_step_select and step_expand_backup, then summary_sample /
    gumbel_finish: the C oracle as the step-wise kernels are driven.  policy "muzero": `noise` is the root's Dirichlet
    noise (fraction 0.25) and the final action samples with the Gumbel row of split(key, 3)[0]; policy "gumbel": `gumbel`
    is the root Gumbel (None: drawn from split(key, 2)[1])."""

    def __init__(self, oracle, B, A, E, S, root_logits, root_value, root_embedding, *, policy="muzero", tiebreak=False,
                 max_depth=None, key=(4, 5), invalid=None, noise=None, gumbel=None,
                 qtransform="qtransform_by_parent_and_siblings", max_considered=16):
        self.o, self.B, self.A, self.S, self.policy = oracle, B, A, S, policy
        self.tree = oracle.Tree(B, S + 1, A, E)
        self.depth_sum = np.zeros(B, np.int64)
        if policy == "gumbel":
            self.kind, self.maxc = QT_KIND[qtransform], max_considered
            self.cfg = oracle.SearchCfg(S, max_depth=max_depth or 0)
            self.gumbel = gumbel if gumbel is not None else oracle.gumbel(oracle.split(list(key), 2)[1], B * A).reshape(B, A)
            prior = oracle.mask_root_logits(root_logits, invalid)
        else:
            self.cfg = oracle.SearchCfg(S, tiebreak=int(tiebreak), max_depth=max_depth or 0)
            self.k_sample, _, self.sim_keys = oracle.sim_keys_from_act_key(list(key), S)
            prior = oracle.root_prior(root_logits, noise, 0.25 if noise is not None else 0.0, invalid)  # (no noise: no mix)
        oracle.tree_init(self.tree, prior, root_value, root_embedding, invalid)

    def select(self, sim):
        if self.policy == "gumbel":
            p, a, d = self.o.gumbel_step_select(self.tree, self.cfg, self.gumbel, self.kind, self.maxc)
        else:
            p, a, d = self.o.step_select(self.tree, self.cfg, sim, self.sim_keys[sim])
        self.depth_sum += d
        return p, a

    def parent_embedding(self, parent):
        return self.tree.embeddings[np.arange(self.B), parent]

    def expand_backup(self, sim, parent, action, outs):
        self.o.step_expand_backup(self.tree, sim, parent, action, *outs)

    def finish(self):
        if self.policy == "gumbel":
            return self.o.gumbel_finish(self.tree, self.gumbel, self.kind)
        g = self.o.gumbel(self.k_sample, self.B * self.A).reshape(self.B, self.A)
        return self.o.summary_sample(self.tree, 1.0, g)


def _script_stepper(oracle, sc, **kw):
    kw.setdefault("max_depth", sc.max_depth)
    policy = kw.get("policy", "muzero")
    return OracleStepper(oracle, sc.B, sc.A, sc.E, sc.S, sc.root_logits, sc.root_value, sc.root_embedding,
                         invalid=sc.invalid, noise=sc.noise if policy == "muzero" else None,
                         gumbel=sc.gumbel if policy == "gumbel" else None, **kw)


def run_oracle(oracle, sc, **kw):
    """The C oracle stepped through the script.  Returns dict(tree, action, action_weights, depth_sum, actions [S, B],
    parents [S, B])."""
    st = _script_stepper(oracle, sc, **kw)
    actions, parents = np.zeros((sc.S, sc.B), np.int32), np.zeros((sc.S, sc.B), np.int32)
    for sim in range(sc.S):
        parents[sim], actions[sim] = st.select(sim)
        st.expand_backup(sim, parents[sim], actions[sim], sc.row(sim))
    action, weights = st.finish()
    return dict(tree=st.tree, action=action, action_weights=weights, depth_sum=st.depth_sum, actions=actions,
                parents=parents)


# ---------------------------------------------------------------- the NumPy restatement

def run_numpy(oracle, sc, *, policy="muzero", max_depth=None, qtransform="qtransform_by_parent_and_siblings",
              max_considered=16):
    """oracle/mz_numpy.py's search / gumbel_search with the script as its recurrent_fn (no tie-break noise).  Returns
    dict(tree, action, action_weights, depth_sum, min_margin)."""
    from oracle import mz_numpy as mn
    B, A, E, S = sc.B, sc.A, sc.E, sc.S
    max_depth = max_depth or sc.max_depth
    t = mn.Tree(B, S + 1, A, E)
    t.raw_values[:, 0] = t.node_values[:, 0] = sc.root_value
    t.node_visits[:, 0] = 1
    t.embeddings[:, 0] = sc.root_embedding
    if sc.invalid is not None:
        t.root_invalid_actions[:] = sc.invalid
    calls = []

    def rec(action, emb):
        calls.append(1)
        return sc.row(len(calls) - 1)

    if policy == "gumbel":
        mode = "mix" if QT_KIND[qtransform] == 1 else "pas"
        t.children_prior_logits[:, 0] = oracle.mask_root_logits(sc.root_logits, sc.invalid)
        margin = np.full(B, np.inf)
        dsum = mn.gumbel_search(t, rec, S, sc.gumbel, max_considered, mode, max_depth, min_margin=margin)
        action, weights = mn.gumbel_finish(t, sc.gumbel, mode)
    else:
        t.children_prior_logits[:, 0] = mn.root_prior(sc.root_logits, sc.noise, 0.25, sc.invalid)
        margin, dsum = mn.search(t, rec, S, max_depth)
        action, weights = None, None  # (the final sample draws from a key: compared C against HIP, not here)
    return dict(tree=t, action=action, action_weights=weights, depth_sum=dsum, min_margin=margin)


# ---------------------------------------------------------------- HIP against the C oracle, lock-step

def drive_hip(oracle, B, A, E, S, root_out, rec, *, policy="muzero", tiebreak=False, max_depth=None, key=(4, 5),
              invalid=None, noise=None, gumbel=None, qtransform="qtransform_by_parent_and_siblings", max_considered=16,
              fused_select=False, check_parent_embedding=True):
    """The step-wise kernels and the C oracle driven with the same net outputs, compared as they go and at the end.

    root_out = (prior_logits [B, A], value [B], embedding [B, E]) and rec(sim, action, parent_embedding) ->
    (reward, discount, prior_logits, value, next_embedding), all torch tensors.  fused_select: mzs_expand_backup_select
    (the next selection in the expand + backward launch) instead of mzs_select + mzs_expand_backup.  Asserts at every
    simulation the selected action (and the parent embedding), at the end the action, the action weights, every tree array
    bit for bit and depth_sum.  Returns dict(handle, out, tree (the oracle's), actions [S, B], parent_emb [S, B, E])."""
    import torch

    from helpers import assert_trees_equal
    from muax_amd import MuZeroSearch, SearchConfig
    pl, v, emb = root_out
    s = MuZeroSearch(B, SearchConfig(A, S, E, tiebreak=tiebreak, max_depth=max_depth, policy=policy, qtransform=qtransform,
                                     max_num_considered_actions=max_considered))
    inv = None if invalid is None else torch.from_numpy(invalid)
    if policy == "gumbel":
        s.root_gumbel(pl, v, emb, list(key), inv, None if gumbel is None else torch.from_numpy(gumbel))
    else:
        s.root(pl, v, emb, list(key), inv, None if noise is None else torch.from_numpy(noise), 0.25)
    st = OracleStepper(oracle, B, A, E, S, pl.cpu().numpy(), v.cpu().numpy(), emb.cpu().numpy(), policy=policy,
                       tiebreak=tiebreak, max_depth=max_depth, key=key, invalid=invalid, noise=noise, gumbel=gumbel,
                       qtransform=qtransform, max_considered=max_considered)
    actions, pembs = np.zeros((S, B), np.int32), np.zeros((S, B, E), F32)
    nxt = None
    for sim in range(S):
        action, pemb = nxt if fused_select and sim > 0 else s.select(sim)
        p_ref, a_ref = st.select(sim)
        actions[sim], pembs[sim] = action.cpu().numpy(), pemb.cpu().numpy()
        bad = np.flatnonzero(a_ref != actions[sim])
        assert bad.size == 0, f"first diverging decision: simulation {sim}, root {bad[:1]}: oracle {a_ref[bad[:1]]} " \
                              f"(from node {p_ref[bad[:1]]}), kernel {actions[sim][bad[:1]]}"
        if check_parent_embedding:
            assert np.array_equal(st.parent_embedding(p_ref), pembs[sim]), f"parent embedding, simulation {sim}"
        outs = rec(sim, action, pemb)
        if fused_select:
            nxt = s.expand_backup_select(sim, *outs)
            assert (nxt is None) == (sim == S - 1)
        else:
            s.expand_backup(sim, *outs)
        st.expand_backup(sim, p_ref, a_ref, [o.cpu().numpy() for o in outs])
    out = s.finish(1.0, None, with_tree=True) if policy == "muzero" else s.finish(with_tree=True)
    a_ref, w_ref = st.finish()
    assert np.array_equal(a_ref, out.action.cpu().numpy())
    assert np.array_equal(w_ref, out.action_weights.cpu().numpy())
    assert_trees_equal(st.tree, out.search_tree, exact_floats=True)
    assert np.array_equal(st.depth_sum, s.depth_sum.cpu().numpy().astype(np.int64))
    return dict(handle=s, out=out, tree=st.tree, actions=actions, parent_emb=pembs)


def script_root_and_rec(sc, device="cuda"):
    """(root_out, rec) of a script as torch tensors on `device`, for drive_hip and MuZeroSearch.search(): rec(sim, ...)
    returns row `sim`; `rec.counting()` is a two-argument recurrent_fn that returns the rows in call order."""
    import torch
    rows = [tuple(torch.from_numpy(np.ascontiguousarray(x)).to(device) for x in sc.row(sim)) for sim in range(sc.S)]
    root_out = tuple(torch.from_numpy(x).to(device) for x in (sc.root_logits, sc.root_value, sc.root_embedding))

    def rec(sim, action, pemb):
        return rows[sim]

    def counting():
        calls = []

        def fn(action, pemb):
            calls.append(1)
            return rows[len(calls) - 1]
        return fn

    rec.counting = counting
    return root_out, rec


def drive_hip_script(oracle, sc, **kw):
    """drive_hip on a script (root noise / root Gumbel / invalid actions / max_depth taken from it)."""
    root_out, rec = script_root_and_rec(sc)
    policy = kw.get("policy", "muzero")
    kw.setdefault("max_depth", sc.max_depth)
    return drive_hip(oracle, sc.B, sc.A, sc.E, sc.S, root_out, rec, invalid=sc.invalid,
                     noise=sc.noise if policy == "muzero" else None, gumbel=sc.gumbel if policy == "gumbel" else None, **kw)


# ---------------------------------------------------------------- what the script itself says the tree must hold

def node_depths(parents):
    """Depth of every node from the parents array [B, N] (unexpanded nodes: 0)."""
    B, N = parents.shape
    depth = np.zeros((B, N), np.int64)
    for k in range(1, N):
        p = parents[:, k]
        depth[:, k] = np.where(p >= 0, depth[np.arange(B), np.maximum(p, 0)] + 1, 0)
    return depth


def expected_last_writes(sc, actions, parent_emb):
    """Replays a run's own decisions -- the action of every simulation and the parent embedding select() handed out,
    whose component 0 names the simulation that last wrote the parent node -- and returns what the script says the final
    tree holds: children_rewards / children_discounts [B, N, A] (the row of the LAST simulation that expanded the edge, 0
    elsewhere), raw_values [B, N], children_prior_logits [B, N, A] and embeddings [B, N, E] of the expanded nodes (the row
    of the last simulation that expanded the node), `expanded` [B, N] (how often) and `reexpanded` (any node twice)."""
    S, B, A, E = sc.S, sc.B, sc.A, sc.E
    N = S + 1
    cr, cd = np.zeros((B, N, A), F32), np.zeros((B, N, A), F32)
    raw, cpl, emb = np.zeros((B, N), F32), np.zeros((B, N, A), F32), np.zeros((B, N, E), F32)
    expanded = np.zeros((B, N), np.int32)
    raw[:, 0], emb[:, 0] = sc.root_value, sc.root_embedding
    for b in range(B):
        child, node_of_sim = {}, {-1: 0}
        for sim in range(S):
            writer = int(round(float(parent_emb[sim, b, 0]) - b / 1024)) - 1
            parent, a = node_of_sim[writer], int(actions[sim, b])
            node = child.setdefault((parent, a), sim + 1)
            node_of_sim[sim] = node
            cr[b, parent, a], cd[b, parent, a] = sc.reward[sim, b], sc.discount[sim, b]
            raw[b, node], cpl[b, node], emb[b, node] = sc.value[sim, b], sc.prior_logits[sim, b], sc.next_embedding[sim, b]
            expanded[b, node] += 1
    return dict(children_rewards=cr, children_discounts=cd, raw_values=raw, children_prior_logits=cpl, embeddings=emb,
                expanded=expanded, reexpanded=bool((expanded > 1).any()))


def reexpansion_share(node_visits, S):
    """Per root, the share of the S simulations that re-expanded an existing node (each of the others created one)."""
    return 1.0 - (np.asarray(node_visits)[:, 1:] > 0).sum(1) / S


def backup_float64(tree, S):
    """node_values recomputed in float64 from the tree's own parents, action_from_parent, children_rewards,
    children_discounts and raw_values, for a search WITHOUT re-expansion (simulation k expanded node k + 1): the
    discounted return every simulation delivered to each ancestor, and the running means."""
    B = tree.parents.shape[0]
    total = tree.raw_values.astype(np.float64).copy()  # a node's own raw value is the first term of its mean
    count = np.ones_like(total)
    for b in range(B):
        par, afp = tree.parents[b], tree.action_from_parent[b]
        r, d = tree.children_rewards[b].astype(np.float64), tree.children_discounts[b].astype(np.float64)
        for sim in range(S):
            n = sim + 1
            g = float(tree.raw_values[b, n])
            while n != 0:
                p = par[n]
                g = r[p, afp[n]] + d[p, afp[n]] * g
                total[b, p] += g
                count[b, p] += 1
                n = p
    return total / count


def check_structure(tree, S, invalid=None, reexpansion=False):
    """Structural invariants of a finished search tree (NumPy arrays): root visits S + 1, visit sums, parent / child
    consistency, masked root actions unvisited.  `reexpansion` (a max_depth cut): every re-expansion of a node counts as
    a visit of it (mctx update_tree_node) that none of its children saw."""
    nv, cv, ci, par, afp = tree.node_visits, tree.children_visits, tree.children_index, tree.parents, tree.action_from_parent
    assert (nv[:, 0] == S + 1).all()
    assert ((cv.sum(-1) <= nv - 1) if reexpansion else (cv.sum(-1) == nv - 1))[nv > 0].all()
    assert (cv[nv == 0] == 0).all() and (ci[nv == 0] == -1).all()
    assert (cv[:, 0].sum(-1) == S).all()
    b, n, a = np.nonzero(ci >= 0)
    c = ci[b, n, a]
    assert (par[b, c] == n).all() and (afp[b, c] == a).all() and (cv[b, n, a] == nv[b, c]).all()
    assert ((ci >= 0) == (cv > 0)).all()
    if invalid is not None:
        some_valid = invalid.sum(1) < invalid.shape[1]  # (an all-invalid root: mctx's argmax over -inf picks action 0)
        assert (cv[:, 0][some_valid][invalid[some_valid] != 0] == 0).all()
