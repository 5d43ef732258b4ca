"""Numeric edge cases of the Stochastic MuZero search kernels (helper, plain Python and NumPy, no test functions).

Every case is an `EdgeCase` (name, shape, weights, root, invalid, noise, gumbel, options): the 28 weight arrays of the
default stochastic MLP family, the RootFnOutput, the optional mask / Dirichlet noise / Gumbel row and the search options,
built on stochastic_mlp_reference.random_weights so that ONE property is driven to an edge -- exact ties, one-ulp margins,
logits near an exponent limit, a decode on the last support bin, a next state of range 0 or 2**-k, rewards that are
zeros of either sign, masks that leave nothing or one action, temperatures of 0 / 1e-3 / 50, Dirichlet fractions of 0 and 1, a max_depth
cut on either kind of node.  `reference(name)` runs the case once through `EdgeStepper`: tests/stochastic_search.py's
StochasticStepper fed by StochasticMlpReference, subclassed only to take the fraction / temperature / Gumbel row of the
case and to COUNT what its selections looked like (the arithmetic is the parent class's).  The counters are what
tests/test_stochastic_edges_cpu.py asserts, so that a case name is a fact about the reference and not a hope;
tests/test_gpu_stochastic_edges.py compares the kernels with the same runs, == on the uint32 views.

The family's search entries read no encoder / codebook array (those belong to the training step), so the shifted rows are
the policy head's, the chance head's, the root's prior_logits and the three support heads'.
"""
import functools
from dataclasses import dataclass
from typing import NamedTuple, Optional

import numpy as np

import scripted_search as ss
import stochastic_mlp_reference as smr
import stochastic_search as st

F32 = np.float32
H = smr.H
KEY = (4, 5)
# (A, C, E, support, B, S): the three-launch route's smallest case; 2048's shape; 58 slots over four 16-lane rows, F = 63,
# E = 64 (every lane), B % waves != 0
SHAPES = [(4, 3, 5, 8, 4, 12), (4, 32, 16, 10, 7, 24), (18, 40, 64, 31, 5, 12)]
MI355X_CUS = 256
BIG = F32(1e4)  # exp(x - 1e4) == 0 in fp32 for every head output of order 1: all of a softmax's mass on one entry


@dataclass(frozen=True)
class Options:
    tiebreak: bool = False
    max_depth: Optional[int] = None
    temperature: float = 1.0
    fraction: float = 0.25  # used when the case has a noise array; without one the root mixes nothing
    discount: float = 0.97


class EdgeCase(NamedTuple):
    name: str
    shape: tuple       # (A, C, E, support, B, S)
    weights: dict
    root: tuple        # (prior_logits [B, A], value [B], embedding [B, E])
    invalid: Optional[np.ndarray]
    noise: Optional[np.ndarray]
    gumbel: Optional[np.ndarray]
    options: Options
    facts: dict        # what the builder did, for the CPU test's conditions (raised index, k, shifted heads, ...)


def _oracle():
    from oracle import pyoracle as oracle
    oracle.build()
    return oracle


# ---------------------------------------------------------------- building blocks
def _generic(shape, salt=0):
    """(rng, root, noise) as the existing stochastic tests draw them."""
    A, C, E, support, B, S = shape
    rng = np.random.default_rng([7, A, C, E, B, S, salt])
    root = (rng.standard_normal((B, A)).astype(F32), rng.uniform(-3, 3, B).astype(F32), rng.uniform(0, 1, (B, E)).astype(F32))
    return rng, root, rng.dirichlet([0.3] * A, B).astype(F32)


def _weights(shape):
    A, C, E, support = shape[:4]
    return smr.random_weights(11, A, C, E, support)


def _constant_head(w, head, row):
    """The head's output layer zeroed: its output is `row` whatever the input (an fma chain over zeros, then the bias)."""
    w[f"{head}_w2"] = np.zeros_like(w[f"{head}_w2"])
    w[f"{head}_b2"] = np.array(np.broadcast_to(np.asarray(row, F32), w[f"{head}_b2"].shape), F32)  # (a writable copy)


def tied_value(support):
    """What a support head with equal logits decodes to (the oracle's own arithmetic)."""
    o = _oracle()
    F = 2 * support + 1
    return F32(o.support_to_scalar(o.softmax(np.ones(F, F32)), support))


def _all_ties_weights(shape):
    """Policy, chance, value, afterstate-value and reward heads: output layers zero, biases 1.0 across the row."""
    w = _weights(shape)
    for head in ("pp", "ac", "pv", "av", "cr"):
        _constant_head(w, head, 1.0)
    return w


def _all_ties_root(shape, rng):
    """Equal logits.  Even roots carry the tied value itself: no visited child ever scores above an unvisited one, the
    search stays broad.  Odd roots carry the tied value - 1: a visited child (value score 1) beats its unvisited siblings,
    the search goes down one line and meets the chance nodes whatever the number of actions."""
    A, C, E, support, B, S = shape
    value = np.full(B, tied_value(support), F32)
    value[1::2] -= F32(1.0)
    return np.ones((B, A), F32), value, rng.uniform(0, 1, (B, E)).astype(F32)


def range_row(rng, E, k):
    """E values within 0.25 -+ 2**-(k + 1), both ends present: max - min == 2**-k exactly."""
    lo, hi = F32(0.25) - F32(2.0 ** -(k + 1)), F32(0.25) + F32(2.0 ** -(k + 1))
    row = rng.choice(np.array([lo, F32(0.25), hi], F32), E).astype(F32)
    row[0], row[-1] = lo, hi
    assert E >= 2 and F32(row.max() - row.min()) == F32(2.0 ** -k) and lo < F32(0.25) < hi
    return row


def outlier_row(rng, E):
    """Order 1e-3 everywhere and one element at 1e6."""
    row = (rng.uniform(0, 1, E) * 1e-3).astype(F32)
    row[int(rng.integers(0, E))] = F32(1e6)
    return row


def edge_masks(rng, B, A):
    """draw_invalid's mask (root 0: every action invalid) with root 1 left a single valid action and root 2 only its
    highest indices."""
    invalid = ss.draw_invalid(rng, B, A)
    assert B >= 3 and invalid[0].all()
    invalid[1, :] = 1
    invalid[1, 1 % A] = 0
    invalid[2, :] = 1
    invalid[2, A - max(1, A // 3):] = 0
    return invalid


# ---------------------------------------------------------------- the cases
def _all_ties(name, shape, tiebreak, max_depth=None, masked=False, temperature=1.0):
    rng, _, _ = _generic(shape, 1)
    A, B = shape[0], shape[4]
    # no Dirichlet noise (it would untie the root); without tie-break noise a constant Gumbel row, so that the final
    # argmax is among tied visit counts as well
    gumbel = None if tiebreak else np.full((B, A), 0.25, F32)
    return EdgeCase(name, shape, _all_ties_weights(shape), _all_ties_root(shape, rng), edge_masks(rng, B, A) if masked else None,
                    None, gumbel, Options(tiebreak=tiebreak, max_depth=max_depth, temperature=temperature),
                    dict(family="all_ties"))


def _chance_ties_only(name, shape, tiebreak):
    rng, root, noise = _generic(shape, 2)
    w = _weights(shape)
    C = shape[1]
    _constant_head(w, "ac", (np.arange(C) // 2).astype(F32) * F32(0.125))  # [0, 0, 1, 1, 2, 2, ...] / 8
    # the last root alone also starts on a tie at its decision node: its two best actions share logit and noise
    logits, noise = root[0].copy(), noise.copy()
    logits[-1, :2] = logits[-1].max() + F32(0.5)
    noise[-1, :2] = F32(0.5) * (noise[-1, 0] + noise[-1, 1])
    root = (logits,) + root[1:]
    return EdgeCase(name, shape, w, root, None, noise, None, Options(tiebreak=tiebreak), dict(family="chance_ties_only"))


def _small_margins(name, shape, last):
    """all_ties with ONE output bias of the policy head, the chance head and the root's logits raised by one ulp."""
    rng, _, _ = _generic(shape, 3)
    A, C, _, _, B, _ = shape
    w = _all_ties_weights(shape)
    up = np.nextafter(F32(1.0), F32(2.0))
    ia, ic = (A - 1, C - 1) if last else (0, 0)
    w["pp_b2"][ia] = up
    w["ac_b2"][ic] = up
    root = _all_ties_root(shape, rng)
    root[0][:, ia] = up
    return EdgeCase(name, shape, w, root, None, None, np.full((B, A), 0.25, F32), Options(),
                    dict(family="small_margins", raised_action=ia, raised_slot=A + ic))


def _shifted_logits(name, shape, shift):
    rng, root, noise = _generic(shape, 4)
    w = _weights(shape)
    for head in ("pp", "ac"):
        w[f"{head}_b2"] = (w[f"{head}_b2"] + F32(shift)).astype(F32)
    root = ((root[0] + F32(shift)).astype(F32),) + root[1:]
    return EdgeCase(name, shape, w, root, None, noise, None, Options(), dict(family="shifted_logits", shift=float(shift)))


def _shifted_support(name, shape, high):
    """All mass of the three support heads on bin 0 / bin 2 * support: every decode is -+support before inv_scaling."""
    rng, root, noise = _generic(shape, 5)
    w = _weights(shape)
    support = shape[3]
    k = 2 * support if high else 0
    for head in ("pv", "av", "cr"):
        w[f"{head}_b2"][k] += BIG
    sign = F32(1.0) if high else F32(-1.0)
    edge = F32(sign * _oracle().inv_scaling(F32(support)))
    root = (root[0], np.full_like(root[1], edge), root[2])
    return EdgeCase(name, shape, w, root, None, noise, None, Options(), dict(family="shifted_support", decode=edge))


def _flat_states(name, shape, kind, heads, k=None):
    """The next-state heads in `heads` ('ad': afterstate dynamics, 'cn': dynamics) give, before the normalisation,
    kind 'flat': E equal elements; 'range': max - min == 2**-k around 0.25; 'outlier': one element far from the rest."""
    rng, root, noise = _generic(shape, 6)
    w = _weights(shape)
    E = shape[2]
    rows = {}
    for head in heads:
        rows[head] = {"flat": lambda: np.full(E, 0.375, F32), "range": lambda: range_row(rng, E, k),
                      "outlier": lambda: outlier_row(rng, E)}[kind]()
        _constant_head(w, head, rows[head])
    return EdgeCase(name, shape, w, root, None, noise, None, Options(), dict(family="flat_states", kind=kind, k=k, rows=rows))


def _zero_rewards(name, shape, discount):
    """Reward logits symmetric about the centre bin (w2 zero, a mirrored bias row): the expectation over the support is
    exactly 0, and the decoded reward is the zero that inv_scaling makes of it.  That zero is -0.0: muax's inverse scaling
    is sign(x) * (e * e - 1) with e * e - 1 < 0 at x = 0 in fp32, so NO reward head output decodes to +0.0, and the tree
    holds both zeros -- +0.0 on the edges into chance nodes (no reward there), -0.0 on the edges out of them."""
    rng, root, noise = _generic(shape, 7)
    w = _weights(shape)
    support = shape[3]
    o = _oracle()
    while True:  # mirrored terms cancel in exact arithmetic; keep a row for which the oracle's own summation order does too
        half = rng.standard_normal(support + 1).astype(F32)
        row = np.concatenate([half, half[:-1][::-1]])
        if o.support_to_scalar(o.softmax(row), support) == 0.0:
            break
    _constant_head(w, "cr", row)
    return EdgeCase(name, shape, w, root, None, noise, None, Options(discount=discount), dict(family="zero_rewards"))


def _masks_generic(name, shape, tiebreak):
    rng, root, noise = _generic(shape, 8)
    return EdgeCase(name, shape, _weights(shape), root, edge_masks(rng, shape[4], shape[0]), noise, None,
                    Options(tiebreak=tiebreak), dict(family="masks"))


def _temperature(name, shape, temperature, one_hot=False):
    """one_hot: +1e4 on one root logit per root and no noise, so that every visit goes to that action."""
    rng, root, noise = _generic(shape, 9)
    A, B = shape[0], shape[4]
    if one_hot:
        logits = root[0].copy()
        logits[np.arange(B), np.arange(B) % A] += BIG
        root, noise = (logits,) + root[1:], None
    return EdgeCase(name, shape, _weights(shape), root, None, noise, None, Options(temperature=temperature),
                    dict(family="temperature", one_hot=one_hot))


def _noise(name, shape, fraction, with_noise, gumbel=False, tiebreak=False):
    rng, root, noise = _generic(shape, 10)
    A, B = shape[0], shape[4]
    if with_noise and fraction == 1.0:
        noise[0, 0] = 0.0  # a noise entry of exactly 0 at fraction 1: the clamp to FLT_MIN before the log
        noise[0] /= noise[0].sum(dtype=F32)
    g = rng.gumbel(size=(B, A)).astype(F32) if gumbel else None
    return EdgeCase(name, shape, _weights(shape), root, None, noise if with_noise else None, g,
                    Options(fraction=fraction, tiebreak=tiebreak), dict(family="noise"))


def more_roots_batch(num_cus=MI355X_CUS):
    """One root more than a full first round of the small plan's launch: waves * resident workgroups + 1."""
    from muax_amd import search
    A, C, E, support = SHAPES[0][:4]
    pl = search.stochastic_plan(A, C, E, support, 3)
    assert pl is not None and pl["roots_per_cu"] % pl["waves"] == 0
    return pl["waves"] * (pl["roots_per_cu"] // pl["waves"]) * num_cus + 1


def more_roots_case(B, tiebreak):
    """The small shape at S = 3 with B roots.  Without tie-break noise and with an injected Gumbel row a root's result
    depends on nothing but its own row, so `rows_of` gives a reference for any subset of roots."""
    shape = SHAPES[0][:4] + (B, 3)
    rng, root, noise = _generic(shape, 11)
    gumbel = None if tiebreak else rng.gumbel(size=(B, shape[0])).astype(F32)
    return EdgeCase(f"more_roots_than_one_round-{B}-{int(tiebreak)}", shape, _weights(shape), root, None, noise, gumbel,
                    Options(tiebreak=tiebreak), dict(family="more_roots"))


def rows_of(case, rows):
    """The case cut to the roots `rows` (a list): for a case whose roots do not depend on their batch index."""
    assert not case.options.tiebreak and case.gumbel is not None
    cut = lambda x: None if x is None else np.ascontiguousarray(x[rows])  # noqa: E731
    shape = case.shape[:4] + (len(rows), case.shape[5])
    return case._replace(shape=shape, root=tuple(cut(x) for x in case.root), invalid=cut(case.invalid), noise=cut(case.noise),
                         gumbel=cut(case.gumbel))


S0, S1, S2 = SHAPES
_BUILDERS = {
    # every prior and chance probability equal, every value and reward one number
    "all_ties-s0": (_all_ties, S0, False), "all_ties-s1": (_all_ties, S1, False), "all_ties-s2": (_all_ties, S2, False),
    "all_ties_noise-s0": (_all_ties, S0, True), "all_ties_noise-s1": (_all_ties, S1, True),
    "all_ties_noise-s2": (_all_ties, S2, True),
    # chance logits equal in pairs, everything else generic (tie-break noise must not reach the chance nodes)
    "chance_ties_only-s0": (_chance_ties_only, S0, False), "chance_ties_only-s1": (_chance_ties_only, S1, False),
    "chance_ties_only-s2": (_chance_ties_only, S2, False), "noisy_decisions_chance_ties-s1": (_chance_ties_only, S1, True),
    "small_margins_first-s0": (_small_margins, S0, False), "small_margins_last-s0": (_small_margins, S0, True),
    "small_margins_first-s1": (_small_margins, S1, False), "small_margins_last-s1": (_small_margins, S1, True),
    "small_margins_first-s2": (_small_margins, S2, False), "small_margins_last-s2": (_small_margins, S2, True),
    "shifted_logits_p80-s0": (_shifted_logits, S0, 80.0), "shifted_logits_m80-s0": (_shifted_logits, S0, -80.0),
    "shifted_logits_p1e4-s0": (_shifted_logits, S0, 1e4), "shifted_logits_m80-s1": (_shifted_logits, S1, -80.0),
    "shifted_logits_p80-s2": (_shifted_logits, S2, 80.0), "shifted_logits_p1e4-s2": (_shifted_logits, S2, 1e4),
    "shifted_support_low-s0": (_shifted_support, S0, False), "shifted_support_high-s0": (_shifted_support, S0, True),
    "shifted_support_low-s2": (_shifted_support, S2, False), "shifted_support_high-s2": (_shifted_support, S2, True),
    "flat_states_zero-s0": (_flat_states, S0, "flat", ("ad", "cn")), "flat_states_zero-s1": (_flat_states, S1, "flat", ("ad",)),
    "flat_states_zero-s2": (_flat_states, S2, "flat", ("cn",)),
    "flat_states_range10-s0": (_flat_states, S0, "range", ("ad", "cn"), 10),
    "flat_states_range20-s0": (_flat_states, S0, "range", ("ad", "cn"), 20),
    "flat_states_range23-s0": (_flat_states, S0, "range", ("ad", "cn"), 23),
    "flat_states_range20-s1": (_flat_states, S1, "range", ("ad", "cn"), 20),
    "flat_states_range10-s2": (_flat_states, S2, "range", ("ad", "cn"), 10),
    "flat_states_range23-s2": (_flat_states, S2, "range", ("ad", "cn"), 23),
    "flat_states_outlier-s0": (_flat_states, S0, "outlier", ("ad", "cn")),
    "flat_states_outlier-s1": (_flat_states, S1, "outlier", ("cn",)),
    "flat_states_outlier-s2": (_flat_states, S2, "outlier", ("ad",)),
    "zero_rewards_discount1-s0": (_zero_rewards, S0, 1.0), "zero_rewards_discount0-s0": (_zero_rewards, S0, 0.0),
    "zero_rewards_discount1-s2": (_zero_rewards, S2, 1.0),
    # root 0 all invalid, root 1 one valid action, root 2 only the highest indices; on all_ties the mask alone decides
    "masks_all_ties-s0": (_all_ties, S0, False, None, True), "masks_all_ties_noise-s0": (_all_ties, S0, True, None, True),
    "masks_all_ties-s2": (_all_ties, S2, False, None, True), "masks_generic-s1": (_masks_generic, S1, False),
    "masks_generic_noise-s2": (_masks_generic, S2, True),
    "temperature_0-s0": (_temperature, S0, 0.0, True), "temperature_0-s1": (_temperature, S1, 0.0, True),
    "temperature_0_tied_visits-s1": (_all_ties, S1, False, None, False, 0.0),
    "temperature_0_generic-s2": (_temperature, S2, 0.0), "temperature_1e-3-s0": (_temperature, S0, 1e-3),
    "temperature_50-s0": (_temperature, S0, 50.0), "temperature_1e-3-s2": (_temperature, S2, 1e-3),
    "fraction_0_no_noise-s0": (_noise, S0, 0.0, False), "fraction_0_with_noise-s0": (_noise, S0, 0.0, True),
    "fraction_1-s0": (_noise, S0, 1.0, True), "fraction_1-s2": (_noise, S2, 1.0, True, False, True),
    "gumbel_injected-s0": (_noise, S0, 0.25, True, True), "gumbel_injected-s1": (_noise, S1, 0.25, True, True, True),
    # the cut lands on a chance node (1) and on a decision node (2) while every comparison ties
    "max_depth_1-s0": (_all_ties, S0, False, 1), "max_depth_2-s0": (_all_ties, S0, False, 2),
    # (a cut of 2 re-expands only where a chance node has fewer outcomes than visits: the smallest shape)
    "max_depth_2_noise-s0": (_all_ties, S0, True, 2), "max_depth_1-s2": (_all_ties, S2, False, 1),
}
NAMES = tuple(_BUILDERS)


def names(*families):
    """The case names that start with one of `families`."""
    return [n for n in NAMES if n.startswith(tuple(families))]


@functools.lru_cache(maxsize=None)
def case(name):
    fn, *args = _BUILDERS[name]
    return fn(name, *args)


# ---------------------------------------------------------------- the instrumented stepper
def _bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


class EdgeStepper(st.StochasticStepper):
    """StochasticStepper with the case's Dirichlet fraction at the root and its temperature / Gumbel row at the finish
    (the parent class fixes 0.25 and 1.0), and counters over its selections.  No arithmetic of its own: the root is the
    parent's own three calls with another fraction, every score is super()._scores()."""

    def __init__(self, oracle, c):
        A, C, E, support, B, S = c.shape
        o = c.options
        super().__init__(oracle, B, A, C, E, S, *c.root, tiebreak=o.tiebreak, max_depth=o.max_depth, key=KEY, invalid=c.invalid,
                         noise=c.noise)
        self.case = c
        if c.noise is not None and o.fraction != 0.25:
            prior = oracle.root_prior(c.root[0], c.noise, o.fraction, c.invalid)
            prior = np.concatenate([prior, np.full((B, C), st.NEG_INF, F32)], axis=1)
            inv = np.ones((B, A + C), np.uint8)
            inv[:, :A] = 0 if c.invalid is None else c.invalid
            oracle.tree_init(self.tree, prior, c.root[1], st.pad_rows(np.asarray(c.root[2], F32), E), inv)
        # [kind]: 0 decision nodes, 1 chance nodes
        self.ties, self.decided, self.all_masked = [0, 0], [[], []], 0

    def _scores(self, b, node, depth, sel_key):
        score = super()._scores(b, node, depth, sel_key)
        top = np.sort(score)[::-1]
        if not np.isfinite(top[0]):
            self.all_masked += 1
        elif len(top) > 1 and np.isfinite(top[1]):
            if _bits(top[0]) == _bits(top[1]):
                self.ties[depth % 2] += 1
            else:
                self.decided[depth % 2].append((int(np.argmax(score)), float(top[0]) - float(top[1])))
        return score

    def finish(self):
        c = self.case
        g = c.gumbel if c.gumbel is not None else self.o.gumbel(self.k_sample, self.B * self.A).reshape(self.B, self.A)
        action, weights = self.o.summary_sample(self.decision_tree(), c.options.temperature, g)
        return action, weights, self.tree.node_values[:, 0].copy()


def run_reference(c):
    """The case through EdgeStepper.  dict(case, action, weights, value, depth_sum, tree; per simulation slots, kinds,
    pembs and rows (StochasticMlpReference.row's outputs); ties [2], decided [2] (winner, margin), all_masked)."""
    oracle = _oracle()
    A, C, E, support, B, S = c.shape
    ref = smr.StochasticMlpReference(oracle, c.weights, A, C, E, support, c.options.discount)
    stp = EdgeStepper(oracle, c)
    slots, kinds, pembs, rows = [], [], [], []
    for sim in range(S):
        parent, slot, kind = stp.select(sim)
        pemb = stp.parent_embedding(parent).copy()
        row = ref.row(slot, pemb)
        slots.append(slot.copy()), kinds.append(kind.copy()), pembs.append(pemb), rows.append(row)
        stp.expand_backup(sim, parent, slot, row)
    action, weights, value = stp.finish()
    return dict(case=c, action=action, weights=weights, value=value, depth_sum=stp.depth_sum.copy(), tree=stp.tree, slots=slots,
                kinds=kinds, pembs=pembs, rows=rows, ties=stp.ties, decided=stp.decided, all_masked=stp.all_masked)


@functools.lru_cache(maxsize=None)
def reference(name):
    """run_reference(case(name)), once per case and shared: treat it as read-only."""
    return run_reference(case(name))


def kind_rows(r, field):
    """The rows of one recurrent output that the search USED: (chance_logits | afterstate_value | afterstate_embedding)
    of the simulations with a decision parent, (action_logits | value | reward | state_embedding) of the others."""
    out = []
    for kinds, ((cl, av), ae, (al, v, rw, d), se) in zip(r["kinds"], r["rows"]):
        x, of_kind = dict(chance_logits=(cl, 1), afterstate_value=(av, 1), afterstate_embedding=(ae, 1), action_logits=(al, 0),
                          value=(v, 0), reward=(rw, 0), state_embedding=(se, 0))[field]
        out.extend(np.asarray(x)[kinds == of_kind])
    return out


# ---------------------------------------------------------------- root inference at its edges
OBS_DIM = 7  # one block of four and a tail


class RootCase(NamedTuple):
    name: str
    search: EdgeCase   # root = the oracle's RootFnOutput on `obs`
    repr_w: np.ndarray
    repr_b: np.ndarray
    obs: np.ndarray
    facts: dict


def root_reference(w, repr_w, repr_b, A, E, support, obs):
    """oracle.root_inference on an oracle.Mlp of the representation and the prediction heads, zero dynamics (the
    composition of tests/test_gpu_stochastic_root.py)."""
    oracle = _oracle()
    F = 2 * support + 1
    z = lambda *s: np.zeros(s, F32)  # noqa: E731
    ws = {"repr_w": repr_w, "repr_b": repr_b}
    ws.update({f"{h}_{a}": w[f"{h}_{a}"] for h in ("pv", "pp") for a in ("w1", "b1", "w2", "b2")})
    for pre, out in (("dr", F), ("dn", E)):
        ws.update({f"{pre}_w1": z(E + A, H), f"{pre}_b1": z(H), f"{pre}_w2": z(H, out), f"{pre}_b2": z(out)})
    return oracle.root_inference(oracle.Mlp(ws, repr_w.shape[0], E, A, F, support_size=support), obs)


def _root_case(name, shape, kind, shift, support_bin):
    """kind 'flat': the representation gives E equal elements (the embedding is all zeros); 'range20': max - min ==
    2**-20; 'one_hot': one element 1 and the rest 0 after the normalisation.  The policy head's biases shifted by
    `shift`, all mass of the value head on bin `support_bin` (None: left alone)."""
    A, C, E, support, B, S = shape
    rng = np.random.default_rng([13, A, C, E, B, S])
    w = _weights(shape)
    w["pp_b2"] = (w["pp_b2"] + F32(shift)).astype(F32)
    if support_bin is not None:
        w["pv_b2"][support_bin] += BIG
    repr_w = (np.clip(rng.standard_normal((OBS_DIM, E)), -2, 2) / np.sqrt(OBS_DIM)).astype(F32)
    obs = rng.uniform(-1, 1, (B, OBS_DIM)).astype(F32)
    if kind == "flat":       # the observations reach the sum, the weights are zero
        repr_w, repr_b = np.zeros_like(repr_w), np.full(E, 0.375, F32)
    elif kind == "range20":
        repr_w, repr_b = np.zeros_like(repr_w), range_row(rng, E, 20)
    else:                    # the weights reach the sum, the observations are zero
        obs, repr_b = np.zeros_like(obs), np.zeros(E, F32)
        repr_b[E // 2] = 0.75
    root = root_reference(w, repr_w, repr_b, A, E, support, obs)
    noise = rng.dirichlet([0.3] * A, B).astype(F32)
    search = EdgeCase(name, shape, w, root, None, noise, None, Options(), dict(family="root"))
    return RootCase(name, search, repr_w, repr_b, obs, dict(kind=kind, shift=float(shift), support_bin=support_bin))


_ROOT_BUILDERS = {
    "root_flat_p80-s2": (S2, "flat", 80.0, 0), "root_range20_m80-s1": (S1, "range20", -80.0, 2 * S1[3]),
    "root_one_hot_p1e4-s0": (S0, "one_hot", 1e4, None), "root_flat_m80-s0": (S0, "flat", -80.0, 2 * S0[3]),
    "root_range20_p1e4-s2": (S2, "range20", 1e4, 0),
}
ROOT_NAMES = tuple(_ROOT_BUILDERS)


@functools.lru_cache(maxsize=None)
def root_case(name):
    return _root_case(name, *_ROOT_BUILDERS[name])


@functools.lru_cache(maxsize=None)
def root_search_reference(name):
    return run_reference(root_case(name).search)
