"""The edge cases of tests/stochastic_edge_cases.py on the CPU: for every case name, proof that the REFERENCE alone
reaches the edge the case is named for (else tests/test_gpu_stochastic_edges.py could pass without the branch being
run), and that the reference is deterministic -- two runs give the same bits -- before it judges a kernel.  The
conditions are exact; each test prints the counters it asserts (pytest -s shows them)."""
import numpy as np
import pytest

import stochastic_edge_cases as ec

F32 = np.float32
NEG_ZERO = 0x80000000


def _bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def _word(x):
    return int(_bits(x).ravel()[0])


def _show(name, **counters):
    print(f"\n{name}: " + ", ".join(f"{k} = {v}" for k, v in counters.items()), end="")


@pytest.fixture(scope="module")
def oracle():
    return ec._oracle()


@pytest.mark.parametrize("name", ec.NAMES + ec.ROOT_NAMES)
def test_reference_is_deterministic(name):
    """A second, uncached run of the case: the same bits in every output and every tree array."""
    first = ec.reference(name) if name in ec.NAMES else ec.root_search_reference(name)
    again = ec.run_reference(first["case"])
    assert np.array_equal(first["action"], again["action"]) and np.array_equal(first["depth_sum"], again["depth_sum"])
    assert np.array_equal(_bits(first["weights"]), _bits(again["weights"]))
    assert np.array_equal(_bits(first["value"]), _bits(again["value"]))
    for f, a in first["tree"].arrays().items():
        b = again["tree"].arrays()[f]
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f
    for f in ("slots", "kinds"):
        assert all(np.array_equal(a, b) for a, b in zip(first[f], again[f])), f
    assert first["ties"] == again["ties"] and first["all_masked"] == again["all_masked"]


@pytest.mark.parametrize("name", ec.names("all_ties", "max_depth", "temperature_0_tied_visits"))
def test_all_ties_reaches_ties_at_both_kinds_of_node(name):
    r = ec.reference(name)
    c = r["case"]
    _show(name, decision_ties=r["ties"][0], chance_ties=r["ties"][1])
    assert r["ties"][0] > 0
    depth_cut = c.options.max_depth
    if depth_cut != 1:  # (a cut of 1 never selects at a chance node)
        assert r["ties"][1] > 0
    # every value and reward the search used is one number per head
    for field in ("afterstate_value", "value", "reward"):
        rows = ec.kind_rows(r, field)
        assert len(rows) > 0 or depth_cut == 1, field
        assert len({_word(x) for x in rows}) <= 1, field
    if not c.options.tiebreak:
        # the lowest index wins: simulation 0 takes action 0 in every root, and its first visit of a chance node outcome 0
        A = c.shape[0]
        assert (r["slots"][0] == 0).all()
        first_chance = [s[k == 0] for s, k in zip(r["slots"], r["kinds"])]
        assert all((s == A).all() for s in first_chance[:2])
    if depth_cut:
        # the cut re-expands: fewer nodes than simulations, of the kind the cut lands on
        t, S = r["tree"], c.shape[5]
        assert ((t.node_visits[:, 1:] > 0).sum(1) < S).any()
        kinds = np.concatenate(r["kinds"])
        assert (kinds == 1).all() if depth_cut == 1 else ((kinds == 0).any() and (kinds == 1).any())
        _show(name, nodes=(t.node_visits[:, 1:] > 0).sum(1).tolist())


def test_tied_final_argmax_takes_the_lowest_index():
    """Equal visit counts and a constant Gumbel row at temperature 1 and 0: action 0, with more than one action at the top."""
    for name in ("all_ties-s1", "all_ties-s2", "temperature_0_tied_visits-s1"):
        r = ec.reference(name)
        top = (r["weights"] == r["weights"].max(1, keepdims=True)).sum(1)
        _show(name, actions_sharing_the_top_visit_count=top.tolist())
        assert (top[::2] > 1).all() and (r["action"][::2] == 0).all()


@pytest.mark.parametrize("name", ec.names("chance_ties_only", "noisy_decisions_chance_ties"))
def test_chance_ties_only(name):
    r = ec.reference(name)
    _show(name, decision_ties=r["ties"][0], chance_ties=r["ties"][1], decided_decisions=len(r["decided"][0]))
    assert r["ties"][1] > 0
    if name.startswith("chance_ties_only"):
        assert r["ties"][0] > 0                            # the last root's first selection, and nothing else:
        assert len(r["decided"][0]) > 10 * r["ties"][0]    # the PUCT rule is otherwise decided by its margins
    # a chance node's first visit (zero visit total) is a tie of the best pair, and the lower outcome takes it
    A = r["case"].shape[0]
    first = r["slots"][1][r["kinds"][1] == 0] if len(r["slots"]) > 1 else []
    assert all((s - A) % 2 == 0 for s in first)


@pytest.mark.parametrize("name", ec.names("small_margins"))
def test_small_margins_follow_the_ulp(name):
    r = ec.reference(name)
    f = r["case"].facts
    won = [sum(1 for w, m in r["decided"][k] if w == idx and m > 0) for k, idx in ((0, f["raised_action"]), (1, f["raised_slot"]))]
    _show(name, decision_ties=r["ties"][0], decisions_won_by_the_raised_action=won[0], chance_won_by_the_raised_outcome=won[1])
    assert r["ties"][0] > 0
    assert won[0] > 0 and won[1] > 0
    # simulation 0 is decided by the ulp alone
    assert (r["slots"][0] == f["raised_action"]).all()


@pytest.mark.parametrize("name", ec.names("shifted_logits"))
def test_shifted_logits_are_beyond_a_naive_softmax(name, oracle):
    """The largest |logit| of a row above 80 (rows of the three kinds counted), and exp(x) / sum(exp(x)) without the maximum taken off
    gives other bits than the specified softmax, or no number at all, on rows of every kind."""
    r = ec.reference(name)
    kinds = dict(root=list(r["case"].root[0]), action_logits=ec.kind_rows(r, "action_logits"),
                 chance_logits=ec.kind_rows(r, "chance_logits"))
    beyond, differs = {}, {}
    for kind, rows in kinds.items():
        assert len(rows) > 0
        beyond[kind] = sum(1 for x in rows if float(np.abs(x).max()) > 80)
        n = 0
        for x in rows:
            with np.errstate(all="ignore"):
                e = oracle.exp(x)
                naive = (e / F32(oracle.sum16(e))).astype(F32)
            n += not np.array_equal(_bits(naive), _bits(oracle.softmax(x)))
        differs[kind] = n
    _show(name, rows_with_max_beyond_80=beyond, rows_a_naive_softmax_gets_wrong=differs)
    assert sum(beyond.values()) > 0
    assert all(n > 0 for n in differs.values())


@pytest.mark.parametrize("name", ec.names("shifted_support"))
def test_shifted_support_decodes_to_the_last_bin(name, oracle):
    r = ec.reference(name)
    c = r["case"]
    edge = c.facts["decode"]
    assert abs(float(edge)) == float(oracle.inv_scaling(F32(c.shape[3])))
    counts = {}
    for field in ("afterstate_value", "value", "reward"):
        rows = ec.kind_rows(r, field)
        counts[field] = len(rows)
        assert len(rows) > 0 and all(_word(x) == _word(edge) for x in rows), field
    _show(name, decode=float(edge), decodes_on_the_last_bin=counts)


@pytest.mark.parametrize("name", ec.names("flat_states"))
def test_flat_states_reach_their_range(name, oracle):
    """The heads' output layers are zero, so the state before the normalisation IS the bias row: its range is the case's
    (0, 2**-k, or set by the outlier), and every state the search expanded from such a head is the oracle's
    normalisation of that row."""
    r = ec.reference(name)
    f = r["case"].facts
    seen = {}
    for head, field in (("ad", "afterstate_embedding"), ("cn", "state_embedding")):
        if head not in f["rows"]:
            continue
        row = f["rows"][head]
        assert not r["case"].weights[f"{head}_w2"].any() and np.array_equal(r["case"].weights[f"{head}_b2"], row)
        span = F32(row.max() - row.min())
        if f["kind"] == "flat":
            assert span == 0
        elif f["kind"] == "range":
            assert span == F32(2.0 ** -f["k"])
        else:
            assert span > 1e5
        want = oracle.min_max_normalize(row)
        states = ec.kind_rows(r, field)
        assert len(states) > 0 and all(np.array_equal(_bits(s), _bits(want)) for s in states)
        if f["kind"] == "flat":
            assert not _bits(want).any()  # range exactly 0: (s - min) / (0 + 1e-5) is +0.0 everywhere
        elif f["kind"] == "range":
            assert want.min() == 0 and (want.max() == 1) == (f["k"] == 10)  # below 1e-5 the range gets 1e-5 added
        seen[head] = (len(states), float(span))
    _show(name, expanded_states_and_range_by_head=seen)
    assert seen


@pytest.mark.parametrize("name", ec.names("zero_rewards"))
def test_zero_rewards_are_zeros_of_the_specified_sign(name, oracle):
    """Every stored reward is a zero.  The issue of this file asked for the pattern 0x00000000 throughout; the reference
    cannot give it for a reward that a head decoded: inv_scaling(0) is sign(0) * (e * e - 1) with e * e - 1 < 0 in fp32,
    which is -0.0 (asserted first), and no other input of inv_scaling gives a zero at all.  So the conditions are: edges
    into chance nodes hold +0.0, edges out of them the decoded -0.0, and both occur."""
    assert _word(oracle.inv_scaling(F32(0.0))) == NEG_ZERO
    r = ec.reference(name)
    t, A = r["tree"], r["case"].shape[0]
    bits = _bits(t.children_rewards)
    assert not (bits & 0x7FFFFFFF).any()
    decoded = ec.kind_rows(r, "reward")
    assert len(decoded) > 0 and all(_word(x) == NEG_ZERO for x in decoded)
    depth = ec.ss.node_depths(t.parents)
    expanded = t.children_index >= 0
    from_chance = expanded & (depth % 2 == 1)[:, :, None]
    from_chance[:, 0] = False
    assert from_chance.any() and (bits[from_chance] == NEG_ZERO).all()
    assert not bits[~from_chance].any() and not bits[..., :A].any()
    _show(name, stored_minus_zero=int((bits == NEG_ZERO).sum()), stored_plus_zero_on_expanded_edges=int((expanded & ~from_chance).sum()),
          discount=r["case"].options.discount)


@pytest.mark.parametrize("name", ec.names("masks"))
def test_masks_reach_every_kind_of_root(name):
    """Root 0: every action invalid.  mctx's stochastic_muzero_policy does not define that root (its masked argmax runs
    over -inf only); what the stepper does is the specification here and is recorded: action 0 at every visit of the
    root, finite weights.  Root 1: one valid action takes all S visits.  Root 2: only the highest indices are visited."""
    r = ec.reference(name)
    c = r["case"]
    A, S = c.shape[0], c.shape[5]
    inv, t = c.invalid, r["tree"]
    assert inv[0].all() and inv[1].sum() == A - 1 and not inv[2, -1] and inv[2, 0]
    root_visits = t.children_visits[:, 0, :A]
    assert r["all_masked"] == S  # one selection at root 0 per simulation, each over -inf only
    assert np.isfinite(r["weights"][0]).all() and root_visits[0, 0] == S and r["action"][0] >= 0
    assert root_visits[1, 1 % A] == S and root_visits[1].sum() == S and r["weights"][1, 1 % A] == 1
    assert root_visits[2][inv[2] != 0].sum() == 0 and root_visits[2].sum() == S
    assert (root_visits[1:][inv[1:] != 0] == 0).all()
    _show(name, all_masked_selections=r["all_masked"], all_invalid_root_weights=r["weights"][0].tolist(),
          all_invalid_root_action=int(r["action"][0]), decision_ties=r["ties"][0])
    if c.facts["family"] == "all_ties":
        assert r["ties"][0] > 0


@pytest.mark.parametrize("name", ec.names("temperature_0-"))
def test_temperature_zero_one_hot(name):
    r = ec.reference(name)
    w = r["weights"]
    _show(name, weights_row_0=w[0].tolist())
    assert r["case"].options.temperature == 0.0
    assert ((w == 0) | (w == 1)).all() and (w.sum(1) == 1).all()
    assert np.array_equal(r["action"], w.argmax(1))


def test_temperature_and_noise_options_change_what_they_should():
    """The options reach the reference: the temperature moves the sampled action but not the weights; fraction 0 with a
    noise array is fraction 0 without one; fraction 1 is another search; an injected Gumbel row is used."""
    lo, hi = ec.reference("temperature_1e-3-s0"), ec.reference("temperature_50-s0")
    assert np.array_equal(_bits(lo["weights"]), _bits(hi["weights"])) and not np.array_equal(lo["action"], hi["action"])
    assert np.array_equal(lo["action"], lo["weights"].argmax(1))  # (1e-3: the visits decide, whatever the Gumbel row)
    a, b, one = (ec.reference(n) for n in ("fraction_0_no_noise-s0", "fraction_0_with_noise-s0", "fraction_1-s0"))
    assert np.array_equal(_bits(a["weights"]), _bits(b["weights"]))
    assert np.array_equal(_bits(a["tree"].children_prior_logits), _bits(b["tree"].children_prior_logits))
    assert not np.array_equal(_bits(a["tree"].children_prior_logits[:, 0]), _bits(one["tree"].children_prior_logits[:, 0]))
    c = one["case"]
    assert c.noise[0, 0] == 0 and c.options.fraction == 1.0
    g = ec.reference("gumbel_injected-s0")
    assert g["case"].gumbel is not None and g["case"].noise is not None


@pytest.mark.parametrize("name", ec.ROOT_NAMES)
def test_root_cases_reach_their_edges(name, oracle):
    rc = ec.root_case(name)
    A, C, E, support, B, S = rc.search.shape
    logits, value, emb = rc.search.root
    kind = rc.facts["kind"]
    if kind == "flat":
        assert not _bits(emb).any()
    elif kind == "range20":
        pre = rc.repr_b
        assert not rc.repr_w.any() and F32(pre.max() - pre.min()) == F32(2.0 ** -20)
        assert all(np.array_equal(_bits(e), _bits(oracle.min_max_normalize(pre))) for e in emb)
    else:
        assert ((emb == 0).sum(1) == E - 1).all() and (emb.max(1) == 1).all()
    assert (np.abs(logits).max(1) > 80).all()
    if rc.facts["support_bin"] is not None:
        sign = 1.0 if rc.facts["support_bin"] else -1.0
        assert (value == F32(sign * oracle.inv_scaling(F32(support)))).all()
    _show(name, largest_logit=float(np.abs(logits).max()), value=float(value[0]), embedding_max=float(emb.max()))


def test_more_roots_than_one_round_is_one_root_more():
    from muax_amd import search
    B = ec.more_roots_batch()
    A, C, E, support = ec.SHAPES[0][:4]
    pl = search.stochastic_plan(A, C, E, support, 3)
    _show("more_roots_than_one_round", B=B, waves=pl["waves"], roots_per_cu=pl["roots_per_cu"])
    assert (B - 1) % pl["waves"] == 0 and (B - 1) // pl["roots_per_cu"] == ec.MI355X_CUS
    c = ec.more_roots_case(B, False)
    last = ec.run_reference(ec.rows_of(c, [B - 1]))
    trio = ec.run_reference(ec.rows_of(c, [0, 1, B - 1]))
    assert np.array_equal(_bits(last["weights"][0]), _bits(trio["weights"][2])) and last["action"][0] == trio["action"][2]
