"""The generic one-launch MLP search (mz_mlp_generic.cuh behind allow_generic(): net shapes, action slots and LDS layout
all run-time values) against the CPU oracle over its run-time parameters: every output and every tree array with ==.

Forcing the route: allow_wide() is never called here and every case asserts `_jit.plan(A, E, F, S) is None` (no fused
instance can exist: more than 16 actions, an embedding wider than 64 or more than 255 simulations), the first act on
the handle must raise "no fused kernel instance", and only then is allow_generic() called.

Which of the eight builds of mz_mlp_search_kernel a case runs is restated from launch_mlp_search (mz_stepwise.hip) in
`_build_of` and asserted per test:

    lds_search = 4 * 15 * (S + 2) + 4 * gen_scratch_words(E, A)          (act_mlp_generic)
    lds_tbl    = lds_search + 4 * 2 * (S + 2);   tbl = S + 2 <= 1030 and lds_tbl <= 64 KiB
    Gumbel policy -> "gumbel";  tbl and A <= 16 -> "as1";  tbl and A <= 32 -> "as2";  else "general"
    occ4 (the 128-register build) = roots of the launch > 2048 and 16 * lds <= 160 KiB, lds = lds_tbl where the table is
    used, else lds_search

Every branch a case exists for (re-expansions, paths deeper than 64 levels, a normaliser range below 1e-5, all-zero
statistics, the chunked launch) is asserted on the ORACLE's result, before the handle is created.
"""
import numpy as np
import pytest
import torch

from helpers import make_case
from test_gpu_parity import _compare, _fused_any, _gumbel_oracle_act, _oracle
from test_gpu_wide import _act as _wide_act, _depths, _handle as _wide_handle
from test_gpu_wide_gumbel import QTS, _oracle as _gumbel_oracle

pytestmark = pytest.mark.gpu

F32 = np.float32
KIB = 1024


def _r4(n):
    return (n + 3) // 4 * 4


def _scratch_words(E, A):
    """gen_scratch_words (mz_mlp_blocks.cuh): sa [E + A] | hid [32] | rl, vl, pl [64 each] | ns [E] | scal [4]."""
    return _r4(E + A) + 32 + 3 * 64 + _r4(E) + 4


def _lds_root(E, A, obs_dim):
    return 4 * _scratch_words(max(E, obs_dim), A)


def _lds_search(E, A, S):
    return 4 * 15 * (S + 2) + 4 * _scratch_words(E, A)


def _has_table(E, A, S):
    return S + 2 <= 1030 and _lds_search(E, A, S) + 8 * (S + 2) <= 64 * KIB


def _build_of(case, policy="muzero", roots=None):
    """(variant, occ4) of the search launch, restated from launch_mlp_search; `roots`: those of one launch."""
    A, E, S = case["A"], case["E"], case["S"]
    n = case["B"] if roots is None else roots
    tbl = _has_table(E, A, S)
    variant = "gumbel" if policy == "gumbel" else "as1" if tbl and A <= 16 else "as2" if tbl and A <= 32 else "general"
    lds = _lds_search(E, A, S) + (8 * (S + 2) if variant in ("as1", "as2") else 0)
    return variant, n > 2 * 4 * 256 and 16 * lds <= 160 * KIB


def _generic(case, key, policy="muzero", tiebreak=True, pred_on="child", use_noise=True, use_gumbel=True,
             temperature=1.0, **cfg_kw):
    """One act on a raw handle through the generic route and nothing else (see the module docstring)."""
    from muax_amd import MuZeroSearch, SearchConfig, _jit
    assert _jit.plan(case["A"], case["E"], case["F"], case["S"]) is None
    s = MuZeroSearch(case["B"], SearchConfig(case["A"], case["S"], case["E"], tiebreak=tiebreak, policy=policy, **cfg_kw))
    s.set_mlp_weights({k: torch.from_numpy(v) for k, v in case["w"].items()}, case["obs_dim"], case["support"], 0.99, pred_on)
    args = dict(invalid_actions=None if case["invalid"] is None else torch.from_numpy(case["invalid"]), with_tree=True,
                temperature=temperature, gumbel=torch.from_numpy(case["gumbel"]) if use_gumbel else None)
    if policy == "muzero" and use_noise:
        args["dirichlet_noise"] = torch.from_numpy(case["noise"])
    with pytest.raises(ValueError, match="no fused kernel instance"):
        s.act_mlp(torch.from_numpy(case["obs"]), key, **args)
    s.allow_generic()
    out = s.act_mlp(torch.from_numpy(case["obs"]), key, **args)
    torch.cuda.synchronize()
    return s, out


def _check(ref, s, out):
    _compare(ref, s, out)
    s.close()


def _reexpands(tree):
    """A simulation cut at max_depth expands an existing node again: its own node stays unused (parent -1), and some
    node is visited more than once."""
    return bool((tree.parents[:, 1:] < 0).any() and (tree.node_visits[:, 1:].max(axis=1) > 1).any())


# ---------------------------------------------------------------- 1. support heads

@pytest.mark.parametrize("policy", ["muzero", "gumbel"])
@pytest.mark.parametrize("support,S,B", [(8, 30, 21), (16, 30, 21), (24, 30, 21), (31, 30, 21), (8, 20, 2100), (31, 20, 2100)])
def test_generic_support_heads(oracle, support, S, B, policy):
    """F = 2 support + 1 in {17, 33, 49, 63}: one real lane in gen_decode's second slot, one past the second and the
    third slot's edge, one pad lane in the fourth -- both policies; F = 17 and 63 also on the 128-register build."""
    case = make_case(oracle, 2000 + support + S, B, 6, 8, 18, S, support=support, invalid_frac=0.2)
    assert case["F"] in (17, 33, 49, 63)
    assert _build_of(case, policy) == ("gumbel" if policy == "gumbel" else "as2", B > 2048)
    key = [support, S]
    if policy == "muzero":
        ref = _oracle(oracle, case, True, key)
        _check(ref, *_fused_any(case, True, key, "generic"))
    else:
        ref = _gumbel_oracle(oracle, case, key, 1, 16)
        _check(ref, *_fused_any(case, False, key, "generic", policy="gumbel", qtransform=QTS[1]))


# ---------------------------------------------------------------- 2. observation widths

@pytest.mark.parametrize("obs_dim,E,A", [(1, 8, 18), (9, 8, 18), (70, 8, 18), (128, 8, 18), (70, 70, 5)])
def test_generic_observation_widths(oracle, obs_dim, E, A):
    """mz_mlp_root_kernel's scratch is laid out with gen_obs_width(E, obs_dim): obs_dim above E (9, 70, 128: G.sa holds
    the observation only because of it), above 64 (gen_embed's copy loop strides twice), below E (1) and equal to it."""
    case = make_case(oracle, 2100 + obs_dim + E, 9, obs_dim, E, A, 20, invalid_frac=0.2)
    assert _lds_root(E, A, obs_dim) == 4 * _scratch_words(max(E, obs_dim), A)
    assert (_lds_root(E, A, obs_dim) > _lds_root(E, A, 1)) == (obs_dim > E)  # gen_obs_width decides the launch's LDS
    assert _build_of(case) == ("as1" if A <= 16 else "as2", False)
    key = [obs_dim, E]
    _check(_oracle(oracle, case, True, key), *_fused_any(case, True, key, "generic"))


# ---------------------------------------------------------------- 3. embedding widths

def _fits(E, A, S, obs_dim):
    """act_mlp_generic's LDS check: lds_root = 4 gen_scratch_words(max(E, obs_dim), A) and lds_search = 4 * 15 (S + 2) +
    4 gen_scratch_words(E, A), both at most 64 KiB."""
    return _lds_root(E, A, obs_dim) <= 64 * KIB and _lds_search(E, A, S) <= 64 * KIB


def _largest_embedding(A, S, obs_dim):
    E = 1
    while _fits(E + 1, A, S, obs_dim):
        E += 1
    return E


@pytest.mark.parametrize("A,E,B", [(4, 65, 9), (4, 67, 9), (4, 100, 9), (5, 66, 9), (18, 1, 9), (4, 255, 9), (4, 65, 2100)])
def test_generic_embedding_widths(oracle, A, E, B):
    """gen_linear's 8-link unroll and tail (E = 65 and 67: tails of 1 and 3, E + A = 71: a tail of 7), gen_lds rounding
    E + A and E up to 4 words, E = 1 (the normaliser over one element: range 0, the `scale + 1e-5f` branch, with 18
    actions), and the widest embedding below the wide-row threshold.  The LDS check itself accepts embeddings far wider
    (7908 at S = 20, A = 4; computed below) -- at or above kWideEmb = 256 the tree kernels move embedding rows another
    way, so the widest case here is E = 255.  (4, 65) at 2100 roots: the one-slot table kernel's 128-register build."""
    S, obs_dim = 20, 6
    if E == 255:
        assert _largest_embedding(A, S, obs_dim) >= 256  # kWideEmb (mz_step.cuh)
        assert _fits(E, A, S, obs_dim)
    if E == 66:
        assert (E + A) % 8 == 7
    case = make_case(oracle, 2200 + A + E, B, obs_dim, E, A, S, invalid_frac=0.2 if A > 2 else 0.0)
    assert _build_of(case) == ("as1" if A <= 16 else "as2", B > 2048)
    key = [A, E]
    _check(_oracle(oracle, case, True, key), *_fused_any(case, True, key, "generic"))


def test_generic_refuses_an_embedding_beyond_the_lds(oracle):
    """The widest embedding the route's LDS check accepts at S = 20, A = 4 (from lds_search: 4 * 15 * 22 + 4 (r4(E + 4) +
    228 + r4(E)) <= 65536, i.e. r4(E + 4) + r4(E) <= 15826: E = 7908), and 64 more: refused with the route's own message
    (the check stands in front of the first launch of act_mlp_generic)."""
    from muax_amd import MuZeroSearch, SearchConfig, _jit
    A, S, obs_dim = 4, 20, 6
    E = _largest_embedding(A, S, obs_dim)
    assert E == 7908 and _fits(E, A, S, obs_dim) and not _fits(E + 1, A, S, obs_dim) and not _fits(E + 64, A, S, obs_dim)
    case = make_case(oracle, 2299, 2, obs_dim, E + 64, A, S)
    assert _jit.plan(A, E + 64, case["F"], S) is None
    s = MuZeroSearch(2, SearchConfig(A, S, E + 64))
    s.set_mlp_weights({k: torch.from_numpy(v) for k, v in case["w"].items()}, obs_dim, 10, 0.99)
    s.allow_generic()
    with pytest.raises(ValueError, match="generic route.*too large for the LDS of a workgroup"):
        s.act_mlp(torch.from_numpy(case["obs"]), [1, 2], dirichlet_noise=torch.from_numpy(case["noise"]))
    torch.cuda.synchronize()
    s.close()


# ---------------------------------------------------------------- 4. the pUCT-table boundary

def _last_table_fit(E, A):
    S = 1
    while _has_table(E, A, S + 1):
        S += 1
    return S


def _dig(case, bias):
    """One action dominates the prior: the search digs lines far deeper than 64 levels."""
    b2 = np.full(case["A"], -bias, F32)
    b2[0] = bias
    case["w"]["pp_b2"] = b2
    return case


@pytest.mark.parametrize("A", [2, 18])
@pytest.mark.parametrize("which,max_depth", [("fit", None), ("nofit", None), ("limit", None), ("fit", 20), ("nofit", 20)])
def test_generic_table_boundary(oracle, A, which, max_depth):
    """The MuZero code with the pUCT table in LDS (one / two action slots) on the last S whose table fits, the general
    code (no slot count, no table) at 32 actions or fewer on the first S without it and at the route's 1023 limit.

    lds_tbl = 4 * 15 (S + 2) + 4 * 2 (S + 2) + 4 gen_scratch_words(E, A) = 68 (S + 2) + 4 words <= 65536:
      (A, E) = (2, 8):  words = 12 + 32 + 192 + 8 + 4 = 248, 68 (S + 2) <= 64544, S + 2 <= 949, last fit S = 947;
      (A, E) = (18, 8): words = 28 + 32 + 192 + 8 + 4 = 264, 68 (S + 2) <= 64480, S + 2 <= 948, last fit S = 946;
    S + 2 <= 1030 holds for every S here, and lds_search at S = 1023 is 61500 + 4 words < 65536 (the route accepts it).
    With max_depth = 20 the cut re-expands nodes inside the one-launch loop; without it the biased prior digs paths
    deeper than 64 levels (the 63-level return chunks), asserted on the oracle's parents."""
    E, B = 8, 3
    last = _last_table_fit(E, A)
    assert last == {2: 947, 18: 946}[A]
    S = {"fit": last, "nofit": last + 1, "limit": 1023}[which]
    assert _fits(E, A, S, 6) and S + 1 <= 1024  # kJumpMaxNodes
    case = _dig(make_case(oracle, 2300 + A, B, 6, E, A, S, invalid_frac=0.2 if A > 2 else 0.0), 3.0)
    want = ("as1" if A <= 16 else "as2") if which == "fit" else "general"
    assert _build_of(case) == (want, False)
    key = [A, S]
    ref = _oracle(oracle, case, True, key, max_depth=max_depth)
    depth = _depths(ref["tree"].parents)
    if max_depth:
        assert depth.max() == max_depth and _reexpands(ref["tree"])
    else:
        assert (depth.max(axis=1)[1:] > 64).all()  # (root 0 has every action masked at A = 18)
    _check(ref, *_generic(case, key, max_depth=max_depth))


# ---------------------------------------------------------------- 5. options on every build

_OPT = {False: (40, 61), True: (20, 2100)}  # occ4 -> (S, B)


def _opt_case(oracle, seed, occ4, A=18):
    S, B = _OPT[occ4]
    return make_case(oracle, seed, B, 6, 8, A, S, invalid_frac=0.2)


@pytest.mark.parametrize("occ4", [False, True])
def test_generic_muzero_options(oracle, occ4):
    """The two-slot table kernel, 181- and 128-register build: prediction on the parent's embedding (G.sa) without
    tie-break noise and with the sample's Gumbel from the key, temperatures 0.25 and 0, no Dirichlet array, a row with
    one valid action and a row with none."""
    case = _opt_case(oracle, 2400, occ4)
    S = case["S"]
    assert _build_of(case) == ("as2", occ4)
    key = [5, 6]
    ref = _oracle(oracle, case, False, key, pred_on=1, use_gumbel=False)
    child = _oracle(oracle, case, False, key, use_gumbel=False)
    assert not np.array_equal(ref["tree"].children_prior_logits, child["tree"].children_prior_logits)
    _check(ref, *_generic(case, key, tiebreak=False, pred_on="parent", use_gumbel=False))
    for temperature in (0.25, 0.0):
        _check(_oracle(oracle, case, True, key, temperature=temperature), *_generic(case, key, temperature=temperature))
    _check(_oracle(oracle, case, True, key, use_noise=False), *_generic(case, key, use_noise=False))
    assert case["invalid"][0].all()  # every action masked
    case["invalid"][3, :] = 1
    case["invalid"][3, 11] = 0
    ref = _oracle(oracle, case, True, key)
    assert int(ref["action"][3]) == 11 and int(ref["tree"].children_visits[3, 0, 11]) == S
    s, out = _generic(case, key)
    assert int(out.search_tree.children_visits[3, 0, 11]) == S
    _check(ref, s, out)


@pytest.mark.parametrize("occ4", [False, True])
@pytest.mark.parametrize("max_depth", [3, 9])
def test_generic_muzero_max_depth(oracle, occ4, max_depth):
    """Re-expansion at the depth limit overwrites a node's embedding row in HBM inside the one-launch loop that gathers
    the parent rows from the same array.  (A mildly biased prior, so that 20 simulations reach depth 9.)"""
    case = _dig(_opt_case(oracle, 2410, occ4), 1.5)
    assert _build_of(case) == ("as2", occ4)
    key = [7, max_depth]
    ref = _oracle(oracle, case, True, key, max_depth=max_depth)
    assert _reexpands(ref["tree"]) and _depths(ref["tree"].parents).max() == max_depth
    _check(ref, *_generic(case, key, max_depth=max_depth))


@pytest.mark.parametrize("occ4", [False, True])
@pytest.mark.parametrize("qt", [0, 1])
def test_generic_gumbel_options(oracle, occ4, qt):
    """The Gumbel build, 181 and 128 registers, both qtransforms: 1, 5, 16 and A = 18 considered actions, a scaled root
    noise drawn from the key, prediction on the parent, re-expansions at max_depth 3 and 9, rows with one / no valid
    action."""
    case = _opt_case(oracle, 2420 + qt, occ4)
    S = case["S"]
    case["invalid"][3, :] = 1
    case["invalid"][3, 11] = 0
    assert _build_of(case, "gumbel") == ("gumbel", occ4)
    key = [9, qt]
    kw = dict(policy="gumbel", tiebreak=False, qtransform=QTS[qt])
    for maxc in (1, 5, 16, 18):
        ref = _gumbel_oracle(oracle, case, key, qt, maxc)
        assert int(ref["action"][3]) == 11 and int(ref["tree"].children_visits[3, 0, 11]) == S
        if maxc == 1:
            assert (ref["tree"].children_visits[:, 0].max(axis=1) == S).all()
        _check(ref, *_generic(case, key, max_num_considered_actions=maxc, **kw))
    ref = _gumbel_oracle(oracle, case, key, qt, 16, use_gumbel=False, gumbel_scale=0.5)
    _check(ref, *_generic(case, key, use_gumbel=False, gumbel_scale=0.5, **kw))
    ref = _gumbel_oracle(oracle, case, key, qt, 16, pred_on=1)
    assert not np.array_equal(ref["tree"].children_prior_logits, _gumbel_oracle(oracle, case, key, qt, 16)["tree"].children_prior_logits)
    _check(ref, *_generic(case, key, pred_on="parent", **kw))
    deep = _dig(dict(case, w=dict(case["w"])), 3.0)  # (20 simulations over two considered actions reach depth 9)
    for max_depth in (3, 9):
        ref = _gumbel_oracle(oracle, deep, key, qt, 2, max_depth=max_depth)
        assert _reexpands(ref["tree"]) and _depths(ref["tree"].parents).max() == max_depth
        _check(ref, *_generic(deep, key, max_num_considered_actions=2, max_depth=max_depth, **kw))


def test_generic_gumbel_default_oracle_composition(oracle):
    """The same Gumbel case against test_gpu_parity's composition of the oracle's pieces (default net options)."""
    case = _opt_case(oracle, 2430, False, A=20)
    assert _build_of(case, "gumbel") == ("gumbel", False)
    ref = _gumbel_oracle_act(oracle, case, [2, 3], 1, 20, gumbel=case["gumbel"])
    _check(ref, *_generic(case, [2, 3], policy="gumbel", tiebreak=False, qtransform=QTS[1], max_num_considered_actions=20))


@pytest.mark.parametrize("option", ["max_depth", "pred_on_parent"])
@pytest.mark.parametrize("policy", ["muzero", "gumbel"])
def test_generic_options_in_chunks(oracle, monkeypatch, option, policy):
    """MZS_JUMP_BUDGET_MB=1: the slab holds 1 MiB / (4 (3 N + N^2)) = 67 roots of N = 61 nodes, 97 roots are searched as
    67 + 30 (ensure_step_state, act_mlp_generic_chunks) -- with re-expansions and with the prediction on the parent."""
    monkeypatch.setenv("MZS_JUMP_BUDGET_MB", "1")
    case = _dig(make_case(oracle, 2440, 97, 6, 8, 18, 60, invalid_frac=0.2), 1.5)
    N = case["S"] + 1
    roots = (1 << 20) // (4 * (3 * N + N * N))
    assert roots == 67 and roots < case["B"] and case["B"] % roots != 0
    assert _build_of(case, policy, roots=roots) == ("gumbel" if policy == "gumbel" else "as2", False)
    key = [78, 60]
    max_depth, pred = (9, 0) if option == "max_depth" else (0, 1)
    opts = dict(max_depth=max_depth or None, pred_on="parent" if pred else "child")
    if policy == "muzero":
        ref = _oracle(oracle, case, True, key, max_depth=max_depth, pred_on=pred)
        s, out = _generic(case, key, **opts)
    else:
        ref = _gumbel_oracle(oracle, case, key, 1, 4, max_depth=max_depth, pred_on=pred)
        s, out = _generic(case, key, policy="gumbel", tiebreak=False, qtransform=QTS[1], max_num_considered_actions=4, **opts)
    assert _reexpands(ref["tree"]) == (option == "max_depth")
    _check(ref, s, out)


# ---------------------------------------------------------------- 6. edge weights

@pytest.mark.parametrize("A,S", [(18, 40), (33, 30)])
def test_generic_all_ties_noise_decides(oracle, A, S):
    """All-zero weights: uniform priors, zero values and rewards at every node -- every decision at every depth is an
    exact tie among the equally visited actions and mctx's 1e-7 * uniform noise decides it; without the noise the first
    action wins, so the two trees differ.  A = 18: the two-slot table kernel, A = 33: the general code."""
    case = make_case(oracle, 77, 37, 4, 8, A, S)
    case["w"] = {k: np.zeros_like(v) for k, v in case["w"].items()}
    assert _build_of(case) == ("as2" if A <= 32 else "general", False)
    key = [11, 22]
    ref, ref0 = (_oracle(oracle, case, tb, key, use_noise=False) for tb in (True, False))
    for r in (ref, ref0):
        t = r["tree"]
        assert not t.children_prior_logits[:, 1:].any() and (t.children_prior_logits[:, 0] == t.children_prior_logits[:, :1, :1]).all()
        assert not t.node_values.any() and not t.children_values.any() and not t.children_rewards.any()
    assert not np.array_equal(ref["tree"].children_index, ref0["tree"].children_index)
    s, out = _generic(case, key, use_noise=False)
    s0, out0 = _generic(case, key, tiebreak=False, use_noise=False)
    assert not torch.equal(out.search_tree.children_index, out0.search_tree.children_index)
    _check(ref, s, out)
    _check(ref0, s0, out0)


def test_generic_small_margins(oracle):
    """Weights scaled by 1e-4: score margins around the 1e-7 noise scale, near ties and clear decisions mixed."""
    case = make_case(oracle, 78, 40, 4, 8, 20, 40)
    case["w"] = {k: (v * 1e-4).astype(F32) for k, v in case["w"].items()}
    assert _build_of(case) == ("as2", False)
    _check(_oracle(oracle, case, True, [5, 5], use_noise=False), *_generic(case, [5, 5], use_noise=False))


@pytest.mark.parametrize("shift", [-300.0, 300.0])
@pytest.mark.parametrize("A,support,B", [(17, 8, 21), (33, 16, 21), (49, 24, 21), (49, 24, 2100)])
def test_generic_policy_logits_shifted(oracle, A, support, B, shift):
    """pp_b2 shifted by -+300 where the last 16-lane slot of the policy head (and of the support heads: F = A) holds one
    real lane: every real logit sits near -+300 while a pad lane's raw value is 0.  (49 actions at 2100 roots: the
    general code's 128-register build.)"""
    S = 30 if B < 2048 else 20
    case = make_case(oracle, 2500 + A, B, 6, 8, A, S, support=support, invalid_frac=0.2)
    case["w"]["pp_b2"] = (case["w"]["pp_b2"] + F32(shift)).astype(F32)
    assert case["F"] == A and A % 16 == 1
    assert _build_of(case) == ("as2" if A <= 32 else "general", B > 2048)
    key = [A, 3]
    ref = _oracle(oracle, case, True, key)
    assert np.abs(np.abs(ref["tree"].children_prior_logits[:, 1]).mean() - 300.0) < 5.0  # (node 1: raw net logits)
    _check(ref, *_generic(case, key))


@pytest.mark.parametrize("log2_c", [-18, -16])
def test_generic_near_constant_state(oracle, log2_c):
    """dn_w2 = 0 and dn_b2 = 0.25 + c k / 8 (k = 0..7, exact in fp32; repr_w / repr_b alike for the root): the range of
    every embedding the search normalises is 7 c / 8 -- 3.3e-6 at c = 2^-18, below gen_min_max_normalize's 1e-5 (the
    `scale + 1e-5f` branch in every simulation), 1.3e-5 at c = 2^-16, above it."""
    A, E, S, B = 18, 8, 30, 21
    case = make_case(oracle, 2600, B, 6, E, A, S, invalid_frac=0.2)
    c = 2.0 ** log2_c
    b2 = (0.25 + c * np.arange(E) / 8).astype(F32)
    assert np.array_equal(b2.astype(np.float64), 0.25 + c * np.arange(E) / 8)
    w = case["w"]
    w["dn_w2"], w["repr_w"] = np.zeros_like(w["dn_w2"]), np.zeros_like(w["repr_w"])
    w["dn_b2"], w["repr_b"] = b2.copy(), b2.copy()
    assert _build_of(case) == ("as2", False)
    key = [2, 18 + log2_c]
    ref = _oracle(oracle, case, True, key)
    rng = b2.max() - b2.min()
    assert rng == F32(7 * c / 8) and (rng < F32(1e-5)) == (log2_c == -18)
    want = (b2 - b2.min()) / (rng + F32(1e-5) if rng < F32(1e-5) else rng)
    assert want.dtype == F32 and (want.max() < 1.0) == (log2_c == -18)
    emb = ref["tree"].embeddings
    live = ref["tree"].node_visits > 0
    assert live[:, 1:].sum() == B * S and (emb[live] == want).all()  # every simulation's next state, and the root's
    _check(ref, *_generic(case, key))


def test_generic_rewards_exactly_zero(oracle):
    """dr_w2 = dr_b2 = 0: a uniform reward softmax decodes to exactly 0 at every edge."""
    case = make_case(oracle, 2610, 21, 6, 8, 18, 30, invalid_frac=0.2)
    case["w"]["dr_w2"], case["w"]["dr_b2"] = np.zeros_like(case["w"]["dr_w2"]), np.zeros_like(case["w"]["dr_b2"])
    assert _build_of(case) == ("as2", False)
    ref = _oracle(oracle, case, True, [6, 1])
    assert not ref["tree"].children_rewards.any() and ref["tree"].node_values.any()
    _check(ref, *_generic(case, [6, 1]))


# ---------------------------------------------------------------- 7. route agreement

@pytest.mark.parametrize("option", ["pred_on_parent", "max_depth"])
def test_generic_same_bits_as_wide_route(oracle, option):
    """Two of the option cases on the wide-action kernel (allow_wide only) and on the generic route (allow_generic only):
    the prediction on the parent with F = 63, and max_depth = 9 -- the same bits in every output and tree array."""
    from muax_amd import _jit
    from muax_amd.search import wide_plan
    support = 31 if option == "pred_on_parent" else 10
    case = _dig(make_case(oracle, 2700, 61, 6, 8, 18, 40, support=support, invalid_frac=0.2), 1.5)
    assert wide_plan(18, 8, support, 40) is not None and _jit.plan(18, 8, case["F"], 40) is None
    kw = dict(pred_on="parent") if option == "pred_on_parent" else dict(max_depth=9)
    key = [8, 9]
    ref = _oracle(oracle, case, True, key, max_depth=kw.get("max_depth", 0), pred_on=int(option == "pred_on_parent"))
    assert _reexpands(ref["tree"]) == (option == "max_depth")
    sw, sg = _wide_handle(case, **kw), _wide_handle(case, wide=False, generic=True, **kw)
    ow, og = _wide_act(sw, case, key), _wide_act(sg, case, key)
    assert torch.equal(ow.action, og.action) and torch.equal(ow.action_weights, og.action_weights)
    assert torch.equal(sw.root_value, sg.root_value) and torch.equal(sw.search_value, sg.search_value)
    assert torch.equal(sw.depth_sum, sg.depth_sum)
    for f in ow.search_tree._fields:
        assert torch.equal(getattr(ow.search_tree, f), getattr(og.search_tree, f)), f
    _compare(ref, sg, og)
    sw.close(), sg.close()
