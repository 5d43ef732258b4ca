"""The Gumbel MuZero modes of the wide-action act() kernel (mz_wide.cuh, modes 2 and 3: 17..64 actions, one root per
wavefront, one lane per action, tree in LDS) against the CPU oracle: every tree array, action, action weights, root value,
search value and depth sum with ==.  The reference is the oracle composition of test_gpu_parity.py::_gumbel_oracle_act
(root inference, mask_root_logits, gumbel_step_select / step_expand_backup per simulation, gumbel_finish), restated here
with the net options (support size, prediction on the parent, gumbel_scale) passed through.  Each check runs on a raw
MuZeroSearch handle with allow_wide(gumbel=True) ONLY, so that a decline shows as "no fused kernel instance" and not as a
silent run of the generic route."""
import warnings

import numpy as np
import pytest
import torch

from helpers import assert_trees_equal, make_case

pytestmark = pytest.mark.gpu

F32 = np.float32
QTS = ["qtransform_by_parent_and_siblings", "qtransform_completed_by_mix_value"]


def _handle(case, qt, maxc, wide=True, generic=False, pred_on="child", B=None, **cfg_kw):
    from muax_amd import MuZeroSearch, SearchConfig
    s = MuZeroSearch(case["B"] if B is None else B,
                     SearchConfig(case["A"], case["S"], case["E"], tiebreak=False, policy="gumbel", qtransform=QTS[qt],
                                  max_num_considered_actions=maxc, **cfg_kw))
    s.set_mlp_weights({k: torch.from_numpy(v) for k, v in case["w"].items()}, case["obs_dim"], case["support"], 0.99, pred_on)
    if wide:
        s.allow_wide(gumbel=True)
    if generic:
        s.allow_generic()
    return s


def _act(s, case, key, rows=slice(None), with_tree=True, use_gumbel=True):
    out = s.act_mlp(torch.from_numpy(case["obs"][rows]), key,
                    invalid_actions=None if case["invalid"] is None else torch.from_numpy(case["invalid"][rows]),
                    gumbel=torch.from_numpy(case["gumbel"][rows]) if use_gumbel else None, with_tree=with_tree)
    torch.cuda.synchronize()
    return out


def _oracle(oracle, case, key, qt, maxc, use_gumbel=True, max_depth=0, pred_on=0, gumbel_scale=1.0):
    """mctx.gumbel_muzero_policy around the oracle's MLP trio, composed from the oracle's pieces."""
    B, A, E, S = case["B"], case["A"], case["E"], case["S"]
    mlp = oracle.Mlp(case["w"], case["obs_dim"], E, A, case["F"], support_size=case["support"], recurrent_pred_on=pred_on,
                     discount=0.99)
    pl, v, emb = oracle.root_inference(mlp, case["obs"])
    # the root noise: the array as given, or gumbel_scale * jax.random.gumbel(split(key)[1], [B, A])
    g = case["gumbel"] if use_gumbel else F32(gumbel_scale) * oracle.gumbel(oracle.split(key, 2)[1], B * A).reshape(B, A)
    tree = oracle.Tree(B, S + 1, A, E)
    cfg = oracle.SearchCfg(S, max_depth=max_depth)
    oracle.tree_init(tree, oracle.mask_root_logits(pl, case["invalid"]), v, emb, case["invalid"])
    dsum = np.zeros(B, np.int64)
    for sim in range(S):
        p_, a_, d_ = oracle.gumbel_step_select(tree, cfg, g, qt, maxc)
        dsum += d_
        oracle.step_expand_backup(tree, sim, p_, a_, *oracle.recurrent_inference(mlp, a_, tree.embeddings[np.arange(B), p_]))
    action, weights = oracle.gumbel_finish(tree, g, qt)
    return {"action": action, "action_weights": weights, "root_value": v, "depth_sum": dsum, "tree": tree}


def _compare_outputs(ref, s, out):
    assert np.array_equal(ref["action"], out.action.cpu().numpy())
    assert np.array_equal(ref["action_weights"], out.action_weights.cpu().numpy())
    assert np.array_equal(ref["root_value"], s.root_value.cpu().numpy())
    assert np.array_equal(ref["depth_sum"], s.depth_sum.cpu().numpy().astype(np.int64))
    assert np.array_equal(ref["tree"].node_values[:, 0], s.search_value.cpu().numpy())


def _compare(ref, s, out):
    _compare_outputs(ref, s, out)
    assert_trees_equal(ref["tree"], out.search_tree, exact_floats=True)


def _depths(parents):
    depth = np.zeros_like(parents)
    for k in range(1, parents.shape[1]):
        live = parents[:, k] >= 0
        depth[live, k] = depth[np.arange(len(parents))[live], parents[live, k]] + 1
    return depth


_S_OF = {17: 120, 18: 50, 31: 70, 32: 40, 33: 100, 48: 60, 64: 20}


@pytest.mark.parametrize("qt", [0, 1])
@pytest.mark.parametrize("E", [8, 20, 64])
@pytest.mark.parametrize("A", [17, 18, 31, 32, 33, 48, 64])
def test_wide_gumbel_shape_sweep_matches_oracle(oracle, A, E, qt):
    """Every slot boundary of the 16-wide canonical sums x embeddings of 8, 20 and 64 x both qtransforms, 20 .. 120
    simulations, ragged batches, both support sizes, max_num_considered_actions of 5, 16 and A, invalid actions: one row
    with every action masked, one with a single valid action, one with three (fewer than any max_num_considered_actions
    here), the others with about a fifth masked (at A = 17 / 18 some of those have fewer than 16 valid actions)."""
    from muax_amd.search import wide_plan
    S, B = _S_OF[A], (5, 97, 130)[(A + E // 8) % 3]
    maxc = (5, 16, A)[(A + E // 8 + qt) % 3]
    support = 10 if (A + E) % 2 else 20
    assert wide_plan(A, E, support, S, policy="gumbel") is not None
    case = make_case(oracle, 1700 + A + E, B, 6, E, A, S, support=support, invalid_frac=0.2)
    case["invalid"][1, :] = 1
    case["invalid"][1, A - 2] = 0
    case["invalid"][2, :] = 1
    case["invalid"][2, [0, 7, A - 1]] = 0
    assert ((case["invalid"] == 0).sum(axis=1) < maxc).sum() >= 3
    key = [43, A + E]
    s = _handle(case, qt, maxc)
    out = _act(s, case, key)
    _compare(_oracle(oracle, case, key, qt, maxc), s, out)
    assert int(out.action[1]) == A - 2 and int(out.search_tree.children_visits[1, 0, A - 2]) == S
    s.close()


@pytest.mark.parametrize("qt", [0, 1])
def test_wide_gumbel_noise_from_the_key_and_sharding(oracle, qt):
    """No noise array: the root Gumbel noise is drawn from split(key)[1] per GLOBAL root -- the whole batch against the
    oracle, and the same batch as two shards (global_batch / root_offset) giving the same rows."""
    A, E, S, B = 18, 8, 40, 300
    case = make_case(oracle, 1811 + qt, B, 6, E, A, S, invalid_frac=0.2)
    key = [9, S]
    s = _handle(case, qt, 8)
    full = _act(s, case, key, use_gumbel=False)
    _compare(_oracle(oracle, case, key, qt, 8, use_gumbel=False), s, full)
    for lo, hi in ((0, 172), (172, 300)):
        rows = slice(lo, hi)
        sh = _handle(case, qt, 8, B=hi - lo, global_batch=B, root_offset=lo)
        part = _act(sh, case, key, rows=rows, use_gumbel=False)
        assert torch.equal(full.action[rows], part.action) and torch.equal(full.action_weights[rows], part.action_weights)
        assert torch.equal(s.search_value[rows], sh.search_value) and torch.equal(s.depth_sum[rows], sh.depth_sum)
        for f in full.search_tree._fields:
            assert torch.equal(getattr(full.search_tree, f)[rows], getattr(part.search_tree, f)), f
        sh.close()
    s.close()


@pytest.mark.parametrize("qt", [0, 1])
def test_wide_gumbel_options_match_oracle(oracle, qt):
    A, E, S, B = 18, 8, 40, 61
    case = make_case(oracle, 1821, B, 6, E, A, S, invalid_frac=0.2)
    key = [5, 6]
    for max_depth in (3, 9):  # re-expansions at the depth limit
        s = _handle(case, qt, 16, max_depth=max_depth)
        out = _act(s, case, key)
        _compare(_oracle(oracle, case, key, qt, 16, max_depth=max_depth), s, out)
        assert (out.search_tree.node_visits.cpu().numpy()[:, 1:].max(axis=1) > 1).any()
        s.close()
    s = _handle(case, qt, 16, pred_on="parent")  # the prediction net on the parent's embedding
    _compare(_oracle(oracle, case, key, qt, 16, pred_on=1), s, _act(s, case, key))
    s.close()
    for scale in (0.5, 3.0):  # gumbel_scale scales the noise drawn from the key
        s = _handle(case, qt, 16, gumbel_scale=scale)
        _compare(_oracle(oracle, case, key, qt, 16, use_gumbel=False, gumbel_scale=scale), s, _act(s, case, key, use_gumbel=False))
        s.close()
    s = _handle(case, qt, 1)  # one considered action: every simulation goes through it
    out = _act(s, case, key)
    _compare(_oracle(oracle, case, key, qt, 1), s, out)
    assert (out.search_tree.children_visits.cpu().numpy()[:, 0].max(axis=1) == S).all()
    s.close()
    case["invalid"] = None  # no mask at all
    s = _handle(case, qt, 16)
    _compare(_oracle(oracle, case, key, qt, 16), s, _act(s, case, key))
    s.close()


@pytest.mark.parametrize("qt,maxc,S", [(0, 1, 120), (1, 2, 170)])
def test_wide_gumbel_deep_paths_beyond_64_levels(oracle, qt, maxc, S):
    """One action dominates the prior and sequential halving considers one (two) root actions: the interior selection
    digs single lines past 64 levels -- backup chunks of 64 levels with the return and the child value carried from chunk
    to chunk.  (Weights and seed were chosen with the oracle; the depth is asserted on the oracle's own tree.)"""
    A, E = 18, 8
    case = make_case(oracle, 46, 9, 4, E, A, S)
    case["w"]["pp_b2"] = np.array([7.0] + [-7.0] * (A - 1), F32)
    ref = _oracle(oracle, case, [3, 1], qt, maxc)
    depth = _depths(ref["tree"].parents)
    assert depth.max() > 64 and (depth.max(axis=1) > 64).sum() >= 5
    s = _handle(case, qt, maxc)
    out = _act(s, case, [3, 1])
    _compare(ref, s, out)
    assert np.array_equal(_depths(out.search_tree.parents.cpu().numpy()), depth)
    s.close()


@pytest.mark.parametrize("A,E,S,qt", [(18, 8, 50, 1), (18, 32, 50, 0), (64, 64, 90, 1)])
def test_wide_gumbel_without_export_and_handle_reuse(oracle, A, E, S, qt):
    """Two acts with different keys on one handle without a tree export, then one with (E = 32 and 64 x 64 keep their
    embeddings in HBM: the handle's scratch without an export, the caller's buffer with one)."""
    from muax_amd.search import wide_plan
    assert wide_plan(A, E, 10, S, policy="gumbel")["emb_lds"] == (E == 8)
    case = make_case(oracle, 1640 + A + E, 75, 6, E, A, S, invalid_frac=0.2)
    s = _handle(case, qt, 16)
    for key in ([5, S], [6, A]):
        out = _act(s, case, key, with_tree=False, use_gumbel=False)
        assert out.search_tree is None
        _compare_outputs(_oracle(oracle, case, key, qt, 16, use_gumbel=False), s, out)
    _compare(_oracle(oracle, case, [7, 7], qt, 16), s, _act(s, case, [7, 7]))
    s.close()


def test_wide_gumbel_full_size(oracle):
    """4096 roots, 18 actions, 8-wide embedding, 50 simulations: the whole tree against the oracle."""
    A, E, S, B = 18, 8, 50, 4096
    case = make_case(oracle, 1902, B, 6, E, A, S, invalid_frac=0.2)
    key = [9, S]
    s = _handle(case, 1, 16)
    out = _act(s, case, key, use_gumbel=False)
    _compare(_oracle(oracle, case, key, 1, 16, use_gumbel=False), s, out)
    s.close()


@pytest.mark.parametrize("qt", [0, 1])
def test_wide_gumbel_same_bits_as_generic_route(oracle, qt):
    case = make_case(oracle, 1333, 150, 6, 12, 33, 60, invalid_frac=0.2)
    key = [8, 9]
    sw, sg = _handle(case, qt, 16), _handle(case, qt, 16, wide=False, generic=True)
    ow, og = _act(sw, case, key), _act(sg, case, key)
    assert torch.equal(ow.action, og.action) and torch.equal(ow.action_weights, og.action_weights)
    assert torch.equal(sw.root_value, sg.root_value) and torch.equal(sw.search_value, sg.search_value)
    assert torch.equal(sw.depth_sum, sg.depth_sum)
    for f in ow.search_tree._fields:
        assert torch.equal(getattr(ow.search_tree, f), getattr(og.search_tree, f)), f
    sw.close(), sg.close()


def test_wide_gumbel_declines(oracle):
    from muax_amd.search import wide_plan
    # 64 actions x 130 simulations: the MuZero record fits a CU's LDS, the Gumbel record (a fifth field) does not
    A, E, S = 64, 8, 130
    assert wide_plan(A, E, 10, S) is not None and wide_plan(A, E, 10, S, policy="gumbel") is None
    case = make_case(oracle, 1171, 11, 5, E, A, S, invalid_frac=0.2)
    s = _handle(case, 1, 16)
    with pytest.raises(ValueError, match="no fused kernel instance"):
        _act(s, case, [1, 2])
    s.close()
    s = _handle(case, 1, 16, generic=True)
    _compare(_oracle(oracle, case, [1, 2], 1, 16), s, _act(s, case, [1, 2]))
    s.close()
    # the MuZero opt-in alone does not serve a Gumbel handle, and the Gumbel opt-in does not serve 16 actions
    case = make_case(oracle, 1172, 20, 5, 8, 18, 30)
    s = _handle(case, 0, 16, wide=False)
    s.allow_wide()
    with pytest.raises(ValueError, match="no fused kernel instance"):
        _act(s, case, [4, 4])
    s.allow_wide(gumbel=True)
    _compare(_oracle(oracle, case, [4, 4], 0, 16), s, _act(s, case, [4, 4]))
    s.allow_wide(False, gumbel=True)  # ... and it can be taken back
    with pytest.raises(ValueError, match="no fused kernel instance"):
        _act(s, case, [4, 4])
    s.close()


def _model_with(w, E, A, obs_dim):
    import muax_amd as mx
    g = torch.Generator().manual_seed(0)
    net = mx.nn.MZNetwork(mx.nn.Representation(E, generator=g), mx.nn.Prediction(A, 21, generator=g),
                          mx.nn.Dynamic(E, A, 21, generator=g))
    m = mx.MuZero(net, policy_class=mx.policy.GumbelMuZeroPolicy)
    m.init(mx.prng.PRNGKey(0), np.zeros((1, obs_dim)))
    with torch.no_grad():
        for k, p in mx.nn.mlp_trio_weights(m.network).items():
            p.copy_(torch.from_numpy(w[k]))
    m.weights_changed()
    return m


def test_wide_gumbel_through_muzero_act(oracle, monkeypatch):
    """MuZero(policy_class=GumbelMuZeroPolicy).act() on an 18-action default trio with the generic route switched off and
    warnings as errors: NumPy in / out (mzs_act_mlp_host) and device outputs both equal the oracle, no step-wise warning;
    with MUAX_AMD_WIDE=0 and the generic route allowed the outputs are identical."""
    import muax_amd as mx
    A, E, obs_dim, S, B = 18, 8, 6, 30, 45
    w = oracle.random_mlp_weights(59, obs_dim, E, A, 21, bias_scale=0.1)
    obs = np.random.default_rng(B).uniform(-1, 1, (B, obs_dim)).astype(F32)
    case = dict(w=w, obs=obs, invalid=None, gumbel=None, B=B, obs_dim=obs_dim, E=E, A=A, F=21, S=S, support=10)
    key = mx.prng.PRNGKey(4321)
    ref = _oracle(oracle, case, key, 0, 16, use_gumbel=False)  # act()'s defaults: by_parent_and_siblings, 16 considered
    monkeypatch.setenv("MUAX_AMD_GENERIC", "0")
    m = _model_with(w, E, A, obs_dim)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        a, pi, v = m.act(key, obs, with_pi=True, with_value=True, obs_from_batch=True, num_simulations=S)
        ad, pid, vd = m.act(key, torch.from_numpy(obs).cuda(), with_pi=True, with_value=True, obs_from_batch=True,
                            num_simulations=S, device_outputs=True)
    assert np.array_equal(a, ref["action"]) and np.array_equal(pi, ref["action_weights"]) and np.array_equal(v, ref["root_value"])
    assert ad.is_cuda and np.array_equal(ad.cpu().numpy(), a) and np.array_equal(pid.cpu().numpy(), pi)
    assert np.array_equal(vd.cpu().numpy(), v)
    monkeypatch.setenv("MUAX_AMD_GENERIC", "1")
    monkeypatch.setenv("MUAX_AMD_WIDE", "0")
    m2 = _model_with(w, E, A, obs_dim)
    a2, pi2, v2 = m2.act(key, obs, with_pi=True, with_value=True, obs_from_batch=True, num_simulations=S)
    assert np.array_equal(a2, a) and np.array_equal(pi2, pi) and np.array_equal(v2, v)
