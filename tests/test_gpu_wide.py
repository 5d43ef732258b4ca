"""The wide-action act() kernel (mz_wide.cuh: 17..64 actions, MuZero policy, one root per wavefront, one lane per action,
tree in LDS) against the CPU oracle: every tree array, action, weights, root value, search value and depth sum with ==.
Each check runs on a raw MuZeroSearch handle with allow_wide() ONLY, so that a decline shows as "no fused kernel
instance" and not as a silent run of the generic route."""
import warnings

import numpy as np
import pytest
import torch

from helpers import assert_trees_equal, make_case

pytestmark = pytest.mark.gpu

F32 = np.float32


def _handle(case, tiebreak=True, wide=True, generic=False, policy="muzero", pred_on="child", B=None, **cfg_kw):
    from muax_amd import MuZeroSearch, SearchConfig
    s = MuZeroSearch(case["B"] if B is None else B, SearchConfig(case["A"], case["S"], case["E"], tiebreak=tiebreak, policy=policy,
                                                                 **cfg_kw))
    s.set_mlp_weights({k: torch.from_numpy(v) for k, v in case["w"].items()}, case["obs_dim"], case["support"], 0.99, pred_on)
    if wide:
        s.allow_wide()
    if generic:
        s.allow_generic()
    return s


def _act(s, case, key, rows=slice(None), with_tree=True, use_noise=True, use_gumbel=True, temperature=1.0, policy="muzero"):
    args = dict(invalid_actions=None if case["invalid"] is None else torch.from_numpy(case["invalid"][rows]), with_tree=with_tree,
                temperature=temperature, gumbel=torch.from_numpy(case["gumbel"][rows]) if use_gumbel else None)
    if policy == "muzero" and use_noise:
        args["dirichlet_noise"] = torch.from_numpy(case["noise"][rows])
    out = s.act_mlp(torch.from_numpy(case["obs"][rows]), key, **args)
    torch.cuda.synchronize()
    return out


def _oracle(oracle, case, tiebreak, key, max_depth=0, temperature=1.0, use_gumbel=True, use_noise=True, pred_on=0):
    mlp = oracle.Mlp(case["w"], case["obs_dim"], case["E"], case["A"], case["F"], support_size=case["support"],
                     recurrent_pred_on=pred_on, discount=0.99)
    cfg = oracle.SearchCfg(case["S"], max_depth=max_depth or 0, tiebreak=int(tiebreak))
    return oracle.act_mlp(mlp, cfg, case["obs"], key, case["noise"] if use_noise else None, 0.25, case["invalid"],
                          temperature, case["gumbel"] if use_gumbel else None)


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


@pytest.mark.parametrize("E", [8, 20, 64])
@pytest.mark.parametrize("A", [17, 18, 31, 32, 33, 48, 64])
def test_wide_shape_sweep_matches_oracle(oracle, A, E):
    """Every slot boundary of the 16-wide canonical sums (17, 31 .. 33, 48, 64 actions) x embeddings of 8, 20 and 64,
    20 .. 120 simulations, ragged batches, both support sizes, invalid actions (one row with every action masked)."""
    from muax_amd.search import wide_plan
    S, B = _S_OF[A], (1, 97, 130)[(A + E // 8) % 3]
    support = 10 if (A + E) % 2 else 20
    assert wide_plan(A, E, support, S) is not None
    case = make_case(oracle, 700 + A + E, B, 6, E, A, S, support=support, invalid_frac=0.2)
    key = [41, A + E]
    s = _handle(case)
    out = _act(s, case, key)
    _compare(_oracle(oracle, case, True, key), s, out)
    s.close()


def test_wide_options_match_oracle(oracle):
    A, E, S, B = 18, 8, 40, 61
    case = make_case(oracle, 811, B, 6, E, A, S, invalid_frac=0.2)
    key = [5, 6]
    # no tie-break noise; the prediction net on the parent's embedding; the categorical's Gumbel from the key
    s = _handle(case, tiebreak=False, pred_on="parent")
    _compare(_oracle(oracle, case, False, key, pred_on=1, use_gumbel=False), s, _act(s, case, key, use_gumbel=False))
    s.close()
    for max_depth in (3, 9):  # re-expansions at the depth limit
        s = _handle(case, max_depth=max_depth)
        out = _act(s, case, key)
        _compare(_oracle(oracle, case, True, key, max_depth=max_depth), s, out)
        assert (out.search_tree.node_visits.cpu().numpy()[:, 1:].max(axis=1) > 1).any()
        s.close()
    for temperature in (0.25, 1.0):
        s = _handle(case)
        _compare(_oracle(oracle, case, True, key, temperature=temperature), s, _act(s, case, key, temperature=temperature))
        s.close()
    s = _handle(case)  # dirichlet_fraction = 0: no noise array
    _compare(_oracle(oracle, case, True, key, use_noise=False), s, _act(s, case, key, use_noise=False))
    s.close()
    # a row whose mask leaves exactly one valid action
    case["invalid"][3, :] = 1
    case["invalid"][3, 11] = 0
    s = _handle(case)
    out = _act(s, case, key)
    _compare(_oracle(oracle, case, True, key), s, out)
    assert int(out.action[3]) == 11 and int(out.search_tree.children_visits[3, 0, 11]) == S
    s.close()


def test_wide_all_ties_noise_decides(oracle):
    """All-zero weights: uniform priors, zero values and rewards -- every decision at every level is an exact tie among
    18 (33) actions and mctx's 1e-7 * uniform noise decides it (the lazily advanced threefry key walk at every depth)."""
    for A, S in ((18, 40), (33, 30)):
        case = make_case(oracle, 77, 37, 4, 8, A, S)
        case["w"] = {k: np.zeros_like(v) for k, v in case["w"].items()}
        key = [11, 22]
        s = _handle(case)
        out = _act(s, case, key, use_noise=False)
        _compare(_oracle(oracle, case, True, key, use_noise=False), s, out)
        s0 = _handle(case, tiebreak=False)
        out0 = _act(s0, case, key, use_noise=False)
        _compare(_oracle(oracle, case, False, key, use_noise=False), s0, out0)
        assert not torch.equal(out.search_tree.children_index, out0.search_tree.children_index)
        s.close(), s0.close()
    case = make_case(oracle, 78, 40, 4, 8, 20, 40)  # margins around the noise scale: near ties and clear decisions mixed
    case["w"] = {k: (v * 1e-4).astype(F32) for k, v in case["w"].items()}
    s = _handle(case)
    _compare(_oracle(oracle, case, True, [5, 5], use_noise=False), s, _act(s, case, [5, 5], use_noise=False))
    s.close()


@pytest.mark.parametrize("A,E,noise", [(18, 8, True), (40, 20, False)])
def test_wide_deep_paths_beyond_64_and_100_levels(oracle, A, E, noise):
    """One action dominates the prior: the search digs a single line past 16, 64 and 100 levels -- backup chunks of 64
    levels with the return and the child value carried from chunk to chunk."""
    case = make_case(oracle, 46, 9, 4, E, A, 120)
    case["w"]["pp_b2"] = np.array([7.0] + [-7.0] * (A - 1), F32)
    for tiebreak in (True, False):
        s = _handle(case, tiebreak=tiebreak)
        out = _act(s, case, [3, 1], use_noise=noise)
        ref = _oracle(oracle, case, tiebreak, [3, 1], use_noise=noise)
        _compare(ref, s, out)
        s.close()
    depth = _depths(out.search_tree.parents.cpu().numpy())
    assert depth.max() > 100 and (depth.max(axis=1) > 64).all()


def test_wide_full_size_and_sharding(oracle):
    """The bar's shape -- 4096 roots, 18 actions, 8-wide embedding, 50 simulations -- whole tree against the oracle, and
    the same batch in two shards of 2048 (root_offset / global_batch) giving the same rows."""
    A, E, S, B = 18, 8, 50, 4096
    case = make_case(oracle, 902, B, 6, E, A, S, invalid_frac=0.2)
    key = [9, S]
    s = _handle(case)
    full = _act(s, case, key, use_gumbel=False)
    _compare(_oracle(oracle, case, True, key, use_gumbel=False), s, full)
    for lo in (0, 2048):
        rows = slice(lo, lo + 2048)
        sh = _handle(case, B=2048, global_batch=B, root_offset=lo)
        part = _act(sh, case, key, rows=rows, use_gumbel=False)
        assert torch.equal(full.action[rows], part.action) and torch.equal(full.action_weights[rows], part.action_weights)
        assert torch.equal(s.search_value[rows], sh.search_value) and torch.equal(s.depth_sum[rows], sh.depth_sum)
        for f in full.search_tree._fields:
            assert torch.equal(getattr(full.search_tree, f)[rows], getattr(part.search_tree, f)), f
        sh.close()
    s.close()


@pytest.mark.parametrize("A,E,S", [(18, 8, 50), (64, 64, 110)])
def test_wide_without_export_and_handle_reuse(oracle, A, E, S):
    """Two acts with different keys on one handle without a tree export, then one with (64 x 64 at 110 simulations keeps
    its embeddings in HBM: the handle's scratch without an export, the caller's buffer with one)."""
    from muax_amd.search import wide_plan
    assert wide_plan(A, E, 10, S)["emb_lds"] == (A == 18)
    case = make_case(oracle, 640 + A, 75, 6, E, A, S, invalid_frac=0.2)
    s = _handle(case)
    for key in ([5, S], [6, A]):
        out = _act(s, case, key, with_tree=False)
        assert out.search_tree is None
        _compare_outputs(_oracle(oracle, case, True, key), s, out)
    _compare(_oracle(oracle, case, True, [7, 7]), s, _act(s, case, [7, 7]))
    s.close()


def test_wide_same_bits_as_generic_route(oracle):
    case = make_case(oracle, 333, 150, 6, 12, 33, 60, invalid_frac=0.2)
    key = [8, 9]
    sw, sg = _handle(case), _handle(case, wide=False, generic=True)
    ow, og = _act(sw, case, key, use_gumbel=False), _act(sg, case, key, use_gumbel=False)
    assert torch.equal(ow.action, og.action) and torch.equal(ow.action_weights, og.action_weights)
    assert torch.equal(sw.root_value, sg.root_value) and torch.equal(sw.search_value, sg.search_value)
    assert torch.equal(sw.depth_sum, sg.depth_sum)
    for f in ow.search_tree._fields:
        assert torch.equal(getattr(ow.search_tree, f), getattr(og.search_tree, f)), f
    sw.close(), sg.close()


def test_wide_declines(oracle):
    from muax_amd.search import wide_plan
    # a Gumbel handle: declined, and with the generic route allowed too it is served there as before
    case = make_case(oracle, 170, 30, 5, 8, 18, 40, invalid_frac=0.3)
    kw = dict(policy="gumbel", qtransform="qtransform_completed_by_mix_value", max_num_considered_actions=16)
    s = _handle(case, tiebreak=False, **kw)
    with pytest.raises(ValueError, match="no fused kernel instance"):
        _act(s, case, [23, 40], policy="gumbel")
    s.close()
    s, g = _handle(case, tiebreak=False, generic=True, **kw), _handle(case, tiebreak=False, wide=False, generic=True, **kw)
    o1, o2 = _act(s, case, [23, 40], policy="gumbel"), _act(g, case, [23, 40], policy="gumbel")
    assert torch.equal(o1.action, o2.action) and torch.equal(o1.action_weights, o2.action_weights)
    for f in o1.search_tree._fields:
        assert torch.equal(getattr(o1.search_tree, f), getattr(o2.search_tree, f)), f
    s.close(), g.close()
    # one root beyond a CU's LDS: the budget formula says so, the kernel declines, the generic route serves it
    A, E, S = 64, 8, 255
    declined = wide_plan(A, E, 10, S) is None
    assert declined == (4 * ((S + 1) * (4 + 4 * A + 1)) > 160 * 1024)  # the records and the path alone exceed it
    case = make_case(oracle, 171, 11, 5, E, A, S, invalid_frac=0.2)
    s = _handle(case)
    if declined:
        with pytest.raises(ValueError, match="no fused kernel instance"):
            _act(s, case, [1, 2])
    s.close()
    s = _handle(case, generic=True)
    _compare(_oracle(oracle, case, True, [1, 2]), s, _act(s, case, [1, 2]))
    s.close()
    # 16 actions: served or refused exactly as without allow_wide
    case = make_case(oracle, 172, 20, 5, 8, 16, 50)
    res = []
    for wide in (False, True):
        s = _handle(case, wide=wide)
        try:
            out = _act(s, case, [4, 4])
            res.append(("ok", out.action.cpu().numpy().tolist(), out.search_tree.children_visits.cpu().numpy().tolist()))
        except ValueError as e:
            res.append(("refused", str(e)))
        s.close()
    assert res[0] == res[1]


def _model_with(w, E, A, obs_dim):
    import muax_amd as mx
    g = torch.Generator().manual_seed(0)
    net = mx.nn.MZNetwork(mx.nn.Representation(E, generator=g), mx.nn.Prediction(A, 21, generator=g),
                          mx.nn.Dynamic(E, A, 21, generator=g))
    m = mx.MuZero(net, policy="muzero")
    m.init(mx.prng.PRNGKey(0), np.zeros((1, obs_dim)))
    with torch.no_grad():
        for k, p in mx.nn.mlp_trio_weights(m.network).items():
            p.copy_(torch.from_numpy(w[k]))
    m.weights_changed()
    return m


def test_wide_through_muzero_act(oracle, monkeypatch):
    """MuZero.act() on an 18-action default trio with the generic route switched off and warnings as errors: NumPy in /
    out (mzs_act_mlp_host) and device outputs both equal the oracle, no step-wise warning; with MUAX_AMD_WIDE=0 and the
    generic route allowed the outputs are identical."""
    import muax_amd as mx
    A, E, obs_dim, S, B = 18, 8, 6, 30, 45
    w = oracle.random_mlp_weights(58, obs_dim, E, A, 21, bias_scale=0.1)
    obs = np.random.default_rng(B).uniform(-1, 1, (B, obs_dim)).astype(F32)
    mlp, cfg = oracle.Mlp(w, obs_dim, E, A, 21), oracle.SearchCfg(S, tiebreak=1)
    key = mx.prng.PRNGKey(4321)
    noise = oracle.dirichlet(oracle.split(key, 3)[1], 0.3, B, A)
    ref = oracle.act_mlp(mlp, cfg, obs, key, noise, 0.25, None, 1.0, None)
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
