"""The one-launch stochastic search (mz_stoch_wide.cuh through mzs_mlp_stochastic_search): the whole search against the
CPU stepper fed the oracle-composed functions, against the three-launch route on the same handle (eager and captured),
independence of the launch geometry, guard words, MuZero(stochastic_one_launch=True) and the entry's refusals.  Every
comparison is == on the uint32 views."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import scripted_search as ss
import stochastic_mlp_reference as smr
import stochastic_search as st

pytestmark = pytest.mark.gpu
F32 = np.float32
SENTINEL = 0x5A5AA5A5  # the bit pattern untouched output words must keep
GUARD = 37             # guard words behind every output array
KEY = (4, 5)


def _emb_hbm_shape():
    """The smallest (E, S) at 3 + 5 slots whose plan keeps the embeddings out of LDS, or None."""
    from muax_amd import search
    for E in (32, 48, 64):
        for S in range(2, 40):
            pl = search.stochastic_plan(3, 5, E, 10, S)
            if pl is not None and not pl["emb_lds"]:
                return E, S
    return None


# (A, C, E, support, B, S, tiebreak, invalid mask, max_depth)
SEARCH_CASES = [
    (4, 3, 5, 8, 4, 12, False, False, None),     # the three-launch route's smallest case
    (4, 3, 5, 8, 4, 12, True, True, None),       # ... with tie-break noise and a mask
    (4, 32, 16, 10, 7, 36, False, False, None),  # 2048's shape
    (4, 32, 16, 10, 7, 36, True, False, None),
    (18, 40, 64, 31, 5, 20, True, True, None),   # 58 slots over four 16-lane rows, F = 63, E = 64, B % waves != 0
    (2, 62, 8, 8, 3, 10, False, False, None),    # all 64 lanes
    (1, 1, 1, 8, 1, 3, False, False, None),      # every width 1
    (4, 3, 5, 8, 4, 1, False, False, None),      # one simulation
    (4, 3, 5, 8, 4, 12, False, False, 3),        # max_depth reached: re-expansion, both node kinds
    (1, 1, 2, 8, 2, 70, False, False, None),     # one chain: simulations 65..70 back up over two chunks of 64 levels
    "emb_hbm",                                   # (3, 5, E*, 10, 2, S*): the plan keeps the embeddings in HBM
]


def _case_id(c):
    return c if isinstance(c, str) else "-".join(str(int(x or 0)) for x in c)


def _resolve(case):
    if case != "emb_hbm":
        return case
    es = _emb_hbm_shape()
    if es is None:
        pytest.skip("no shape with 3 + 5 slots, E <= 64 and fewer than 40 simulations keeps its embeddings out of LDS")
    return (3, 5, es[0], 10, 2, es[1], False, False, None)


@functools.lru_cache(maxsize=None)
def _search_reference(case):
    """The stepper fed the helper's functions, once per case: everything the tests compare against."""
    from oracle import pyoracle as oracle
    oracle.build()
    A, Cn, E, support, B, S, tiebreak, masked, max_depth = case
    w = smr.random_weights(11, A, Cn, E, support)
    ref = smr.StochasticMlpReference(oracle, w, A, Cn, E, support, 0.97)
    rng = np.random.default_rng([7, A, Cn, E, B, S])
    root = (rng.standard_normal((B, A)).astype(F32), rng.uniform(-3, 3, B).astype(F32), rng.uniform(0, 1, (B, E)).astype(F32))
    invalid = ss.draw_invalid(rng, B, A, all_invalid_root=False) if masked else None
    noise = rng.dirichlet([0.3] * A, B).astype(F32)
    stp = st.StochasticStepper(oracle, B, A, Cn, E, S, *root, tiebreak=tiebreak, max_depth=max_depth, key=KEY, invalid=invalid,
                               noise=noise)
    for sim in range(S):
        parent, slot, _ = stp.select(sim)
        stp.expand_backup(sim, parent, slot, ref.row(slot, stp.parent_embedding(parent).copy()))
    action, weights, value = stp.finish()
    return dict(w=w, root=root, invalid=invalid, noise=noise, action=action, weights=weights, value=value,
                depth_sum=stp.depth_sum.copy(), tree=stp.tree)


def _handle(case, w, batch=None, **cfg):
    from muax_amd import MuZeroSearch, SearchConfig
    A, Cn, E, support, B, S, tiebreak, _, max_depth = case
    s = MuZeroSearch(batch or B, SearchConfig(A, S, E, policy="stochastic", num_chance_outcomes=Cn, tiebreak=tiebreak,
                                              max_depth=max_depth, **cfg))
    s.set_stochastic_mlp_weights({k: torch.from_numpy(v).cuda() for k, v in w.items()}, support, 0.97)
    return s


def _tt(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _root_args(r, rows=slice(None)):
    return tuple(_tt(x[rows]) for x in r["root"]), _tt(None if r["invalid"] is None else r["invalid"][rows]), _tt(r["noise"][rows])


def _bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def _snapshot(s, out):
    """Host copies of everything a search returns (the handle's buffers are overwritten by the next call)."""
    tree = None if out.search_tree is None else type(out.search_tree)(*[t.clone() for t in out.search_tree])
    return dict(action=out.action.cpu().numpy().copy(), weights=out.action_weights.cpu().numpy().copy(),
                value=s.search_value.cpu().numpy().copy(), depth_sum=s.depth_sum.cpu().numpy().copy(), tree=tree)


def _check(got, r):
    from helpers import assert_trees_equal
    assert np.array_equal(r["action"], got["action"])
    assert np.array_equal(_bits(r["weights"]), _bits(got["weights"]))
    assert np.array_equal(_bits(r["value"]), _bits(got["value"]))
    assert np.array_equal(np.asarray(r["depth_sum"]).astype(np.int64), got["depth_sum"].astype(np.int64))
    assert_trees_equal(r["tree"], got["tree"], exact_floats=True)


def _same(a, b):
    """Two snapshots hold the same bits."""
    for f in ("action", "weights", "value", "depth_sum"):
        assert np.array_equal(np.ascontiguousarray(a[f]).view(np.uint32), np.ascontiguousarray(b[f]).view(np.uint32)), f
    for f in a["tree"]._fields:
        assert torch.equal(getattr(a["tree"], f).view(torch.int32), getattr(b["tree"], f).view(torch.int32)), f


@pytest.mark.parametrize("case", SEARCH_CASES, ids=_case_id)
def test_whole_search_matches_stepper(case):
    from muax_amd import search
    case = _resolve(case)
    A, Cn, E, support, B, S = case[:6]
    pl = search.stochastic_plan(A, Cn, E, support, S)
    assert pl is not None
    if case[:2] == (3, 5):
        assert not pl["emb_lds"]
    if case[0] == 18:
        assert B % pl["waves"] != 0
    r = _search_reference(case)
    s = _handle(case, r["w"])
    root, invalid, noise = _root_args(r)
    out = s.search_stochastic_mlp(root, key=list(KEY), invalid_actions=invalid, dirichlet_noise=noise, with_tree=True,
                                  one_launch=True)
    _check(_snapshot(s, out), r)
    s.close()


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("case", [SEARCH_CASES[1], SEARCH_CASES[3]], ids=_case_id)
def test_one_launch_equals_three_launches(case, graph):
    """Both routes on the SAME handle; graph: the capturing call and one replay, the replay with another key (a capture
    must not freeze the per-call values)."""
    r = _search_reference(case)
    s = _handle(case, r["w"])
    root, invalid, noise = _root_args(r)
    for key in ([list(KEY), [9, 1]] if graph else [list(KEY)]):
        kw = dict(key=key, invalid_actions=invalid, dirichlet_noise=noise, with_tree=True, temperature=0.7 if key[0] == 9 else 1.0)
        three = _snapshot(s, s.search_stochastic_mlp(root, graph=graph, **kw))
        one = _snapshot(s, s.search_stochastic_mlp(root, graph=graph, one_launch=True, **kw))
        if key == list(KEY):
            _check(one, r)
        _same(one, three)
    if graph:
        g = [v[0] for k, v in s._graphs.items() if isinstance(k, tuple) and "one_launch" in k]
        assert len(g) == 1
    s.close()


def test_result_does_not_depend_on_the_launch_geometry():
    """Five roots as one batch and as shards of 2 + 3 (global_batch / root_offset): the same bits per root, so neither
    the wavefront nor the workgroup that ran a root shows in its result.  No Gumbel row is given: the shards draw the
    rows of their global root indices."""
    case = (4, 32, 16, 10, 5, 24, True, True, None)
    r = _search_reference(case)
    whole = _handle(case, r["w"])
    root, invalid, noise = _root_args(r)
    ref = _snapshot(whole, whole.search_stochastic_mlp(root, key=list(KEY), invalid_actions=invalid, dirichlet_noise=noise,
                                                       with_tree=True, one_launch=True))
    _check(ref, r)
    whole.close()
    for off, n in ((0, 2), (2, 3)):
        rows = slice(off, off + n)
        s = _handle(case, r["w"], batch=n, global_batch=5, root_offset=off)
        root, invalid, noise = _root_args(r, rows)
        got = _snapshot(s, s.search_stochastic_mlp(root, key=list(KEY), invalid_actions=invalid, dirichlet_noise=noise,
                                                   with_tree=True, one_launch=True))
        for f in ("action", "weights", "value", "depth_sum"):
            assert np.array_equal(np.ascontiguousarray(ref[f][rows]).view(np.uint32), np.ascontiguousarray(got[f]).view(np.uint32)), f
        for f in ref["tree"]._fields:
            a, b = getattr(ref["tree"], f)[rows].contiguous(), getattr(got["tree"], f)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f
        s.close()


def test_guard_words_and_untouched_tree():
    """Through the C ABI with sentinel tails behind every output: none is written, and with export_tree == 0 the handle's
    HBM tree keeps what a three-launch search left there."""
    from muax_amd import _lib
    case = SEARCH_CASES[1]
    A, Cn, E, support, B, S = case[:6]
    r = _search_reference(case)
    s = _handle(case, r["w"])
    root, invalid, noise = _root_args(r)
    # the handle's HBM tree after a three-launch search of OTHER roots: the pattern the one-launch call must leave alone
    other = tuple(torch.flip(t, dims=[0]).contiguous() for t in root)
    before = _snapshot(s, s.search_stochastic_mlp(other, key=[1, 2], dirichlet_noise=noise, with_tree=True))
    widths = dict(action=1, action_weights=A, search_value=1, depth_sum=1)
    outs = {n: torch.full((B * k + GUARD,), SENTINEL, dtype=torch.int32, device="cuda") for n, k in widths.items()}
    a = _lib.args(_lib.MzsStochasticSearchArgs, export_tree=0, prior_logits=root[0].data_ptr(), value=root[1].data_ptr(),
                  embedding=root[2].data_ptr(), invalid_actions=invalid.data_ptr(), dirichlet_noise=noise.data_ptr(),
                  key=KEY, dirichlet_fraction=0.25, temperature=1.0, **{n: t.data_ptr() for n, t in outs.items()})
    _lib.check(s._L.mzs_mlp_stochastic_search(s._h, C.byref(a), None), s._h)
    torch.cuda.synchronize()
    got = {n: t.cpu().numpy().view(np.uint32) for n, t in outs.items()}
    for n, k in widths.items():
        assert (got[n][B * k:] == SENTINEL).all(), f"{n}: guard tail written"
    assert np.array_equal(got["action"][:B].view(np.int32), r["action"])
    assert np.array_equal(got["action_weights"][:B * A], _bits(r["weights"]).ravel())
    assert np.array_equal(got["search_value"][:B], _bits(r["value"]))
    assert np.array_equal(got["depth_sum"][:B].view(np.int32), np.asarray(r["depth_sum"]).astype(np.int32))
    tree = s._alloc_tree()
    view = s._tree_view(tree)
    _lib.check(s._L.mzs_tree_export(s._h, C.byref(view), None), s._h)
    for f in tree._fields:
        assert torch.equal(getattr(tree, f).view(torch.int32), getattr(before["tree"], f).view(torch.int32)), f
    s.close()


# ---------------------------------------------------------------- MuZero(SMZNetwork, stochastic_one_launch=True)
def _model(A=4, Cn=32, E=16, support=10, obs_dim=16, seed=0, **kw):
    import muax_amd as mx
    g = torch.Generator().manual_seed(seed)
    net = mx.create_stochastic_muzero_network(E, A, Cn, 2 * support + 1, generator=g)
    m = mx.MuZero(net, policy="stochastic", support_size=support, discount=0.97,
                  optimizer=mx.optimizers.create_optimizer("adam", 1e-2), **kw)
    m.init(0, np.zeros((1, obs_dim), F32))
    with torch.no_grad():  # haiku's zero biases hide every bias path
        for mod in net:
            for n, p in mod.named_parameters():
                if n.endswith(".b") or n == "b":
                    p.add_(0.1 * torch.randn(p.shape, generator=g).to(p.device))
    m.weights_changed()
    return m


def _act_inputs(B, A, obs_dim, seed=2):
    rng = np.random.default_rng(seed)
    obs = torch.from_numpy(rng.uniform(0, 1, (B, obs_dim)).astype(F32)).cuda()
    invalid = torch.from_numpy(ss.draw_invalid(rng, B, A, all_invalid_root=False)).cuda()
    return obs, invalid


def test_model_one_launch_route(monkeypatch):
    import muax_amd as mx
    monkeypatch.delenv("MUAX_AMD_STOCHASTIC_MLP", raising=False)
    B, A, Cn, E, od, S = 9, 4, 32, 16, 16, 20
    one, default = _model(A, Cn, E, stochastic_one_launch=True), _model(A, Cn, E)
    assert one.stochastic_one_launch and not default.stochastic_one_launch
    obs, invalid = _act_inputs(B, A, od)
    kw = dict(with_pi=True, obs_from_batch=True, num_simulations=S, invalid_actions=invalid, dirichlet_fraction=0.0,
              device_outputs=True)
    a1, w1 = one.act([3, 4], obs, **kw)
    assert one._last_route == "hip_stochastic_one_launch"
    a0, w0 = default.act([3, 4], obs, **kw)
    assert default._last_route == "hip_stochastic_mlp"
    assert torch.equal(a1, a0) and torch.equal(w1.view(torch.int32), w0.view(torch.int32))
    assert (w1[invalid.bool()] == 0).all()
    # after an update() the route searches with the rebound weights: == a search by hand on them
    rng = np.random.default_rng(4)
    batch = mx.Transition(obs=rng.uniform(0, 1, (4, 3, od)).astype(F32), a=rng.integers(0, A, (4, 3)),
                          r=rng.uniform(-1, 2, (4, 3)).astype(F32), Rn=rng.uniform(-5, 9, (4, 3)).astype(F32),
                          pi=rng.dirichlet(np.ones(A), (4, 3)).astype(F32))
    assert np.isfinite(one.update(batch)["loss"])
    a2, w2 = one.act([3, 4], obs, **kw)
    assert one._last_route == "hip_stochastic_one_launch"
    s = mx.MuZeroSearch(B, mx.SearchConfig(A, S, E, policy="stochastic", num_chance_outcomes=Cn))
    s.set_stochastic_mlp_weights({k: t.detach() for k, t in mx.nn.stochastic_mlp_weights(one.network).items()}, 10, 0.97)
    out = s.search_stochastic_mlp(one._root_inference_eager(obs), key=[3, 4], invalid_actions=invalid, dirichlet_fraction=0.0)
    assert torch.equal(out.action, a2) and torch.equal(out.action_weights.view(torch.int32), w2.view(torch.int32))
    s.close()


def test_model_declined_shape_keeps_the_three_launch_route(monkeypatch):
    monkeypatch.delenv("MUAX_AMD_STOCHASTIC_MLP", raising=False)
    A, E = 4, 70
    m = _model(A, 32, E, stochastic_one_launch=True)
    obs, invalid = _act_inputs(3, A, 16)
    _, w = m.act([3, 4], obs, with_pi=True, obs_from_batch=True, num_simulations=6, invalid_actions=invalid,
                 dirichlet_fraction=0.0, device_outputs=True)
    assert m._last_route == "hip_stochastic_mlp"
    assert (w[invalid.bool()] == 0).all()


def test_model_callable_route_is_untouched(monkeypatch):
    monkeypatch.setenv("MUAX_AMD_STOCHASTIC_MLP", "0")
    m = _model(4, stochastic_one_launch=True)
    obs, invalid = _act_inputs(3, 4, 16)
    m.act([3, 4], obs, obs_from_batch=True, num_simulations=4, invalid_actions=invalid, device_outputs=True)
    assert m._last_route == "callables"


# ---------------------------------------------------------------- refusals
def test_refusals_name_the_limit():
    """What mzs_mlp_stochastic_search refuses on the host, before any launch: the outputs keep their sentinel."""
    from muax_amd import MuZeroSearch, SearchConfig, _lib
    A, Cn, E, B = 3, 2, 4, 2
    w = {k: torch.from_numpy(v).cuda() for k, v in smr.random_weights(1, A, Cn, E, 8).items()}
    z = lambda *sh, dt=torch.float32: torch.zeros(*sh, dtype=dt, device="cuda")  # noqa: E731
    root = (z(B, A), z(B), z(B, E))
    outs = dict(action=torch.full((B,), SENTINEL, dtype=torch.int32, device="cuda"),
                action_weights=torch.full((B * A,), SENTINEL, dtype=torch.int32, device="cuda"))

    def args(**over):
        kw = dict(prior_logits=root[0].data_ptr(), value=root[1].data_ptr(), embedding=root[2].data_ptr(),
                  **{n: t.data_ptr() for n, t in outs.items()})
        kw.update(over)
        return _lib.args(_lib.MzsStochasticSearchArgs, **kw)

    def refused(h, a, code, text):
        assert h._L.mzs_mlp_stochastic_search(h._h, None if a is None else C.byref(a), None) == code
        assert h._L.mzs_last_error(h._h).decode() == "mzs_mlp_stochastic_search: " + text

    d = MuZeroSearch(B, SearchConfig(A, 3, E))
    refused(d, args(), -1, "this handle does not run the stochastic policy (policy 2)")
    s = MuZeroSearch(B, SearchConfig(A, 3, E, policy="stochastic", num_chance_outcomes=Cn))
    refused(s, args(), -1, "call mzs_mlp_set_stochastic_weights first")
    with pytest.raises(ValueError, match="set_stochastic_mlp_weights"):
        s.search_stochastic_mlp(root, one_launch=True)
    s.set_stochastic_mlp_weights(w, 8, 0.99)
    refused(s, None, -1, "null or size mismatch (ABI)")
    bad = args()
    bad.struct_size -= 8
    refused(s, bad, -1, "null or size mismatch (ABI)")
    for name in ("prior_logits", "value", "embedding"):
        refused(s, args(**{name: None}), -1, "null input")
    for name in ("action", "action_weights"):
        refused(s, args(**{name: None}), -1, "null output")
    refused(s, args(dirichlet_fraction=0.25), -1, "dirichlet_fraction != 0 needs dirichlet_noise")
    # shapes the plan declines: the typed "no kernel for this configuration" code, the limit named
    wide = MuZeroSearch(B, SearchConfig(A, 3, 70, policy="stochastic", num_chance_outcomes=Cn))
    wide.set_stochastic_mlp_weights({k: torch.from_numpy(v).cuda() for k, v in smr.random_weights(1, A, Cn, 70, 8).items()}, 8, 0.99)
    with pytest.raises(_lib.Unsupported, match=r"embed_dim must be 1\.\.64"):
        wide.search_stochastic_mlp((z(B, A), z(B), z(B, 70)), one_launch=True)
    long = MuZeroSearch(B, SearchConfig(A, 256, E, policy="stochastic", num_chance_outcomes=Cn))
    long.set_stochastic_mlp_weights(w, 8, 0.99)
    with pytest.raises(ValueError, match=r"num_simulations must be 1\.\.255"):
        long.search_stochastic_mlp(root, one_launch=True)
    torch.cuda.synchronize()
    for t in outs.values():
        assert (t.cpu().numpy().view(np.uint32) == SENTINEL).all()
    for h in (d, s, wide, long):
        h.close()
