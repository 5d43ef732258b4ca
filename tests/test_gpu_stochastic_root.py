"""Root inference of the default stochastic MLP family inside the library (mz_stoch_wide.cuh: mz_stoch_root_kernel and the
ROOT instantiations of mz_stoch_wide_kernel, through mzs_mlp_stochastic_root / mzs_mlp_stochastic_search_obs): the root
kernel against the C oracle's root_inference at the edges of its loop and mapping, the one-launch search on
observations against itself on the oracle's RootFnOutput (eager and captured), the three-launch route, independence of
the launch geometry, guard words, the refusals, MuZero(stochastic_root_in_kernel=True) and -- the only comparison that
is not == on the uint32 views -- the distance to the modules evaluated in float64, next to torch fp32's own."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import scripted_search as ss
import stochastic_mlp_reference as smr

pytestmark = pytest.mark.gpu
F32 = np.float32
H = 16
SENTINEL = 0x5A5AA5A5  # the bit pattern untouched output words must keep
GUARD = 37             # guard words behind every output array
KEY = (4, 5)
OBS_DIM = 7            # of the search cases: one block of four and a tail


def _oracle():
    from oracle import pyoracle as oracle
    oracle.build()
    return oracle


def _family(seed, obs_dim, A, Cn, E, support, repr_bias=0.1):
    """The 28 arrays of the decision and chance function and the representation's two."""
    w = smr.random_weights(seed, A, Cn, E, support)
    rng = np.random.default_rng([seed, obs_dim, E])
    repr_w = (np.clip(rng.standard_normal((obs_dim, E)), -2, 2) / np.sqrt(obs_dim)).astype(F32)
    repr_b = (repr_bias * rng.standard_normal(E)).astype(F32)
    return w, repr_w, repr_b


def _root_reference(w, repr_w, repr_b, A, E, support, obs):
    """oracle.root_inference on an oracle.Mlp of the representation and the prediction heads, zero dynamics."""
    oracle = _oracle()
    F = 2 * support + 1
    z = lambda *s: np.zeros(s, F32)  # noqa: E731
    ws = {"repr_w": repr_w, "repr_b": repr_b}
    ws.update({f"{h}_{a}": w[f"{h}_{a}"] for h in ("pv", "pp") for a in ("w1", "b1", "w2", "b2")})
    for pre, out in (("dr", F), ("dn", E)):
        ws.update({f"{pre}_w1": z(E + A, H), f"{pre}_b1": z(H), f"{pre}_w2": z(H, out), f"{pre}_b2": z(out)})
    return oracle.root_inference(oracle.Mlp(ws, repr_w.shape[0], E, A, F, support_size=support), obs)


def _tt(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def _handle(A, Cn, E, support, B, S, w, repr_w, repr_b, **cfg):
    from muax_amd import MuZeroSearch, SearchConfig
    s = MuZeroSearch(B, SearchConfig(A, S, E, policy="stochastic", num_chance_outcomes=Cn, **cfg))
    s.set_stochastic_mlp_weights({k: _tt(v) for k, v in w.items()}, support, 0.97)
    s.set_stochastic_representation(_tt(repr_w), _tt(repr_b))
    return s


# ---------------------------------------------------------------- the root kernel against the oracle
# (obs_dim, E, A, C, support, B): obs_dim 1 and 3 tail only, 4 one block, 5 block + tail, 131 a long row; E 1 (width-1
# normalisation: the scale < 1e-5 branch), 5, 64 (all lanes); A 1 and 18; A + C = 64; support 8 and 31 (F = 17, 63);
# B = 5 is no multiple of the four waves of a workgroup
ROOT_CASES = [
    (1, 1, 1, 1, 8, 5),
    (3, 5, 4, 3, 8, 5),
    (4, 5, 18, 46, 31, 5),
    (5, 64, 18, 40, 31, 5),
    (131, 64, 1, 63, 8, 5),
    (131, 5, 18, 3, 31, 5),
    "constant",  # all-zero observations, a constant bias: a constant embedding, the scale < 1e-5 branch at E = 5
]


def _root_case(case):
    if case != "constant":
        obs_dim, E, A, Cn, support, B = case
        w, repr_w, repr_b = _family(3, obs_dim, A, Cn, E, support)
        obs = np.random.default_rng([5, obs_dim, E]).uniform(-1, 1, (B, obs_dim)).astype(F32)
        return (obs_dim, E, A, Cn, support, B), w, repr_w, repr_b, obs
    obs_dim, E, A, Cn, support, B = 4, 5, 4, 3, 8, 5
    w, repr_w, _ = _family(3, obs_dim, A, Cn, E, support)
    return (obs_dim, E, A, Cn, support, B), w, repr_w, np.full(E, 0.375, F32), np.zeros((B, obs_dim), F32)


@pytest.mark.parametrize("case", ROOT_CASES, ids=lambda c: c if isinstance(c, str) else "-".join(map(str, c)))
def test_root_kernel_matches_oracle(case):
    (obs_dim, E, A, Cn, support, B), w, repr_w, repr_b, obs = _root_case(case)
    logits, value, emb = _root_reference(w, repr_w, repr_b, A, E, support, obs)
    if case == "constant":
        assert (emb == 0).all()  # (s - min) / (0 + 1e-5) of a constant row
    s = _handle(A, Cn, E, support, B, 2, w, repr_w, repr_b)
    got = s.stochastic_mlp_root(_tt(obs))
    assert got[1] is s.root_value
    assert tuple(got[0].shape) == (B, A) and tuple(got[1].shape) == (B,) and tuple(got[2].shape) == (B, E)
    assert np.array_equal(_bits(logits), _bits(got[0].cpu().numpy()))
    assert np.array_equal(_bits(value), _bits(got[1].cpu().numpy()))
    assert np.array_equal(_bits(emb), _bits(got[2].cpu().numpy()))
    s.close()


# ---------------------------------------------------------------- the search on observations
def _emb_hbm_shape():
    """The smallest (E, S) at 3 + 5 slots whose plan keeps the embeddings out of LDS, or None."""
    from muax_amd import search
    for E in (32, 48, 64):
        for S in range(2, 40):
            pl = search.stochastic_plan(3, 5, E, 10, S)
            if pl is not None and not pl["emb_lds"]:
                return E, S
    return None


# (A, C, E, support, B, S, tiebreak, invalid mask, max_depth): rows 1, 3, 5, 6 and 7 of test_gpu_stochastic_one_launch.py's
# SEARCH_CASES and its emb_hbm case
SEARCH_CASES = [
    (4, 3, 5, 8, 4, 12, False, False, None),     # the three-launch route's smallest case
    (4, 32, 16, 10, 7, 36, False, False, None),  # 2048's shape
    (18, 40, 64, 31, 5, 20, True, True, None),   # 58 slots over four 16-lane rows, F = 63, E = 64, B % waves != 0; mask, tie-break
    (2, 62, 8, 8, 3, 10, False, False, None),    # all 64 lanes
    (1, 1, 1, 8, 1, 3, False, False, None),      # every width 1
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
def _search_inputs(case):
    """Weights, two sets of observations with the oracle's RootFnOutput for each, mask and noise: once per case."""
    A, Cn, E, support, B, S, tiebreak, masked, max_depth = case
    w, repr_w, repr_b = _family(11, OBS_DIM, A, Cn, E, support)
    rng = np.random.default_rng([7, A, Cn, E, B, S])
    obs = [rng.uniform(0, 1, (B, OBS_DIM)).astype(F32) for _ in range(2)]
    roots = [_root_reference(w, repr_w, repr_b, A, E, support, o) for o in obs]
    invalid = ss.draw_invalid(rng, B, A, all_invalid_root=False) if masked else None
    noise = rng.dirichlet([0.3] * A, B).astype(F32)
    return dict(w=w, repr_w=repr_w, repr_b=repr_b, obs=obs, roots=roots, invalid=invalid, noise=noise)


def _search_handle(case, r, batch=None, **cfg):
    A, Cn, E, support, B, S, tiebreak, _, max_depth = case
    return _handle(A, Cn, E, support, batch or B, S, r["w"], r["repr_w"], r["repr_b"], tiebreak=tiebreak, max_depth=max_depth, **cfg)


def _snapshot(s, out):
    """Host copies of everything a search returns (the handle's buffers are overwritten by the next call)."""
    tree = None if out.search_tree is None else type(out.search_tree)(*[t.clone() for t in out.search_tree])
    return dict(action=out.action.cpu().numpy().copy(), weights=out.action_weights.cpu().numpy().copy(),
                value=s.search_value.cpu().numpy().copy(), depth_sum=s.depth_sum.cpu().numpy().copy(),
                root_value=s.root_value.cpu().numpy().copy(), tree=tree)


def _same(a, b, rows=slice(None)):
    """Two snapshots hold the same bits (`rows`: those of a, when b is a shard); the root value is compared by the caller."""
    for f in ("action", "weights", "value", "depth_sum"):
        assert np.array_equal(np.ascontiguousarray(a[f][rows]).view(np.uint32), np.ascontiguousarray(b[f]).view(np.uint32)), f
    for f in a["tree"]._fields:
        x, y = getattr(a["tree"], f)[rows].contiguous(), getattr(b["tree"], f)
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f


def _kw(r, key=KEY, rows=slice(None), **more):
    return dict(key=list(key), invalid_actions=_tt(None if r["invalid"] is None else r["invalid"][rows]),
                dirichlet_noise=_tt(r["noise"][rows]), with_tree=True, **more)


@pytest.mark.parametrize("case", SEARCH_CASES, ids=_case_id)
def test_search_on_observations_equals_search_on_the_oracle_root(case):
    """The SAME handle, one launch each: on the oracle's RootFnOutput, then on the observations -- eager, and captured:
    the capturing call and a replay with the other observations, which must give the eager result for those."""
    case = _resolve(case)
    r = _search_inputs(case)
    s = _search_handle(case, r)
    ref = [_snapshot(s, s.search_stochastic_mlp(tuple(_tt(x) for x in root), one_launch=True, **_kw(r))) for root in r["roots"]]
    for graph in (False, True):
        for i in ((0, 1) if graph else (0,)):
            got = _snapshot(s, s.search_stochastic_mlp(None, obs=_tt(r["obs"][i]), one_launch=True, graph=graph, **_kw(r)))
            _same(ref[i], got)
            assert np.array_equal(_bits(got["root_value"]), _bits(r["roots"][i][1]))
            # node 0 of the exported tree: the oracle's embedding and value
            assert np.array_equal(_bits(got["tree"].embeddings[:, 0].cpu().numpy()), _bits(r["roots"][i][2]))
            assert np.array_equal(_bits(got["tree"].raw_values[:, 0].cpu().numpy()), _bits(r["roots"][i][1]))
    assert case[2] == 1 or not np.array_equal(r["roots"][0][1], r["roots"][1][1])  # (the two sets of observations differ in effect)
    g = [k for k in s._graphs if isinstance(k, tuple) and "obs" in k]
    assert len(g) == 1
    s.close()


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("case", [SEARCH_CASES[0], SEARCH_CASES[2]], ids=_case_id)
def test_three_launch_route_on_observations(case, graph):
    """The root kernel in front of the three-launch loop == the one launch, on the same handle."""
    r = _search_inputs(case)
    s = _search_handle(case, r)
    for i in ((0, 1) if graph else (0,)):
        one = _snapshot(s, s.search_stochastic_mlp(None, obs=_tt(r["obs"][i]), one_launch=True, **_kw(r)))
        three = _snapshot(s, s.search_stochastic_mlp(None, obs=_tt(r["obs"][i]), graph=graph, **_kw(r)))
        _same(one, three)
        assert np.array_equal(_bits(three["root_value"]), _bits(r["roots"][i][1]))
        assert np.array_equal(_bits(one["root_value"]), _bits(r["roots"][i][1]))
    s.close()


def test_result_does_not_depend_on_the_launch_geometry():
    """Five roots as one batch and as shards of 2 + 3 (global_batch / root_offset): the same bits per root."""
    case = (4, 32, 16, 10, 5, 24, True, True, None)
    r = _search_inputs(case)
    whole = _search_handle(case, r)
    ref = _snapshot(whole, whole.search_stochastic_mlp(None, obs=_tt(r["obs"][0]), one_launch=True, **_kw(r)))
    assert np.array_equal(_bits(ref["root_value"]), _bits(r["roots"][0][1]))
    whole.close()
    for off, n in ((0, 2), (2, 3)):
        rows = slice(off, off + n)
        s = _search_handle(case, r, batch=n, global_batch=5, root_offset=off)
        got = _snapshot(s, s.search_stochastic_mlp(None, obs=_tt(r["obs"][0][rows]), one_launch=True, **_kw(r, rows=rows)))
        _same(ref, got, rows)
        assert np.array_equal(_bits(ref["root_value"][rows]), _bits(got["root_value"]))
        s.close()


def test_guard_words():
    """Through the C ABI with sentinel tails behind root_value_out (and the search's other outputs) and behind the root
    kernel's three outputs: none is written."""
    from muax_amd import _lib
    case = SEARCH_CASES[2]
    A, Cn, E, support, B, S = case[:6]
    r = _search_inputs(case)
    s = _search_handle(case, r)
    ref = _snapshot(s, s.search_stochastic_mlp(tuple(_tt(x) for x in r["roots"][0]), one_launch=True, **_kw(r)))
    obs, invalid, noise = _tt(r["obs"][0]), _tt(r["invalid"]), _tt(r["noise"])

    def guarded(widths):
        return {n: torch.full((B * k + GUARD,), SENTINEL, dtype=torch.int32, device="cuda") for n, k in widths.items()}

    def untouched(outs, widths):
        torch.cuda.synchronize()
        got = {n: t.cpu().numpy().view(np.uint32) for n, t in outs.items()}
        for n, k in widths.items():
            assert (got[n][B * k:] == SENTINEL).all(), f"{n}: guard tail written"
            assert (got[n][:B * k] != SENTINEL).all(), f"{n}: not all written"
        return got

    widths = dict(action=1, action_weights=A, search_value=1, depth_sum=1, root_value=1)
    outs = guarded(widths)
    a = _lib.args(_lib.MzsStochasticSearchArgs, export_tree=0, invalid_actions=invalid.data_ptr(), dirichlet_noise=noise.data_ptr(),
                  key=KEY, dirichlet_fraction=0.25, temperature=1.0,
                  **{n: t.data_ptr() for n, t in outs.items() if n != "root_value"})
    _lib.check(s._L.mzs_mlp_stochastic_search_obs(s._h, C.byref(a), C.c_void_p(obs.data_ptr()),
                                                  C.c_void_p(outs["root_value"].data_ptr()), None), s._h)
    got = untouched(outs, widths)
    assert np.array_equal(got["root_value"][:B], _bits(r["roots"][0][1]))
    assert np.array_equal(got["action"][:B].view(np.int32), ref["action"])
    assert np.array_equal(got["action_weights"][:B * A], _bits(ref["weights"]).ravel())
    assert np.array_equal(got["search_value"][:B], _bits(ref["value"]))

    widths = dict(prior_logits=A, value=1, embedding=E)
    outs = guarded(widths)
    _lib.check(s._L.mzs_mlp_stochastic_root(s._h, C.c_void_p(obs.data_ptr()), *[C.c_void_p(outs[n].data_ptr()) for n in widths],
                                            None), s._h)
    got = untouched(outs, widths)
    for n, x in zip(widths, r["roots"][0]):
        assert np.array_equal(got[n][:B * widths[n]], _bits(x).ravel()), n
    s.close()


# ---------------------------------------------------------------- refusals
def test_refusals_name_the_cause():
    """What the three entries refuse on the host, before any launch: the code, the message, the outputs' sentinel kept."""
    from muax_amd import MuZeroSearch, SearchConfig, _lib
    A, Cn, E, B, od = 3, 2, 4, 2, 5
    INVALID, UNSUPPORTED = -1, -2  # MZS_E_INVALID, MZS_E_UNSUPPORTED
    w, repr_w, repr_b = _family(1, od, A, Cn, E, 8)
    wt = {k: _tt(v) for k, v in w.items()}
    rw, rb = _tt(repr_w), _tt(repr_b)
    z = lambda *sh, dt=torch.float32: torch.zeros(*sh, dtype=dt, device="cuda")  # noqa: E731
    obs = z(B, od)
    outs = {n: torch.full((B * k,), SENTINEL, dtype=torch.int32, device="cuda")
            for n, k in dict(action=1, action_weights=A, root_value=1, prior_logits=A, value=1, embedding=E).items()}
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731

    def args(**over):
        kw = dict(action=outs["action"].data_ptr(), action_weights=outs["action_weights"].data_ptr())
        kw.update(over)
        return _lib.args(_lib.MzsStochasticSearchArgs, **kw)

    def refused(h, rc, code, who, text):
        assert rc == code, (rc, h._L.mzs_last_error(h._h))
        assert h._L.mzs_last_error(h._h).decode() == who + ": " + text

    def search(h, a, code, text, obs_=obs, rv=outs["root_value"]):
        refused(h, h._L.mzs_mlp_stochastic_search_obs(h._h, None if a is None else C.byref(a), p(obs_), p(rv), None), code,
                "mzs_mlp_stochastic_search_obs", text)

    def root(h, code, text, obs_=obs, **over):
        o = dict(prior_logits=outs["prior_logits"], value=outs["value"], embedding=outs["embedding"])
        o.update(over)
        refused(h, h._L.mzs_mlp_stochastic_root(h._h, p(obs_), p(o["prior_logits"]), p(o["value"]), p(o["embedding"]), None), code,
                "mzs_mlp_stochastic_root", text)

    def bind(h, code, text, obs_dim=od, w_=rw, b_=rb):
        refused(h, h._L.mzs_mlp_set_stochastic_representation(h._h, obs_dim, p(w_), p(b_)), code,
                "mzs_mlp_set_stochastic_representation", text)

    other = "this handle does not run the stochastic policy (policy 2)"
    d = MuZeroSearch(B, SearchConfig(A, 3, E))
    bind(d, INVALID, other)
    root(d, INVALID, other)
    search(d, args(), INVALID, other)
    s = MuZeroSearch(B, SearchConfig(A, 3, E, policy="stochastic", num_chance_outcomes=Cn))
    root(s, INVALID, "call mzs_mlp_set_stochastic_weights first")
    search(s, args(), INVALID, "call mzs_mlp_set_stochastic_weights first")
    with pytest.raises(ValueError, match="set_stochastic_mlp_weights"):
        s.search_stochastic_mlp(None, obs=obs, one_launch=True)
    s.set_stochastic_mlp_weights(wt, 8, 0.99)
    root(s, INVALID, "call mzs_mlp_set_stochastic_representation first")
    search(s, args(), INVALID, "call mzs_mlp_set_stochastic_representation first")
    with pytest.raises(ValueError, match="set_stochastic_representation"):
        s.stochastic_mlp_root(obs)
    bind(s, INVALID, "obs_dim must be at least 1", obs_dim=0)
    bind(s, INVALID, "null weight array", w_=None)
    bind(s, INVALID, "null weight array", b_=None)
    root(s, INVALID, "call mzs_mlp_set_stochastic_representation first")  # (a refused binding binds nothing)
    with pytest.raises(ValueError, match="repr_b"):
        s.set_stochastic_representation(rw, z(E + 1))
    s.set_stochastic_representation(rw, rb)
    root(s, INVALID, "null obs", obs_=None)
    for name in ("prior_logits", "value", "embedding"):
        root(s, INVALID, "null output", **{name: None})
    search(s, None, INVALID, "null or size mismatch (ABI)")
    bad = args()
    bad.struct_size -= 8
    search(s, bad, INVALID, "null or size mismatch (ABI)")
    search(s, args(), INVALID, "null obs", obs_=None)
    search(s, args(), INVALID, "null root_value_out", rv=None)
    for name, t in (("prior_logits", z(B, A)), ("value", z(B)), ("embedding", z(B, E))):
        search(s, args(**{name: t.data_ptr()}), INVALID,
               "prior_logits, value and embedding must be NULL (the kernel computes them from obs)")
    for name in ("action", "action_weights"):
        search(s, args(**{name: None}), INVALID, "null output")
    search(s, args(dirichlet_fraction=0.25), INVALID, "dirichlet_fraction != 0 needs dirichlet_noise")
    with pytest.raises(ValueError, match="both|either"):
        s.search_stochastic_mlp((z(B, A), z(B), z(B, E)), obs=obs)
    with pytest.raises(ValueError, match="obs: expected shape"):
        s.search_stochastic_mlp(None, obs=z(B, od + 1), one_launch=True)
    # shapes the plan (or the one-wavefront root) declines: the typed "no kernel for this configuration" code
    w70, rw70, rb70 = _family(1, od, A, Cn, 70, 8)
    wide = MuZeroSearch(B, SearchConfig(A, 3, 70, policy="stochastic", num_chance_outcomes=Cn))
    wide.set_stochastic_mlp_weights({k: _tt(v) for k, v in w70.items()}, 8, 0.99)
    wide.set_stochastic_representation(_tt(rw70), _tt(rb70))
    with pytest.raises(_lib.Unsupported, match=r"embed_dim must be 1\.\.64"):
        wide.search_stochastic_mlp(None, obs=obs, one_launch=True)
    with pytest.raises(_lib.Unsupported, match=r"mzs_mlp_stochastic_root: embed_dim must be 1\.\.64"):
        wide.stochastic_mlp_root(obs)
    long = MuZeroSearch(B, SearchConfig(A, 256, E, policy="stochastic", num_chance_outcomes=Cn))
    long.set_stochastic_mlp_weights(wt, 8, 0.99)
    long.set_stochastic_representation(rw, rb)
    with pytest.raises(ValueError, match=r"num_simulations must be 1\.\.255"):
        long.search_stochastic_mlp(None, obs=obs, one_launch=True)
    a = args()
    rc = long._L.mzs_mlp_stochastic_search_obs(long._h, C.byref(a), p(obs), p(outs["root_value"]), None)
    assert rc == UNSUPPORTED and "num_simulations must be 1..255" in long._L.mzs_last_error(long._h).decode()
    search(wide, args(), UNSUPPORTED, "embed_dim must be 1..64")
    root(wide, UNSUPPORTED, "embed_dim must be 1..64")
    torch.cuda.synchronize()
    for t in outs.values():
        assert (t.cpu().numpy().view(np.uint32) == SENTINEL).all()
    for h in (d, s, wide, long):
        h.close()


# ---------------------------------------------------------------- MuZero(SMZNetwork, stochastic_root_in_kernel=True)
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


def test_model_routes(monkeypatch):
    import muax_amd as mx
    monkeypatch.delenv("MUAX_AMD_STOCHASTIC_MLP", raising=False)
    B, A, Cn, E, od, S = 9, 4, 32, 16, 16, 20
    obs, invalid = _act_inputs(B, A, od)
    kw = dict(with_pi=True, with_value=True, obs_from_batch=True, num_simulations=S, invalid_actions=invalid,
              dirichlet_fraction=0.0, device_outputs=True)
    one = _model(A, Cn, E, stochastic_one_launch=True, stochastic_root_in_kernel=True)
    assert one.stochastic_root_in_kernel and not _model(A, Cn, E).stochastic_root_in_kernel
    a1, w1, v1 = one.act([3, 4], obs, **kw)
    assert one._last_route == "hip_stochastic_one_launch_root"
    # == a search by hand on a handle bound by hand
    s = mx.MuZeroSearch(B, mx.SearchConfig(A, S, E, policy="stochastic", num_chance_outcomes=Cn))
    s.set_stochastic_mlp_weights({k: t.detach() for k, t in mx.nn.stochastic_mlp_weights(one.network).items()}, 10, 0.97)
    s.set_stochastic_representation(*[t.detach() for t in mx.nn.stochastic_root_weights(one.network)])
    out = s.search_stochastic_mlp(None, obs=obs, key=[3, 4], invalid_actions=invalid, dirichlet_fraction=0.0, one_launch=True)
    assert torch.equal(out.action, a1) and torch.equal(out.action_weights.view(torch.int32), w1.view(torch.int32))
    assert torch.equal(s.root_value.view(torch.int32), v1.view(torch.int32))
    assert (w1[invalid.bool()] == 0).all()
    s.close()
    # the three-launch route with the root kernel in front: the same bits
    three = _model(A, Cn, E, stochastic_root_in_kernel=True)
    a3, w3, v3 = three.act([3, 4], obs, **kw)
    assert three._last_route == "hip_stochastic_mlp_root"
    assert torch.equal(a3, a1) and torch.equal(w3.view(torch.int32), w1.view(torch.int32))
    assert torch.equal(v3.view(torch.int32), v1.view(torch.int32))
    # host observations and host results, then Dirichlet noise drawn from the key: served as before
    a_h, w_h, v_h = one.act([3, 4], obs.cpu().numpy(), with_pi=True, with_value=True, obs_from_batch=True, num_simulations=S,
                            invalid_actions=invalid, dirichlet_fraction=0.0)
    assert one._last_route == "hip_stochastic_one_launch_root" and isinstance(a_h, np.ndarray)
    assert np.array_equal(a_h, a1.cpu().numpy()) and np.array_equal(_bits(w_h), _bits(w1.cpu().numpy()))
    assert np.array_equal(_bits(v_h), _bits(v1.cpu().numpy()))
    one.act([3, 4], obs, obs_from_batch=True, num_simulations=S, invalid_actions=invalid, device_outputs=True)
    assert one._last_route == "hip_stochastic_one_launch_root"
    # an embedding wider than a wavefront keeps the torch root and the route's present name
    big = _model(A, Cn, 70, stochastic_root_in_kernel=True)
    big.act([3, 4], obs[:3], obs_from_batch=True, num_simulations=6, invalid_actions=invalid[:3], dirichlet_fraction=0.0,
            device_outputs=True)
    assert big._last_route == "hip_stochastic_mlp"
    # the library route switched off: the torch root and the callables, as a flag-off model
    monkeypatch.setenv("MUAX_AMD_STOCHASTIC_MLP", "0")
    off = _model(A, Cn, E)
    small = dict(kw, num_simulations=4, invalid_actions=invalid[:3])
    ac, wc, vc = one.act([3, 4], obs[:3], **small)
    assert one._last_route == "callables"
    ao, wo, vo = off.act([3, 4], obs[:3], **small)
    assert off._last_route == "callables"
    assert torch.equal(ac, ao) and torch.equal(wc.view(torch.int32), wo.view(torch.int32))
    assert torch.equal(vc.view(torch.int32), vo.view(torch.int32))


# ---------------------------------------------------------------- against the torch root
def test_root_against_the_modules_in_float64(capsys):
    """The only non-exact check.  The kernel's root (another summation order than torch's GEMMs, its own exp / log) and
    torch fp32's, each against the same modules evaluated in float64: per output, the kernel's largest distance may be
    at most 4x torch fp32's own.  The figures are printed; profiles/stochastic_search.txt records a run."""
    import muax_amd as mx
    from muax_amd import utils as mx_utils
    B, A, Cn, E, od = 64, 4, 32, 16, 16
    m = _model(A, Cn, E, stochastic_root_in_kernel=True)
    obs, _ = _act_inputs(B, A, od, seed=9)
    s = mx.MuZeroSearch(B, mx.SearchConfig(A, 2, E, policy="stochastic", num_chance_outcomes=Cn))
    s.set_stochastic_mlp_weights({k: t.detach() for k, t in mx.nn.stochastic_mlp_weights(m.network).items()}, 10, 0.97)
    s.set_stochastic_representation(*[t.detach() for t in mx.nn.stochastic_root_weights(m.network)])
    kernel = [t.double() for t in s.stochastic_mlp_root(obs)]
    fp32 = [t.double() for t in m._root_inference_eager(obs)]
    with torch.no_grad():
        rep, pred = copy.deepcopy(m.repr_func).double(), copy.deepcopy(m.pred_func).double()
        st = rep(obs.double())
        v, logits = pred(st)
        exact = [logits, mx_utils.support_to_scalar(torch.softmax(v, dim=-1), 10).flatten(), st]
    assert all(t.dtype == torch.float64 for t in exact)
    report = []
    for name, k, t, e in zip(("logits", "value", "embedding"), kernel, fp32, exact):
        dk, dt = float((k - e).abs().max()), float((t - e).abs().max())
        report.append((name, dk, dt))
    with capsys.disabled():
        for name, dk, dt in report:
            print(f"\nroot {name}: |kernel - fp64| = {dk:.3e}, |torch fp32 - fp64| = {dt:.3e}", end="")
        print()
    for name, dk, dt in report:
        assert dk <= 4 * dt, (name, dk, dt)
    s.close()
