"""The root's Dirichlet noise drawn inside the one-launch stochastic search (the DRAW instantiations of mz_stoch_wide_kernel
through mzs_mlp_stochastic_search_draw, mz_dirichlet.cuh wave_dirichlet_row): the drawn rows against the oracle's
restatement and against mzs_dirichlet, the search against the existing route handed that array, shards, captured
launches replayed with a new key, guard words, MuZero(stochastic_noise_in_kernel=True) and the entry's refusals.  Every
comparison is == on the bits."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import scripted_search as ss
import stochastic_mlp_reference as smr

pytestmark = pytest.mark.gpu
F32 = np.float32
SENTINEL = 0x5A5AA5A5  # the bit pattern untouched output words must keep
GUARD = 37             # guard words behind every output array
KEYS = ((4, 5), (0xFFFFFFFF, 7))
OBS_DIM = 7
S = 6


def _tt(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def _k_dir(key):
    from muax_amd import prng
    return tuple(int(w) for w in prng.split(key, 3)[1])  # mctx: rng_key, dirichlet_rng_key, search_rng_key = split(key, 3)


def _separate(key, alpha, B, A, global_batch=None, root_offset=0):
    """The noise as act() draws it today: mzs_dirichlet's launch on the Dirichlet sub-key."""
    from muax_amd.model import _dirichlet
    return _dirichlet(_k_dir(key), alpha, (B, A), "cuda", global_batch, root_offset)


@functools.lru_cache(maxsize=None)
def _inputs(A, Cn, E, support, B, masked):
    """Weights of the family and its representation, a RootFnOutput, observations and a mask: once per shape."""
    rng = np.random.default_rng([13, A, Cn, E, B])
    repr_w = (np.clip(rng.standard_normal((OBS_DIM, E)), -2, 2) / np.sqrt(OBS_DIM)).astype(F32)
    return dict(w=smr.random_weights(11, A, Cn, E, support), repr_w=repr_w, repr_b=(0.1 * rng.standard_normal(E)).astype(F32),
                root=(rng.standard_normal((B, A)).astype(F32), rng.uniform(-3, 3, B).astype(F32),
                      rng.uniform(0, 1, (B, E)).astype(F32)),
                obs=rng.uniform(0, 1, (B, OBS_DIM)).astype(F32),
                invalid=ss.draw_invalid(rng, B, A, all_invalid_root=False) if masked else None)


def _handle(A, Cn, E, support, B, r, **cfg):
    from muax_amd import MuZeroSearch, SearchConfig
    s = MuZeroSearch(B, SearchConfig(A, S, E, policy="stochastic", num_chance_outcomes=Cn, **cfg))
    s.set_stochastic_mlp_weights({k: _tt(v) for k, v in r["w"].items()}, support, 0.97)
    s.set_stochastic_representation(_tt(r["repr_w"]), _tt(r["repr_b"]))
    return s


def _root_kw(r, with_obs, rows=slice(None)):
    """search_stochastic_mlp's root arguments: the observations or the RootFnOutput, and the mask."""
    kw = dict(invalid_actions=_tt(None if r["invalid"] is None else r["invalid"][rows]), one_launch=True, with_tree=True)
    if with_obs:
        return dict(kw, root_fn_output=None, obs=_tt(r["obs"][rows]))
    return dict(kw, root_fn_output=tuple(_tt(x[rows]) for x in r["root"]))


def _snapshot(s, out):
    """Host copies of everything a search returns (the handle's buffers are overwritten by the next call)."""
    return dict(action=out.action.cpu().numpy().copy(), weights=out.action_weights.cpu().numpy().copy(),
                value=s.search_value.cpu().numpy().copy(), depth_sum=s.depth_sum.cpu().numpy().copy(),
                root_value=s.root_value.cpu().numpy().copy(), tree=type(out.search_tree)(*[t.clone() for t in out.search_tree]),
                noise=None if s.root_noise is None else s.root_noise.cpu().numpy().copy())


def _same(a, b, rows=slice(None), with_obs=False):
    """Two snapshots hold the same bits (`rows`: those of a, when b is a shard)."""
    for f in ("action", "weights", "value", "depth_sum") + (("root_value",) if with_obs else ()):
        assert np.array_equal(np.ascontiguousarray(a[f][rows]).view(np.uint32), np.ascontiguousarray(b[f]).view(np.uint32)), f
    for f in a["tree"]._fields:
        x, y = getattr(a["tree"], f)[rows].contiguous(), getattr(b["tree"], f)
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f


# ---------------------------------------------------------------- the noise itself
# (A, C): one element (the row is [1.0]); three; 2048's; one full pass of sixteen; a second pass holding one element; three
# passes with every lane a slot; 63 actions, the last pass one group short
NOISE_SHAPES = [(1, 1), (3, 2), (4, 32), (16, 5), (17, 5), (33, 31), (63, 1)]
ALPHAS = [0.03, 0.3, 1.0, 2.5]  # (1.0: the boundary of the boost)


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("A,Cn", NOISE_SHAPES, ids=lambda v: str(v))
def test_drawn_rows_are_the_oracles_and_mzs_dirichlets(A, Cn, alpha):
    """Five roots -- no multiple of the 2, 3 or 4 wavefronts of a workgroup, the tail wavefronts exit --, as the whole
    batch and as rows 4..8 of a global batch of 11."""
    from muax_amd import search
    from oracle import pyoracle as oracle
    oracle.build()
    B, E, support, key = 5, 5, 8, KEYS[0]
    pl = search.stochastic_plan(A, Cn, E, support, S)
    assert pl is not None and B % pl["waves"] != 0
    r = _inputs(A, Cn, E, support, B, False)
    for gb, off in ((None, 0), (11, 4)):
        s = _handle(A, Cn, E, support, B, r, **({} if gb is None else dict(global_batch=gb, root_offset=off)))
        got = _snapshot(s, s.search_stochastic_mlp(key=list(key), draw_dirichlet=alpha, noise_out=True, **_root_kw(r, False)))
        ref = oracle.dirichlet(_k_dir(key), alpha, B, A, gb, off)
        assert got["noise"].shape == (B, A) and np.array_equal(_bits(got["noise"]), _bits(ref))
        sep = _separate(key, alpha, B, A, gb, off)
        assert np.array_equal(_bits(got["noise"]), _bits(sep.cpu().numpy()))
        if A == 1:
            assert (got["noise"] == 1.0).all()
        # ... and the search is the one the existing route runs on that array
        _same(_snapshot(s, s.search_stochastic_mlp(key=list(key), dirichlet_noise=sep, **_root_kw(r, False))), got)
        s.close()


def test_drawn_rows_where_the_speculative_lanes_are_exhausted():
    """16384 roots x 63 actions, one simulation: of a million elements some (~6e-6 each) see all four speculative
    candidates rejected and their group walks the serial loop on -- beside groups that do not, and in the last pass beside
    the shadow group.  The rows are mzs_dirichlet's."""
    A, Cn, E, support, B, alpha, key = 63, 1, 1, 8, 16384, 0.3, KEYS[1]
    from muax_amd import MuZeroSearch, SearchConfig
    r = _inputs(A, Cn, E, support, 1, False)
    s = MuZeroSearch(B, SearchConfig(A, 1, E, policy="stochastic", num_chance_outcomes=Cn))
    s.set_stochastic_mlp_weights({k: _tt(v) for k, v in r["w"].items()}, support, 0.97)
    root = (torch.zeros(B, A, device="cuda"), torch.zeros(B, device="cuda"), torch.zeros(B, E, device="cuda"))
    s.search_stochastic_mlp(root, key=list(key), draw_dirichlet=alpha, noise_out=True, one_launch=True)
    assert torch.equal(s.root_noise.view(torch.int32), _separate(key, alpha, B, A).view(torch.int32))
    s.close()


# ---------------------------------------------------------------- the search
SHAPE =(4, 32, 16, 10, 7)  # 2048's (A, C, E, support) at seven roots: two workgroups, the second one short


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("masked", [False, True], ids=["free", "masked"])
@pytest.mark.parametrize("tiebreak", [False, True], ids=["first", "tiebreak"])
@pytest.mark.parametrize("with_obs", [False, True], ids=["rootfn", "obs"])
def test_search_equals_the_route_given_the_separately_drawn_array(with_obs, tiebreak, masked, graph):
    """Field for field, trees included.  graph=True: the capturing call with one key, a replay with another -- each must
    be the eager result of the existing route for that key; the captured launch stages no noise."""
    A, Cn, E, support, B = SHAPE
    alpha = 0.3
    r = _inputs(A, Cn, E, support, B, masked)
    s = _handle(A, Cn, E, support, B, r, tiebreak=tiebreak)
    kw = _root_kw(r, with_obs)
    ref = [_snapshot(s, s.search_stochastic_mlp(key=list(k), dirichlet_noise=_separate(k, alpha, B, A), **kw)) for k in KEYS]
    assert not np.array_equal(ref[0]["weights"], ref[1]["weights"])  # (the two keys differ in effect)
    for i, k in enumerate(KEYS if graph else KEYS[:1]):
        got = _snapshot(s, s.search_stochastic_mlp(key=list(k), draw_dirichlet=alpha, noise_out=True, graph=graph, **kw))
        _same(ref[i], got, with_obs=with_obs)
        assert np.array_equal(_bits(got["noise"]), _bits(_separate(k, alpha, B, A).cpu().numpy()))
    if graph:
        drawn = [g for g in s._graphs if isinstance(g, tuple) and "draw" in g]
        assert len(drawn) == 1 and len(s._graphs) == 1
        bufs, host, block = s._graphs[drawn[0]][1][:3]
        assert bufs["dirichlet_noise"] is None and block.numel() == 7 + 2 * S
        # the same variant without the rows: another graph, the same search
        got = _snapshot(s, s.search_stochastic_mlp(key=list(KEYS[1]), draw_dirichlet=alpha, graph=True, **kw))
        assert got["noise"] is None and len(s._graphs) == 2
        _same(ref[1], got, with_obs=with_obs)
    s.close()


def test_shards_draw_their_own_rows():
    """Five roots as one batch and as shards of 2 + 3 (global_batch / root_offset): the same noise, the same results."""
    A, Cn, E, support = SHAPE[:4]
    alpha, key = 0.3, KEYS[0]
    r = _inputs(A, Cn, E, support, 5, True)
    whole = _handle(A, Cn, E, support, 5, r, tiebreak=True)
    ref = _snapshot(whole, whole.search_stochastic_mlp(key=list(key), draw_dirichlet=alpha, noise_out=True, **_root_kw(r, True)))
    whole.close()
    for off, n in ((0, 2), (2, 3)):
        rows = slice(off, off + n)
        s = _handle(A, Cn, E, support, n, r, tiebreak=True, global_batch=5, root_offset=off)
        got = _snapshot(s, s.search_stochastic_mlp(key=list(key), draw_dirichlet=alpha, noise_out=True, **_root_kw(r, True, rows)))
        _same(ref, got, rows, with_obs=True)
        assert np.array_equal(_bits(ref["noise"][rows]), _bits(got["noise"]))
        s.close()


# ---------------------------------------------------------------- guard words
def test_guard_words_and_no_rows_unless_asked():
    """Through the C ABI with sentinel tails behind noise_out and the other outputs: none is written, every word in front
    is.  Without noise_out nothing is written anywhere else: the caller's tensor and the handle's buffer keep their words."""
    from muax_amd import _lib
    A, Cn, E, support, B = 17, 5, 5, 8, 5  # (two passes, the second holding one element)
    alpha, key = 0.3, KEYS[0]
    r = _inputs(A, Cn, E, support, B, True)
    s = _handle(A, Cn, E, support, B, r)
    ref = _snapshot(s, s.search_stochastic_mlp(key=list(key), dirichlet_noise=_separate(key, alpha, B, A), **_root_kw(r, True)))
    obs, invalid = _tt(r["obs"]), _tt(r["invalid"])
    widths = dict(action=1, action_weights=A, search_value=1, depth_sum=1, root_value=1, noise=A)
    outs = {n: torch.full((B * k + GUARD,), SENTINEL, dtype=torch.int32, device="cuda") for n, k in widths.items()}
    a = _lib.args(_lib.MzsStochasticSearchArgs, export_tree=0, invalid_actions=invalid.data_ptr(), key=key,
                  dirichlet_fraction=0.25, temperature=1.0,
                  **{n: t.data_ptr() for n, t in outs.items() if n not in ("root_value", "noise")})
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    _lib.check(s._L.mzs_mlp_stochastic_search_draw(s._h, C.byref(a), p(obs), p(outs["root_value"]), alpha, p(outs["noise"]), None),
               s._h)
    torch.cuda.synchronize()
    got = {n: t.cpu().numpy().view(np.uint32) for n, t in outs.items()}
    for n, k in widths.items():
        assert (got[n][B * k:] == SENTINEL).all(), f"{n}: guard tail written"
        assert (got[n][:B * k] != SENTINEL).all(), f"{n}: not all written"
    assert np.array_equal(got["noise"][:B * A], _bits(_separate(key, alpha, B, A).cpu().numpy()).ravel())
    assert np.array_equal(got["action"][:B].view(np.int32), ref["action"])
    assert np.array_equal(got["action_weights"][:B * A], _bits(ref["weights"]).ravel())
    assert np.array_equal(got["search_value"][:B], _bits(ref["value"]))
    assert np.array_equal(got["root_value"][:B], _bits(ref["root_value"]))
    # the caller's tensor receives the rows; without noise_out the handle's buffer of an earlier call is not written again
    mine = torch.zeros(B, A, device="cuda")
    s.search_stochastic_mlp(key=list(key), draw_dirichlet=alpha, noise_out=mine, **_root_kw(r, True))
    assert s.root_noise is mine and np.array_equal(_bits(mine.cpu().numpy()).ravel(), got["noise"][:B * A])
    s.search_stochastic_mlp(key=list(key), draw_dirichlet=alpha, noise_out=True, **_root_kw(r, True))
    own = s.root_noise
    assert own is not mine and np.array_equal(_bits(own.cpu().numpy()).ravel(), got["noise"][:B * A])
    own.view(torch.int32).fill_(SENTINEL)
    mine.view(torch.int32).fill_(SENTINEL)
    out = _snapshot(s, s.search_stochastic_mlp(key=list(key), draw_dirichlet=alpha, **_root_kw(r, True)))
    assert s.root_noise is None and out["noise"] is None
    _same(ref, out, with_obs=True)
    for t in (own, mine):
        assert (t.cpu().numpy().view(np.uint32) == SENTINEL).all()
    with pytest.raises(ValueError, match="noise_out: expected True or a contiguous float32 tensor"):
        s.search_stochastic_mlp(key=list(key), draw_dirichlet=alpha, noise_out=torch.zeros(B, A + 1, device="cuda"),
                                **_root_kw(r, True))
    s.close()


# ---------------------------------------------------------------- MuZero(SMZNetwork, stochastic_noise_in_kernel=True)
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


def _equal(got, ref):
    for g, x in zip(got, ref):
        assert g.dtype == x.dtype and torch.equal(g.view(torch.int32), x.view(torch.int32))


@pytest.mark.parametrize("root_in_kernel", [True, False], ids=["root", "torch_root"])
def test_model_flag(monkeypatch, root_in_kernel):
    monkeypatch.delenv("MUAX_AMD_STOCHASTIC_MLP", raising=False)
    B, A, od = 9, 4, 16
    rng = np.random.default_rng(2)
    obs = torch.from_numpy(rng.uniform(0, 1, (B, od)).astype(F32)).cuda()
    invalid = torch.from_numpy(ss.draw_invalid(rng, B, A, all_invalid_root=False)).cuda()
    kw = dict(with_pi=True, with_value=True, obs_from_batch=True, num_simulations=S, invalid_actions=invalid, device_outputs=True)
    flags = dict(stochastic_one_launch=True, stochastic_root_in_kernel=root_in_kernel)
    on, off = _model(stochastic_noise_in_kernel=True, **flags), _model(**flags)
    assert on.stochastic_noise_in_kernel and not off.stochastic_noise_in_kernel
    name = "hip_stochastic_one_launch" + ("_root" if root_in_kernel else "")
    results = []
    for key in ([3, 4], [5, 6], 7):
        got = [t.clone() for t in on.act(key, obs, **kw)]
        assert on._last_route == name + "_noise"
        ref = off.act(key, obs, **kw)
        assert off._last_route == name
        _equal(got, ref)
        results.append(got[1])
    assert not torch.equal(results[0], results[1])  # (the noise, and with it the search, follows the key)
    # another alpha is handed down
    got = [t.clone() for t in on.act([3, 4], obs, dirichlet_alpha=1.5, **kw)]
    _equal(got, off.act([3, 4], obs, dirichlet_alpha=1.5, **kw))
    assert not torch.equal(got[1], results[0])
    # a shard draws its rows of the global batch
    part = on.act([3, 4], obs[2:5], global_batch=B, root_offset=2, **dict(kw, invalid_actions=invalid[2:5]))
    assert on._last_route == name + "_noise"
    for g, x in zip(part, on.act([3, 4], obs, **kw)):
        assert torch.equal(g.view(torch.int32), x[2:5].view(torch.int32))
    # an array from the caller, or no noise at all: the routes and results of a model without the flag
    noise = torch.from_numpy(rng.dirichlet([0.3] * A, B).astype(F32)).cuda()
    for more in (dict(dirichlet_noise=noise), dict(dirichlet_fraction=0.0)):
        got = [t.clone() for t in on.act([3, 4], obs, **kw, **more)]
        assert on._last_route == name
        _equal(got, off.act([3, 4], obs, **kw, **more))
    # the three-launch route draws as before
    three = _model(stochastic_noise_in_kernel=True, stochastic_root_in_kernel=root_in_kernel)
    got = [t.clone() for t in three.act([3, 4], obs, **kw)]
    assert three._last_route == "hip_stochastic_mlp" + ("_root" if root_in_kernel else "")
    _equal(got, off.act([3, 4], obs, **kw))


# ---------------------------------------------------------------- refusals
def test_refusals_name_the_cause():
    """What mzs_mlp_stochastic_search_draw refuses on the host, before any launch: the code, the message, the outputs'
    sentinel kept."""
    from muax_amd import MuZeroSearch, SearchConfig, _lib
    A, Cn, E, B, support = 3, 2, 4, 2, 8
    INVALID, UNSUPPORTED = -1, -2  # MZS_E_INVALID, MZS_E_UNSUPPORTED
    r = _inputs(A, Cn, E, support, B, False)
    z = lambda *sh: torch.zeros(*sh, dtype=torch.float32, device="cuda")  # noqa: E731
    obs = _tt(r["obs"])
    outs = {n: torch.full((B * k,), SENTINEL, dtype=torch.int32, device="cuda")
            for n, k in dict(action=1, action_weights=A, root_value=1, noise=A).items()}
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731

    def args(**over):
        kw = dict(action=outs["action"].data_ptr(), action_weights=outs["action_weights"].data_ptr(), key=KEYS[0],
                  dirichlet_fraction=0.25, temperature=1.0)
        kw.update(over)
        return _lib.args(_lib.MzsStochasticSearchArgs, **kw)

    def draw(h, a, code, text, obs_=obs, rv=outs["root_value"], alpha=0.3):
        rc = h._L.mzs_mlp_stochastic_search_draw(h._h, None if a is None else C.byref(a), p(obs_), p(rv), alpha, p(outs["noise"]),
                                                 None)
        assert rc == code, (rc, h._L.mzs_last_error(h._h))
        assert h._L.mzs_last_error(h._h).decode() == "mzs_mlp_stochastic_search_draw: " + text

    d = MuZeroSearch(B, SearchConfig(A, 3, E))
    draw(d, args(), INVALID, "this handle does not run the stochastic policy (policy 2)")
    s = MuZeroSearch(B, SearchConfig(A, 3, E, policy="stochastic", num_chance_outcomes=Cn))
    draw(s, args(), INVALID, "call mzs_mlp_set_stochastic_weights first")
    s.set_stochastic_mlp_weights({k: _tt(v) for k, v in r["w"].items()}, support, 0.99)
    draw(s, args(), INVALID, "call mzs_mlp_set_stochastic_representation first")
    root = dict(prior_logits=z(B, A), value=z(B), embedding=z(B, E))
    rootp = {n: t.data_ptr() for n, t in root.items()}
    for name in root:  # obs == NULL: the RootFnOutput arrays, as mzs_mlp_stochastic_search asks for them
        draw(s, args(**dict(rootp, **{name: None})), INVALID, "null input", obs_=None)
    s.set_stochastic_representation(_tt(r["repr_w"]), _tt(r["repr_b"]))
    draw(s, None, INVALID, "null or size mismatch (ABI)")
    bad = args()
    bad.struct_size -= 8
    draw(s, bad, INVALID, "null or size mismatch (ABI)")
    draw(s, args(), INVALID, "null root_value_out", rv=None)
    draw(s, args(prior_logits=rootp["prior_logits"]), INVALID,
         "prior_logits, value and embedding must be NULL (the kernel computes them from obs)")
    draw(s, args(action=None), INVALID, "null output")
    noise = z(B, A)
    for obs_, more in ((obs, {}), (None, rootp)):
        draw(s, args(dirichlet_noise=noise.data_ptr(), **more), INVALID, "dirichlet_noise must be NULL (the kernel draws the noise)",
             obs_=obs_)
        for alpha in (0.0, -0.3, float("inf"), float("nan")):
            draw(s, args(**more), INVALID, "dirichlet_alpha must be positive and finite", obs_=obs_, alpha=alpha)
    # a shape the plan declines: the typed "no kernel for this configuration" code, from the C entry and from Python
    long = MuZeroSearch(B, SearchConfig(A, 256, E, policy="stochastic", num_chance_outcomes=Cn))
    long.set_stochastic_mlp_weights({k: _tt(v) for k, v in r["w"].items()}, support, 0.99)
    long.set_stochastic_representation(_tt(r["repr_w"]), _tt(r["repr_b"]))
    draw(long, args(), UNSUPPORTED, "num_simulations must be 1..255")
    with pytest.raises(_lib.Unsupported, match=r"num_simulations must be 1\.\.255"):
        long.search_stochastic_mlp(None, obs=obs, one_launch=True, draw_dirichlet=0.3)
    torch.cuda.synchronize()
    for t in outs.values():
        assert (t.cpu().numpy().view(np.uint32) == SENTINEL).all()
    for h in (d, s, long):
        h.close()
