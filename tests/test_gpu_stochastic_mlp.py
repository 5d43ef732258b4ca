"""The default stochastic MLP family on the GPU: the one-launch recurrent step (mz_stoch_mlp.cuh through
mzs_mlp_stochastic_recurrent) against the oracle-composed functions of tests/stochastic_mlp_reference.py, bit for bit --
alone, inside the hand-written select -> recurrent -> expand loop, and through MuZeroSearch.search_stochastic_mlp eager
and captured -- then MuZero(SMZNetwork, policy="stochastic").act() on both routes and one update() step."""
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

# (A, C, E, support, B): A != C, odd E, F = 17, the smallest; 2048's shape; A + C = 58 and F = 63, every list over
# several 16-lane slots; E beyond one wavefront's lanes; all ones
KERNEL_SHAPES = [(4, 3, 5, 8, 3), (4, 32, 16, 10, 7), (18, 40, 64, 31, 5), (2, 2, 70, 10, 2), (1, 1, 1, 8, 1)]


def _handle(B, A, Cn, E, S, support, w, **cfg):
    from muax_amd import MuZeroSearch, SearchConfig
    s = MuZeroSearch(B, SearchConfig(A, S, E, policy="stochastic", num_chance_outcomes=Cn, **cfg))
    s.set_stochastic_mlp_weights({k: torch.from_numpy(v).cuda() for k, v in w.items()}, support, 0.97)
    return s


def _bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


@pytest.mark.parametrize("A,Cn,E,support,B", KERNEL_SHAPES)
def test_recurrent_kernel_matches_reference_bits(oracle, A, Cn, E, support, B):
    """mzs_mlp_stochastic_recurrent through the C ABI on hand-made slot / kind / embedding arrays that mix both kinds in
    one launch, twice with the kinds swapped (so every row is evaluated as either kind).  Row 0 is a clamp case in both
    launches: a decision parent with slot A + C - 1 >= A, a chance parent with slot 0 < A.  Rows of the parent's kind ==
    the reference on the uint32 views; rows of the other kind and every guard tail keep the sentinel."""
    from muax_amd import _lib
    w = smr.random_weights(3, A, Cn, E, support)
    ref = smr.StochasticMlpReference(oracle, w, A, Cn, E, support, 0.97)
    s = _handle(B, A, Cn, E, 2, support, w)
    rng = np.random.default_rng([A, Cn, E, B])
    emb = rng.uniform(0, 1, (B, E)).astype(F32)
    widths = dict(chance_logits=Cn, afterstate_value=1, afterstate_embedding=E, action_logits=A, value=1, reward=1, discount=1,
                  state_embedding=E)
    for swap in (0, 1):
        kind = ((np.arange(B) + swap) % 2).astype(np.int32)
        slot = rng.integers(0, A + Cn, B).astype(np.int32)
        slot[0] = A + Cn - 1 if kind[0] else 0
        assert (slot[0] >= A) if kind[0] else (slot[0] < A)
        out = {n: torch.full((B * k + GUARD,), SENTINEL, dtype=torch.int32, device="cuda") for n, k in widths.items()}
        o = _lib.args(_lib.MzsStochasticOutputs, **{n: t.data_ptr() for n, t in out.items()})
        t_slot, t_kind, t_emb = (torch.from_numpy(x).cuda() for x in (slot, kind, emb))
        _lib.check(_lib.load().mzs_mlp_stochastic_recurrent(s._h, t_slot.data_ptr(), t_kind.data_ptr(), t_emb.data_ptr(),
                                                            C.byref(o), None), s._h)
        torch.cuda.synchronize()
        cl, av, ae = ref.decision(np.clip(slot, 0, A - 1), emb)
        al, v, r, d, se = ref.chance(np.clip(slot - A, 0, Cn - 1), emb)
        want = dict(chance_logits=(cl, 1), afterstate_value=(av, 1), afterstate_embedding=(ae, 1), action_logits=(al, 0),
                    value=(v, 0), reward=(r, 0), discount=(d, 0), state_embedding=(se, 0))
        for n, (x, of_kind) in want.items():
            got = out[n].cpu().numpy().view(np.uint32)
            assert (got[B * widths[n]:] == SENTINEL).all(), f"{n}: guard tail written"
            got = got[:B * widths[n]].reshape(B, widths[n])
            exp = np.where((kind == of_kind)[:, None], _bits(x).reshape(B, widths[n]), np.uint32(SENTINEL))
            bad = np.argwhere(got != exp)
            assert bad.size == 0, f"{n} (kinds swapped: {swap}): first mismatch at {bad[0]}: {got[tuple(bad[0])]:#x} != " \
                                  f"{exp[tuple(bad[0])]:#x}"
    s.close()


# ---------------------------------------------------------------- whole search
# (A, C, E, support, B, S, tiebreak, invalid mask)
SEARCH_CASES = [(4, 3, 5, 8, 4, 12, False, False), (4, 3, 5, 8, 4, 12, True, True), (4, 32, 16, 10, 7, 36, False, False),
                (4, 32, 16, 10, 7, 36, True, False)]
KEY = (4, 5)


@functools.lru_cache(maxsize=None)
def _search_reference(case):
    """The stepper fed the helper's functions, once per case: everything the tests compare against."""
    from oracle import pyoracle as oracle
    oracle.build()
    A, Cn, E, support, B, S, tiebreak, masked = case
    w = smr.random_weights(11, A, Cn, E, support)
    ref = smr.StochasticMlpReference(oracle, w, A, Cn, E, support, 0.97)
    rng = np.random.default_rng([7, A, Cn, E, B, S])
    root = (rng.standard_normal((B, A)).astype(F32), rng.uniform(-3, 3, B).astype(F32), rng.uniform(0, 1, (B, E)).astype(F32))
    invalid = ss.draw_invalid(rng, B, A, all_invalid_root=False) if masked else None
    noise = rng.dirichlet([0.3] * A, B).astype(F32)
    stp = st.StochasticStepper(oracle, B, A, Cn, E, S, *root, tiebreak=tiebreak, key=KEY, invalid=invalid, noise=noise)
    slots, kinds, pembs = [], [], []
    for sim in range(S):
        parent, slot, kind = stp.select(sim)
        pemb = stp.parent_embedding(parent).copy()
        slots.append(slot.copy()), kinds.append(kind.copy()), pembs.append(pemb)
        stp.expand_backup(sim, parent, slot, ref.row(slot, pemb))
    action, weights, value = stp.finish()
    return dict(w=w, root=root, invalid=invalid, noise=noise, slots=slots, kinds=kinds, pembs=pembs, action=action,
                weights=weights, value=value, depth_sum=stp.depth_sum.copy(), tree=stp.tree)


def _search_handle(case, r):
    A, Cn, E, support, B, S, tiebreak, _ = case
    return _handle(B, A, Cn, E, S, support, r["w"], tiebreak=tiebreak)


def _root_args(r):
    tt = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    return tuple(tt(x) for x in r["root"]), tt(r["invalid"]), tt(r["noise"])


def _check_finish(s, out, r):
    from helpers import assert_trees_equal
    assert np.array_equal(r["action"], out.action.cpu().numpy())
    assert np.array_equal(_bits(r["weights"]), _bits(out.action_weights.cpu().numpy()))
    assert np.array_equal(_bits(r["value"]), _bits(s.search_value.cpu().numpy()))
    assert np.array_equal(r["depth_sum"], s.depth_sum.cpu().numpy().astype(np.int64))
    assert_trees_equal(r["tree"], out.search_tree, exact_floats=True)


@pytest.mark.parametrize("case", SEARCH_CASES, ids=lambda c: "-".join(str(int(x)) for x in c))
def test_hand_written_loop_matches_stepper(case):
    """mzs_select_stochastic -> mzs_mlp_stochastic_recurrent -> mzs_expand_backup_stochastic, compared per simulation
    (slot, kind, parent embedding) and at the end (action, weights, search value, depth_sum, exported tree): ==."""
    r = _search_reference(case)
    s = _search_handle(case, r)
    root, invalid, noise = _root_args(r)
    s.root_stochastic(*root, list(KEY), invalid, noise, 0.25)
    for sim in range(case[5]):
        slot, kind, pemb = s.select_stochastic(sim)
        assert np.array_equal(r["slots"][sim], slot.cpu().numpy()), f"slot, simulation {sim}"
        assert np.array_equal(r["kinds"][sim], kind.cpu().numpy()), f"parent kind, simulation {sim}"
        assert np.array_equal(_bits(r["pembs"][sim]), _bits(pemb.cpu().numpy())), f"parent embedding, simulation {sim}"
        s.expand_backup_stochastic_outputs(sim, s.stochastic_mlp_recurrent(slot, kind, pemb))
    _check_finish(s, s.finish_stochastic(1.0, None, with_tree=True), r)
    s.close()


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("case", SEARCH_CASES, ids=lambda c: "-".join(str(int(x)) for x in c))
def test_search_stochastic_mlp_eager_and_graph(case, graph):
    """search_stochastic_mlp gives the hand-written loop's bits, eager and as a captured graph (the graph: the capturing
    call and a replay)."""
    r = _search_reference(case)
    s = _search_handle(case, r)
    root, invalid, noise = _root_args(r)
    for _ in range(2 if graph else 1):
        out = s.search_stochastic_mlp(root, key=list(KEY), invalid_actions=invalid, dirichlet_noise=noise, with_tree=True,
                                      graph=graph)
        _check_finish(s, out, r)
    s.close()


# ---------------------------------------------------------------- MuZero(SMZNetwork)
def _model(A=4, Cn=32, E=16, support=10, obs_dim=16, seed=0):
    import muax_amd as mx
    g = torch.Generator().manual_seed(seed)
    net = mx.create_stochastic_muzero_network(E, A, Cn, 2 * support + 1, generator=g)
    m = mx.MuZero(net, policy="stochastic", support_size=support, discount=0.97,
                  optimizer=mx.optimizers.create_optimizer("adam", 1e-2))
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


def _check_structure(weights, invalid):
    assert (weights[invalid.bool()] == 0).all()
    assert torch.allclose(weights.sum(1), torch.ones_like(weights[:, 0]), atol=1e-6)


def test_model_act_takes_the_hip_route_and_equals_the_search_by_hand(monkeypatch):
    import muax_amd as mx
    from muax_amd import MuZeroSearch, SearchConfig
    monkeypatch.delenv("MUAX_AMD_STOCHASTIC_MLP", raising=False)
    B, A, Cn, E, S = 9, 4, 32, 16, 20
    m = _model(A, Cn, E)
    obs, invalid = _act_inputs(B, A, 16)
    a, w, v = m.act([3, 4], obs, with_pi=True, with_value=True, obs_from_batch=True, num_simulations=S,
                    invalid_actions=invalid, dirichlet_fraction=0.0, device_outputs=True)
    assert m._last_route == "hip_stochastic_mlp"
    _check_structure(w, invalid)
    # the same search by hand on the model's own root outputs
    root = m._root_inference_eager(obs)
    s = MuZeroSearch(B, SearchConfig(A, S, E, policy="stochastic", num_chance_outcomes=Cn))
    s.set_stochastic_mlp_weights({k: t.detach() for k, t in mx.nn.stochastic_mlp_weights(m.network).items()}, 10, 0.97)
    out = s.search_stochastic_mlp(root, key=[3, 4], invalid_actions=invalid, dirichlet_fraction=0.0)
    assert torch.equal(out.action, a) and torch.equal(out.action_weights.view(torch.int32), w.view(torch.int32))
    assert torch.equal(root[1].view(torch.int32), v.view(torch.int32))
    s.close()


def test_model_act_callable_route(monkeypatch):
    """MUAX_AMD_STOCHASTIC_MLP=0: StochasticMuZeroPolicy on callables built from the modules; the same structural checks
    (no equality of bits across the routes: torch's matmul is not the spec)."""
    monkeypatch.setenv("MUAX_AMD_STOCHASTIC_MLP", "0")
    B, A = 9, 4
    m = _model(A)
    obs, invalid = _act_inputs(B, A, 16)
    a, w = m.act([3, 4], obs, with_pi=True, obs_from_batch=True, num_simulations=20, invalid_actions=invalid,
                 device_outputs=True)
    assert m._last_route == "callables"
    _check_structure(w, invalid)
    assert not invalid[torch.arange(B), a.long()].any()


def test_model_update_step_and_rebound_weights(monkeypatch):
    """One update() on a host-buffer batch at B = 4, L = 3: the loss is finite, every module's parameters change, and the
    next act() searches with the new weights (== the search by hand on them)."""
    import muax_amd as mx
    monkeypatch.delenv("MUAX_AMD_STOCHASTIC_MLP", raising=False)
    B, L, A, Cn, E, od, S = 4, 3, 4, 32, 16, 16, 10
    m = _model(A, Cn, E)
    obs, invalid = _act_inputs(5, A, od)
    kw = dict(with_pi=True, obs_from_batch=True, num_simulations=S, invalid_actions=invalid, dirichlet_fraction=0.0,
              device_outputs=True)
    m.act([1, 2], obs, **kw)  # binds the weights of the first version
    rng = np.random.default_rng(4)
    batch = mx.Transition(obs=rng.uniform(0, 1, (B, L, od)).astype(F32), a=rng.integers(0, A, (B, L)),
                          r=rng.uniform(-1, 2, (B, L)).astype(F32), Rn=rng.uniform(-5, 9, (B, L)).astype(F32),
                          pi=rng.dirichlet(np.ones(A), (B, L)).astype(F32))
    before = [[p.detach().clone() for p in mod.parameters()] for mod in m.network]
    with pytest.raises(ValueError):
        m.update(batch, backend="hip")
    loss = m.update(batch)["loss"]
    assert np.isfinite(loss)
    for mod, old in zip(m.network, before):
        assert any(not torch.equal(p.detach(), q) for p, q in zip(mod.parameters(), old)), type(mod).__name__
    a, w = m.act([1, 2], obs, **kw)
    assert m._last_route == "hip_stochastic_mlp"
    s = mx.MuZeroSearch(5, mx.SearchConfig(A, S, E, policy="stochastic", num_chance_outcomes=Cn))
    s.set_stochastic_mlp_weights({k: t.detach() for k, t in mx.nn.stochastic_mlp_weights(m.network).items()}, 10, 0.97)
    out = s.search_stochastic_mlp(m._root_inference_eager(obs), key=[1, 2], invalid_actions=invalid, dirichlet_fraction=0.0)
    assert torch.equal(out.action, a) and torch.equal(out.action_weights.view(torch.int32), w.view(torch.int32))
    s.close()


def test_refusals_name_the_limit():
    """What the two entries refuse on the host, before any launch."""
    from muax_amd import MuZeroSearch, SearchConfig
    A, Cn, E = 3, 2, 4
    w = {k: torch.from_numpy(v).cuda() for k, v in smr.random_weights(1, A, Cn, E, 8).items()}
    s = MuZeroSearch(2, SearchConfig(A, 3, E, policy="stochastic", num_chance_outcomes=Cn))
    z = lambda *sh, dt=torch.float32: torch.zeros(*sh, dtype=dt, device="cuda")  # noqa: E731
    with pytest.raises(ValueError, match="set_stochastic_mlp_weights"):
        s.search_stochastic_mlp((z(2, A), z(2), z(2, E)))
    from muax_amd import _lib
    o = _lib.args(_lib.MzsStochasticOutputs)
    L = s._L
    assert L.mzs_mlp_stochastic_recurrent(s._h, None, None, None, C.byref(o), None) == -1
    assert L.mzs_last_error(s._h).decode() == "mzs_mlp_stochastic_recurrent: call mzs_mlp_set_stochastic_weights first"
    for support in (7, 32):
        w2 = {k: torch.from_numpy(v).cuda() for k, v in smr.random_weights(1, A, Cn, E, support).items()}
        with pytest.raises(ValueError, match=r"support_size must be 8\.\.31"):
            s.set_stochastic_mlp_weights(w2, support, 0.99)
    d = MuZeroSearch(2, SearchConfig(A, 3, E))
    raw = _lib.args(_lib.MzsStochasticMlpWeights, support_size=8, discount=0.99, **{k: t.data_ptr() for k, t in w.items()})
    assert d._L.mzs_mlp_set_stochastic_weights(d._h, C.byref(raw)) == -1
    assert d._L.mzs_last_error(d._h).decode() == \
        "mzs_mlp_set_stochastic_weights: this handle does not run the stochastic policy (policy 2)"
    raw.struct_size = 8
    assert L.mzs_mlp_set_stochastic_weights(s._h, C.byref(raw)) == -1
    assert L.mzs_last_error(s._h).decode() == "mzs_mlp_set_stochastic_weights: null or size mismatch (ABI)"
    assert d._L.mzs_mlp_stochastic_recurrent(d._h, None, None, None, C.byref(o), None) == -1
    assert "does not run the stochastic policy" in d._L.mzs_last_error(d._h).decode()
    u = MuZeroSearch(2, SearchConfig(A, 3, 6, policy="stochastic", num_chance_outcomes=Cn, state_embed_dim=6,
                                     afterstate_embed_dim=4))
    w6 = {k: torch.from_numpy(v).cuda() for k, v in smr.random_weights(1, A, Cn, 6, 8).items()}
    with pytest.raises(ValueError, match="must both equal embed_dim"):
        u.set_stochastic_mlp_weights(w6, 8, 0.99)
    s.set_stochastic_mlp_weights(w, 8, 0.99)
    assert L.mzs_mlp_stochastic_recurrent(s._h, None, None, None, C.byref(o), None) == -1
    assert L.mzs_last_error(s._h).decode() == "mzs_mlp_stochastic_recurrent: null input"
    for h in (s, d, u):
        h.close()
