"""The Stochastic MuZero search kernels at their numeric edges (tests/stochastic_edge_cases.py: exact ties, one-ulp
margins, shifted logits and support heads, next states of range 0 and 2**-k, zero rewards, masks, temperatures and
Dirichlet fractions, max_depth cuts) against the CPU stepper, on every route: the one-launch search
(mzs_mlp_stochastic_search), the three-launch route on the same handle, the step-wise entries around the recurrent kernel
(mzs_select_stochastic -> mzs_mlp_stochastic_recurrent -> mzs_expand_backup_stochastic), the root kernel
(mzs_mlp_stochastic_root) and the search on observations (mzs_mlp_stochastic_search_obs).  tests/test_stochastic_edges_cpu.py
proves that the reference reaches each edge.  Every comparison is == on the uint32 views."""
import ctypes as C

import numpy as np
import pytest
import torch

import stochastic_edge_cases as ec

pytestmark = pytest.mark.gpu
F32 = np.float32
SENTINEL = 0x5A5AA5A5  # the bit pattern untouched output words must keep
GUARD = 37             # guard words behind every output array
KEY = ec.KEY


def _tt(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def _handle(c, batch=None, representation=None, **cfg):
    from muax_amd import MuZeroSearch, SearchConfig
    A, Cn, E, support, B, S = c.shape
    s = MuZeroSearch(batch or B, SearchConfig(A, S, E, policy="stochastic", num_chance_outcomes=Cn, tiebreak=c.options.tiebreak,
                                              max_depth=c.options.max_depth, **cfg))
    s.set_stochastic_mlp_weights({k: _tt(v) for k, v in c.weights.items()}, support, c.options.discount)
    if representation is not None:
        s.set_stochastic_representation(*[_tt(x) for x in representation])
    return s


def _root(c):
    return tuple(_tt(x) for x in c.root)


def _kw(c, **more):
    o = c.options
    return dict(key=list(KEY), invalid_actions=_tt(c.invalid), dirichlet_noise=_tt(c.noise), dirichlet_fraction=o.fraction,
                temperature=o.temperature, gumbel=_tt(c.gumbel), with_tree=True, **more)


def _snapshot(s, out):
    """Host copies of everything a search returns (the handle's buffers are overwritten by the next call)."""
    tree = None if out.search_tree is None else type(out.search_tree)(*[t.clone() for t in out.search_tree])
    return dict(action=out.action.cpu().numpy().copy(), weights=out.action_weights.cpu().numpy().copy(),
                value=s.search_value.cpu().numpy().copy(), depth_sum=s.depth_sum.cpu().numpy().copy(), tree=tree)


def _check(got, r, rows=slice(None)):
    """A snapshot against a reference run (`rows`: the roots of the snapshot the reference holds)."""
    from helpers import assert_trees_equal
    assert np.array_equal(r["action"], got["action"][rows])
    assert np.array_equal(_bits(r["weights"]), _bits(got["weights"][rows]))
    assert np.array_equal(_bits(r["value"]), _bits(got["value"][rows]))
    assert np.array_equal(np.asarray(r["depth_sum"]).astype(np.int64), got["depth_sum"][rows].astype(np.int64))
    tree = got["tree"] if rows == slice(None) else type(got["tree"])(*[t[rows] for t in got["tree"]])
    # assert_trees_equal compares values; the uint32 views on top: a -0.0 is not a +0.0 here
    assert_trees_equal(r["tree"], tree, exact_floats=True)
    for f, a in r["tree"].arrays().items():
        b = getattr(tree, f).cpu().numpy()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{f}: the sign of a zero, or a NaN's payload"


def _same(a, b, rows=slice(None)):
    """Two snapshots hold the same bits (`rows`: those of a, when b holds fewer roots)."""
    for f in ("action", "weights", "value", "depth_sum"):
        assert np.array_equal(np.ascontiguousarray(a[f][rows]).view(np.uint32), np.ascontiguousarray(b[f]).view(np.uint32)), f
    for f in a["tree"]._fields:
        x, y = getattr(a["tree"], f)[rows].contiguous(), getattr(b["tree"], f)
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f


# ---------------------------------------------------------------- whole search: one launch, three launches
@pytest.mark.parametrize("name", ec.NAMES)
def test_one_launch_and_three_launches_match_stepper(name):
    """The one launch against the stepper; then the three-launch route on the SAME handle: the one launch's bits, and the
    stepper's."""
    r = ec.reference(name)
    c = r["case"]
    s = _handle(c)
    one = _snapshot(s, s.search_stochastic_mlp(_root(c), one_launch=True, **_kw(c)))
    _check(one, r)
    three = _snapshot(s, s.search_stochastic_mlp(_root(c), **_kw(c)))
    _check(three, r)
    _same(one, three)
    s.close()


# ---------------------------------------------------------------- the step-wise entries around the recurrent kernel
STEPWISE = ec.names("all_ties", "chance_ties_only", "noisy_decisions_chance_ties", "flat_states", "shifted_logits", "shifted_support")


@pytest.mark.parametrize("name", STEPWISE)
def test_hand_written_loop_matches_stepper(name):
    """mzs_select_stochastic -> mzs_mlp_stochastic_recurrent -> mzs_expand_backup_stochastic: per simulation the slot, the
    parent's kind, the parent embedding and the recurrent kernel's outputs on the rows of the parent's kind; at the end
    what the whole search returns."""
    from muax_amd.search import STOCHASTIC_OUTPUT_FIELDS
    r = ec.reference(name)
    c = r["case"]
    A, Cn, E, support, B, S = c.shape
    o = c.options
    s = _handle(c)
    s.root_stochastic(*_root(c), list(KEY), _tt(c.invalid), _tt(c.noise), o.fraction)
    for sim in range(S):
        slot, kind, pemb = s.select_stochastic(sim)
        assert np.array_equal(r["slots"][sim], slot.cpu().numpy()), f"slot, simulation {sim}"
        assert np.array_equal(r["kinds"][sim], kind.cpu().numpy()), f"parent kind, simulation {sim}"
        assert np.array_equal(_bits(r["pembs"][sim]), _bits(pemb.cpu().numpy())), f"parent embedding, simulation {sim}"
        outputs = s.stochastic_mlp_recurrent(slot, kind, pemb)
        (cl, av), ae, (al, v, rw, d), se = r["rows"][sim]
        want = dict(zip(STOCHASTIC_OUTPUT_FIELDS, s._stochastic_out[1]))
        ref = dict(chance_logits=(cl, 1), afterstate_value=(av, 1), afterstate_embedding=(ae, 1), action_logits=(al, 0),
                   value=(v, 0), reward=(rw, 0), discount=(d, 0), state_embedding=(se, 0))
        assert set(ref) == set(want)
        k = r["kinds"][sim]
        for n, (x, of_kind) in ref.items():
            got = want[n].cpu().numpy().reshape(B, -1)[k == of_kind]
            exp = np.asarray(x, F32).reshape(B, -1)[k == of_kind]
            assert np.array_equal(_bits(exp), _bits(got)), f"{n}, simulation {sim}"
        s.expand_backup_stochastic_outputs(sim, outputs)
    out = s.finish_stochastic(o.temperature, _tt(c.gumbel), with_tree=True)
    _check(_snapshot(s, out), r)
    s.close()


# ---------------------------------------------------------------- the device block
@pytest.mark.parametrize("name", ["temperature_0-s0", "temperature_1e-3-s2", "temperature_50-s0", "fraction_1-s2", "fraction_0_with_noise-s0",
                                  "all_ties_noise-s1"])
def test_device_block_replaces_the_struct_fields(name):
    """key, temperature and dirichlet_fraction through mzs_stochastic_search_block's device block, the struct's own fields
    holding OTHER values: the bits of the struct-field call, which are the stepper's."""
    from muax_amd import _lib
    from muax_amd.search import MzsStochasticSearchArgs
    r = ec.reference(name)
    c = r["case"]
    A, Cn, E, support, B, S = c.shape
    o = c.options
    s = _handle(c)
    fraction = o.fraction if c.noise is not None else 0.0
    ref = _snapshot(s, s.search_stochastic_mlp(_root(c), one_launch=True, **_kw(c)))
    _check(ref, r)
    kw = (C.c_uint32 * 2)(*KEY)
    host = torch.empty(4 + 2 * S, dtype=torch.int32)
    _lib.check(s._L.mzs_stochastic_search_block(C.byref(kw), S, o.temperature, fraction, host.data_ptr()))
    block = host.cuda()
    root, invalid, noise, gumbel = _root(c), _tt(c.invalid), _tt(c.noise), _tt(c.gumbel)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    outs = dict(action=torch.full((B,), -7, dtype=torch.int32, device="cuda"), action_weights=torch.full((B, A), -7.0, device="cuda"),
                search_value=torch.full((B,), -7.0, device="cuda"), depth_sum=torch.full((B,), -7, dtype=torch.int32, device="cuda"))
    a = _lib.args(MzsStochasticSearchArgs, export_tree=1, prior_logits=p(root[0]), value=p(root[1]), embedding=p(root[2]),
                  invalid_actions=p(invalid), dirichlet_noise=p(noise), gumbel=p(gumbel), key=(77, 99),
                  dirichlet_fraction=0.5 if noise is not None else 0.0, temperature=3.0, device_block=block.data_ptr(),
                  **{n: t.data_ptr() for n, t in outs.items()})
    _lib.check(s._L.mzs_mlp_stochastic_search(s._h, C.byref(a), None), s._h)
    torch.cuda.synchronize()
    assert np.array_equal(outs["action"].cpu().numpy(), ref["action"])
    assert np.array_equal(_bits(outs["action_weights"].cpu().numpy()), _bits(ref["weights"]))
    assert np.array_equal(_bits(outs["search_value"].cpu().numpy()), _bits(ref["value"]))
    assert np.array_equal(outs["depth_sum"].cpu().numpy(), ref["depth_sum"])
    tree = s._export_tree()
    for f in tree._fields:
        assert torch.equal(getattr(tree, f).view(torch.int32), getattr(ref["tree"], f).view(torch.int32)), f
    s.close()


# ---------------------------------------------------------------- more roots than one round of workgroups
@pytest.mark.parametrize("tiebreak", [False, True])
def test_more_roots_than_one_round(tiebreak):
    """B = waves * resident workgroups + 1 at S = 3: the last root's bits are those of the same root run alone
    (global_batch / root_offset); without tie-break noise the first two roots and the last also equal the stepper."""
    from muax_amd import search
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = ec.more_roots_batch(cus)
    c = ec.more_roots_case(B, tiebreak)
    pl = search.stochastic_plan(*c.shape[:4], 3)
    assert B == pl["roots_per_cu"] * cus + 1 and -(-B // pl["waves"]) > (pl["roots_per_cu"] // pl["waves"]) * cus
    s = _handle(c)
    whole = _snapshot(s, s.search_stochastic_mlp(_root(c), one_launch=True, **_kw(c)))
    s.close()
    rows = slice(B - 1, B)
    cut = lambda x: None if x is None else np.ascontiguousarray(x[rows])  # noqa: E731
    alone_case = c._replace(shape=c.shape[:4] + (1, 3), root=tuple(cut(x) for x in c.root), noise=cut(c.noise), gumbel=cut(c.gumbel))
    s = _handle(alone_case, global_batch=B, root_offset=B - 1)
    alone = _snapshot(s, s.search_stochastic_mlp(_root(alone_case), one_launch=True, **_kw(alone_case)))
    s.close()
    _same(whole, alone, rows)
    if not tiebreak:
        pick = [0, 1, B - 1]
        _check(whole, ec.run_reference(ec.rows_of(c, pick)), pick)


# ---------------------------------------------------------------- the root kernel and the search on observations
@pytest.mark.parametrize("name", ec.ROOT_NAMES)
def test_root_kernel_and_search_on_observations(name):
    """mzs_mlp_stochastic_root against the oracle's root_inference on a flat / 2**-20 wide / one-hot embedding under
    shifted root heads; mzs_mlp_stochastic_search_obs == the root kernel followed by the search, == the stepper on the
    oracle's root; the three-launch route on the observations as well."""
    rc = ec.root_case(name)
    c = rc.search
    r = ec.root_search_reference(name)
    s = _handle(c, representation=(rc.repr_w, rc.repr_b))
    obs = _tt(rc.obs)
    got = [t.clone() for t in s.stochastic_mlp_root(obs)]
    for n, want, t in zip(("prior_logits", "value", "embedding"), c.root, got):
        assert np.array_equal(_bits(want), _bits(t.cpu().numpy())), n
    after_root = _snapshot(s, s.search_stochastic_mlp(tuple(got), one_launch=True, **_kw(c)))
    _check(after_root, r)
    on_obs = _snapshot(s, s.search_stochastic_mlp(None, obs=obs, one_launch=True, **_kw(c)))
    assert np.array_equal(_bits(c.root[1]), _bits(s.root_value.cpu().numpy()))
    _same(after_root, on_obs)
    three = _snapshot(s, s.search_stochastic_mlp(None, obs=obs, **_kw(c)))
    assert np.array_equal(_bits(c.root[1]), _bits(s.root_value.cpu().numpy()))
    _same(after_root, three)
    s.close()


# ---------------------------------------------------------------- guard words
@pytest.mark.parametrize("name", ["masks_all_ties-s0", "masks_all_ties_noise-s0", "masks_generic_noise-s2", "temperature_0-s0",
                                  "temperature_0_tied_visits-s1", "temperature_0_generic-s2"])
def test_guard_words(name):
    """The all-invalid root and temperature 0 through the C ABI with sentinel tails behind every output: none is written,
    every word in front of them is, and holds the stepper's bits."""
    from muax_amd import _lib
    from muax_amd.search import MzsStochasticSearchArgs
    r = ec.reference(name)
    c = r["case"]
    A, Cn, E, support, B, S = c.shape
    o = c.options
    s = _handle(c)
    root, invalid, noise, gumbel = _root(c), _tt(c.invalid), _tt(c.noise), _tt(c.gumbel)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    widths = dict(action=1, action_weights=A, search_value=1, depth_sum=1)
    outs = {n: torch.full((B * k + GUARD,), SENTINEL, dtype=torch.int32, device="cuda") for n, k in widths.items()}
    a = _lib.args(MzsStochasticSearchArgs, export_tree=0, prior_logits=p(root[0]), value=p(root[1]), embedding=p(root[2]),
                  invalid_actions=p(invalid), dirichlet_noise=p(noise), gumbel=p(gumbel), key=KEY,
                  dirichlet_fraction=o.fraction if noise is not None else 0.0, temperature=o.temperature,
                  **{n: t.data_ptr() for n, t in outs.items()})
    _lib.check(s._L.mzs_mlp_stochastic_search(s._h, C.byref(a), None), s._h)
    torch.cuda.synchronize()
    got = {n: t.cpu().numpy().view(np.uint32) for n, t in outs.items()}
    for n, k in widths.items():
        assert (got[n][B * k:] == SENTINEL).all(), f"{n}: guard tail written"
    assert np.array_equal(got["action"][:B].view(np.int32), r["action"])
    assert np.array_equal(got["action_weights"][:B * A], _bits(r["weights"]).ravel())
    assert np.array_equal(got["search_value"][:B], _bits(r["value"]))
    assert np.array_equal(got["depth_sum"][:B].view(np.int32), np.asarray(r["depth_sum"]).astype(np.int32))
    s.close()
