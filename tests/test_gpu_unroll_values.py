"""GPU tests of the forward value unroll (mz_mlp_unroll_kernel in muax_amd/csrc/mz_unroll.cuh): through the C ABI alone,
every buffer a view between the 64-element guards of tests/replay_abi.py, against the C oracle's chain
(tests/unroll_reference.py) bit for bit; then through MuZero.unroll_values, DeviceReplayBuffer and fit_vector.

Shapes (A, E, support, obs_dim): between them the fan-in of a layer takes 1, 7, 8, 9, 16, 17, 33 and 128 -- below, at
and above the eight-link blocks of gen_linear, with and without a tail --, the support heads fill two, three and four
16-lane slots, E and A sit on either side of 16 and at 64.  B in {1, 3, 257}: one block and many; (L, kp) in {(1, 1),
(5, 1), (5, 2), (5, 5)}: kp == L, kp < L (stride L), no dynamics step at all.  Rows are independent and step i depends
on columns < i only, so ONE oracle chain per shape (257 rows, 5 steps) is the reference of every (B, L, kp).

Bit for bit means the uint32 patterns, except that a NaN priority (from a NaN return) is held to being a NaN: which
payload a subtraction hands on is not part of the arithmetic spec."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import muax_amd as mx
import priority_reference as pref
import unroll_reference as uref
from helpers import set_trio, train_model
from muax_amd import _lib, vector
from replay_abi import Guarded

pytestmark = pytest.mark.gpu
SHAPES = [(2, 8, 10, 4), (1, 1, 8, 1), (16, 15, 16, 17), (17, 16, 24, 7), (15, 17, 31, 9), (64, 1, 10, 1), (64, 64, 31, 128)]
BATCHES = (1, 3, 257)
WINDOWS = ((1, 1), (5, 1), (5, 2), (5, 5))
NAN, INF = float("nan"), float("inf")
CPU_BAR = 2e-5  # test_unroll_values_cpu.py: of the case's largest priority


@functools.lru_cache(maxsize=None)
def _case(A, E, support, obs_dim, B=257, L=5, bias_scale=0.1):
    from oracle import pyoracle
    c = uref.make_case(pyoracle, A, E, support, obs_dim, B, L, bias_scale=bias_scale)
    c["v"], c["p"] = uref.oracle_chain(pyoracle, c["w"], c["obs"], c["a"], c["Rn"], support, L)
    return c


class Unroll:
    """The weights of one net as guarded device arrays, and the call."""

    def __init__(self, w, support):
        self.L = _lib.load()
        self.g = {n: Guarded.of(np.asarray(w[n], np.float32)) for n in _lib.MLP_WEIGHT_NAMES}
        self.support = support
        (self.obs_dim, self.E), self.A = w["repr_w"].shape, w["pp_b2"].shape[0]

    def __call__(self, obs, a, Rn, kp, values=True, prio=True, override=None):
        """(status, values [B, kp] or None, prio [B, kp] or None) as host arrays; asserts that every guard, every input
        and every weight is bit-identical afterwards."""
        obs, a, Rn = Guarded.of(obs, torch.float32), Guarded.of(a, torch.int32), Guarded.of(Rn, torch.float32)
        B, L = a.t.shape
        out = [Guarded(B, kp, torch.float32, flat=False) if on else None for on in (values, prio)]
        w = _lib.MzsMlpWeights()
        w.struct_size = C.sizeof(_lib.MzsMlpWeights)
        w.obs_dim, w.support_size, w.discount = self.obs_dim, self.support, 0.99
        for n, g in self.g.items():
            setattr(w, n, g.ptr)
        u = _lib.MzsUnrollArgs()
        u.struct_size = C.sizeof(_lib.MzsUnrollArgs)
        u.device, u.batch, u.row_steps, u.k_prio = torch.cuda.current_device(), B, L, kp
        u.num_actions, u.embed_dim = self.A, self.E
        u.obs, u.actions, u.returns = obs.ptr, a.ptr, Rn.ptr
        u.values, u.prio = (g.ptr if g is not None else None for g in out)
        for k, x in (override or {}).items():
            setattr(w if k in ("obs_dim", "support_size") else u, k, x)
        inputs = [obs, a, Rn] + list(self.g.values())
        torch.cuda.synchronize()
        before = [g.bits.clone() for g in inputs]
        untouched = [g.bits.clone() for g in out if g is not None]
        rc = self.L.mzs_mlp_unroll_values(C.byref(w), C.byref(u), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        for g, was in zip(inputs, before):
            assert torch.equal(g.bits, was), "an input or a weight was written"
        for g in out:
            assert g is None or g.guards_intact(), "a guard of an output was overwritten"
        if rc != _lib.MZS_OK:
            for g, was in zip([g for g in out if g is not None], untouched):
                assert torch.equal(g.bits, was), "a refused call wrote an output"
        return (rc,) + tuple(g.host() if g is not None else None for g in out)


def _same_bits(got, want, what):
    got, want = uref.bits(got), uref.bits(want)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} of {got.size} differ, first at {tuple(bad[0])}: " \
                          f"{got[tuple(bad[0])]:#010x} vs {want[tuple(bad[0])]:#010x}"


def _same_prio(got, want, what):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    _same_bits(np.where(nan, 0, got), np.where(nan, 0, want), what)


# ---- 1. the C ABI against the oracle chain ----
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_values_and_priorities_have_the_oracles_bits(oracle, shape):
    A, E, support, obs_dim = shape
    c = _case(*shape)
    run = Unroll(c["w"], support)
    for B in BATCHES:
        for L, kp in WINDOWS:
            obs, a, Rn = c["obs"][:B], c["a"][:B, :L], c["Rn"][:B, :L]
            rc, v, p = run(obs, a, Rn, kp)
            assert rc == _lib.MZS_OK, run.L.mzs_last_error(None)
            _same_bits(v, c["v"][:B, :kp], (shape, B, L, kp, "values"))
            _same_bits(p, c["p"][:B, :kp], (shape, B, L, kp, "prio"))
            rc, v2, p2 = run(obs, a, Rn, kp)  # a second call: the same bits
            assert rc == _lib.MZS_OK
            _same_bits(v2, v, "second call, values")
            _same_bits(p2, p, "second call, prio")
    # either output alone
    obs, a, Rn = c["obs"][:3], c["a"][:3], c["Rn"][:3]
    rc, v, p = run(obs, a, Rn, 5, prio=False)
    assert rc == _lib.MZS_OK and p is None
    _same_bits(v, c["v"][:3], "values alone")
    rc, v, p = run(obs, a, Rn, 5, values=False)
    assert rc == _lib.MZS_OK and v is None
    _same_bits(p, c["p"][:3], "prio alone")


def _scaled_value_head(c, reach=300.0):
    """The weights with the value head's output layer scaled until its root logits reach about +-reach."""
    from oracle import mz_train_numpy as ref
    w64 = {n: np.asarray(c["w"][n], np.float64) for n in ref.WEIGHT_NAMES}
    s0 = ref._minmax(np.asarray(c["obs"], np.float64) @ w64["repr_w"] + w64["repr_b"])[0]
    logits, _ = ref._mlp(w64, "pv", s0)
    f = np.float32(reach / np.abs(logits).max())
    w = dict(c["w"])
    w["pv_w2"], w["pv_b2"] = c["w"]["pv_w2"] * f, c["w"]["pv_b2"] * f
    return w


@pytest.mark.parametrize("shape", [(2, 8, 10, 4), (17, 16, 24, 7), (64, 64, 31, 128)], ids=str)
def test_edges_keep_the_oracles_bits(oracle, shape):
    A, E, support, obs_dim = shape
    c = _case(*shape, B=48, L=4)
    B, L = 48, 4
    top = float(uref._inv_h(support))

    def check(w, obs, a, Rn, what, chain_a=None):
        v, p = uref.oracle_chain(oracle, w, obs, a if chain_a is None else chain_a, Rn, support, L)
        rc, gv, gp = Unroll(w, support)(obs, a, Rn, L)
        assert rc == _lib.MZS_OK, what
        _same_bits(gv, v, (shape, what, "values"))
        _same_prio(gp, p, (shape, what, "prio"))
        return v, gp

    # value logits of about +-300: the softmax is one-hot on whichever bin wins; then with the first and with the last
    # bin's bias raised above every logit, so that the decode saturates at either end of the support in every row
    big = _scaled_value_head(c)
    v, _ = check(big, c["obs"], c["a"], c["Rn"], "large logits")
    assert np.abs(v).max() > 0.25 * top, (v.min(), v.max(), top)
    for end, sign in ((0, -1.0), (2 * support, 1.0)):
        w = dict(big)
        w["pv_b2"] = big["pv_b2"].copy()
        w["pv_b2"][end] += np.float32(1000.0)
        v, _ = check(w, c["obs"], c["a"], c["Rn"], f"large logits, bin {end}")
        assert (np.abs(v - sign * top) <= 1e-3 * top).all(), (end, v.min(), v.max(), top)
    # all-zero observations on a zero-bias net: the representation is all zeros, the normaliser's < 1e-5 branch
    z = _case(*shape, B=48, L=4, bias_scale=0.0)
    assert not z["w"]["repr_b"].any()
    check(z["w"], np.zeros_like(z["obs"]), z["a"], z["Rn"], "zero observations")
    # the first and the last action everywhere
    check(c["w"], c["obs"], np.zeros_like(c["a"]), c["Rn"], "actions all 0")
    check(c["w"], c["obs"], np.full_like(c["a"], A - 1), c["Rn"], "actions all A - 1")
    # returns that are no numbers, or huge
    Rn = c["Rn"].copy()
    Rn[0], Rn[1], Rn[2] = (NAN, INF, -INF, 1e7), (-1e7, NAN, 1e7, -INF), (INF, INF, NAN, NAN)
    _, gp = check(c["w"], c["obs"], c["a"], Rn, "special returns")
    assert np.array_equal(np.isnan(gp[:3]), np.isnan(Rn[:3])) and np.array_equal(np.isinf(gp[:3]), np.isinf(Rn[:3]))
    assert (gp[:3][np.isinf(Rn[:3])] == INF).all() and np.isfinite(gp[3:]).all()
    # an action below and one above the range at step 1 of 4: the all-zero one-hot (the oracle: a zero row, action A)
    a = c["a"].copy()
    a[5, 1], a[9, 1] = -1, A
    v, _ = check(c["w"], c["obs"], a, c["Rn"], "actions out of range")
    assert np.array_equal(uref.bits(v[:, :2]), uref.bits(c["v"][:, :2]))
    assert not np.array_equal(uref.bits(v[[5, 9], 2:]), uref.bits(c["v"][[5, 9], 2:]))


REJECTED = [({"obs_dim": 129}, _lib.MZS_E_UNSUPPORTED, "obs_dim must be 1..128"),
            ({"embed_dim": 65}, _lib.MZS_E_UNSUPPORTED, "embed_dim must be 1..64"),
            ({"num_actions": 65}, _lib.MZS_E_UNSUPPORTED, "num_actions must be 1..64"),
            ({"support_size": 7}, _lib.MZS_E_UNSUPPORTED, "support_size must be 8..31"),
            ({"support_size": 32}, _lib.MZS_E_UNSUPPORTED, "support_size must be 8..31"),
            ({"k_prio": 6}, _lib.MZS_E_INVALID, "k_prio must be in 1..row_steps"),
            ({"k_prio": 0}, _lib.MZS_E_INVALID, "k_prio"), ({"batch": 0}, _lib.MZS_E_INVALID, "batch"),
            ({"obs_dim": 0}, _lib.MZS_E_UNSUPPORTED, "obs_dim"), ({"embed_dim": 0}, _lib.MZS_E_UNSUPPORTED, "embed_dim"),
            ({"num_actions": 0}, _lib.MZS_E_UNSUPPORTED, "num_actions"),
            ({"struct_size": C.sizeof(_lib.MzsUnrollArgs) - 8}, _lib.MZS_E_INVALID, "size mismatch"),
            ({"obs": None}, _lib.MZS_E_INVALID, "null"), ({"actions": None}, _lib.MZS_E_INVALID, "null"),
            ({"returns": None}, _lib.MZS_E_INVALID, "null"),
            ({"values": None, "prio": None}, _lib.MZS_E_INVALID, "at least one")]


def test_limits_are_refused_before_any_launch_with_the_limit_named(oracle):
    c = _case(2, 8, 10, 4)
    run = Unroll(c["w"], 10)
    for override, code, text in REJECTED:  # (the call asserts that a refused call wrote nothing)
        rc, _, _ = run(c["obs"][:3], c["a"][:3], c["Rn"][:3], 5, override=override)
        message = run.L.mzs_last_error(None).decode()
        assert rc == code and "mzs_mlp_unroll_values" in message and text in message, (override, rc, message)
    # through the model: "hip" hands the library's refusal on, "auto" takes the torch route
    m = train_model(2, 65, 4, seed=5, support=10)
    b = _batch(_case(2, 8, 10, 4), 6)
    with pytest.raises(ValueError, match="embed_dim must be 1..64"):
        m.unroll_values(b, backend="hip")
    v, p = m.unroll_values(b)
    vt, pt = m.unroll_values(b, backend="torch")
    assert v.shape == (6, 5) and torch.equal(v, vt) and torch.equal(p, pt)
    m = train_model(2, 8, 4, seed=5, support=7)
    with pytest.raises(ValueError, match="support_size must be 8..31"):
        m.unroll_values(b, backend="hip")
    assert torch.equal(m.unroll_values(b)[0], m.unroll_values(b, backend="torch")[0])


# ---- 2. MuZero.unroll_values ----
def _batch(c, B):
    L = c["a"].shape[1]
    obs = np.repeat(c["obs"][:B, None], L, 1)
    obs[:, 1:] += 100.0  # only obs[:, 0] may be read
    return mx.Transition(obs=obs, a=c["a"][:B], r=np.zeros((B, L), np.float32), Rn=c["Rn"][:B],
                         pi=np.full((B, L, 1, c["A"]), 1.0 / c["A"], np.float32))


def test_the_first_value_is_acts_root_value_and_the_routes_agree(oracle):
    c = _case(2, 8, 10, 4)  # CartPole's shape
    m = train_model(2, 8, 4, seed=3, support=10)
    set_trio(m, **c["w"])
    m.weights_changed()
    B = 64
    b = _batch(c, B)
    v, p = m.unroll_values(b)
    assert v.shape == p.shape == (B, 5) and v.dtype == p.dtype == torch.float32 and v.device == m.device
    _same_bits(v.cpu().numpy(), c["v"][:B], "model, values")
    _same_bits(p.cpu().numpy(), c["p"][:B], "model, prio")
    _, root_value = m.act(mx.prng.PRNGKey(7), torch.as_tensor(c["obs"][:B], device=m.device), with_value=True, obs_from_batch=True,
                          num_simulations=8, device_outputs=True)
    assert torch.equal(root_value.view(torch.int32), v[:, 0].contiguous().view(torch.int32))
    vh, ph = m.unroll_values(b, backend="hip")
    assert torch.equal(vh, v) and torch.equal(ph, p)
    vt, pt = m.unroll_values(b, backend="torch")
    worst = float((ph - pt).abs().max() / pt.max())
    print(f"[hip against torch: priorities within {worst:.2e} of the largest]", end=" ")
    assert worst <= CPU_BAR
    for kp in (1, 3):  # kp < L: stride L, the prefix; device tensors of the kernel's types pass through as they are
        dev_b = mx.Transition(obs=torch.as_tensor(b.obs, device=m.device), a=torch.as_tensor(b.a, device=m.device),
                              r=b.r, Rn=torch.as_tensor(b.Rn, device=m.device), pi=b.pi)
        vk, pk = m.unroll_values(dev_b, k_prio=kp)
        assert torch.equal(vk, v[:, :kp]) and torch.equal(pk, p[:, :kp])
        assert torch.equal(vector.unroll_value_priorities(m, dev_b, kp), p[:, :kp])
    with pytest.raises(ValueError, match="k_prio"):
        m.unroll_values(b, k_prio=6)
    # the struct is kept while the parameters stay where they are, and follows an in-place update
    fused = m._fused_unroll
    kept = fused._w
    with torch.no_grad():
        mx.nn.mlp_trio_weights(m.network)["pv_b2"][0] += 2.0  # (one bin: a shift of all of them cancels in the softmax)
    v3, _ = m.unroll_values(b)
    assert m._fused_unroll is fused and fused._w is kept and not torch.equal(v3, v)


# ---- 3. the loop closed: sample -> unroll_value_priorities -> update_priorities ----
N, GAMMA, K = 3, 0.997, 4
EPISODES = (12, 20, 9)


def test_sampled_windows_get_the_kernels_priorities_written_back():
    rng = np.random.default_rng(31)
    M = sum(EPISODES)
    buf = mx.DeviceReplayBuffer(3, 64, random_seed=0)
    buf.add_raw(rng.uniform(-1, 1, (M, 4)).astype(np.float32), rng.integers(0, 2, M), rng.uniform(-2, 3, M),
                rng.uniform(-30, 60, M), rng.dirichlet(np.ones(2), M).astype(np.float32), list(EPISODES), N, GAMMA, 0.5,
                weight="mean")
    m = train_model(2, 8, 4, seed=3, support=10)
    batch, (serial, start) = buf.sample(16, k_steps=K, key=5, with_indices=True)
    prio = vector.unroll_value_priorities(m, batch)
    assert prio.shape == (16, K) and prio.device == batch.Rn.device
    v, _ = m.unroll_values(batch)
    assert torch.equal(prio, (v - batch.Rn).abs())
    live = [(e.slot, e.start, e.length, e.serial) for e in buf._eps]
    before = {n: buf._t[n].cpu().numpy() for n in ("w", "cw", "t_w")}
    for weight in ("mean", "sum"):
        want = pref.update(before["w"], before["cw"], before["t_w"], live, serial.cpu().numpy(), start.cpu().numpy(),
                           prio.cpu().numpy(), 1.0, 0.0, weight)
        buf.update_priorities((serial, start), prio, alpha=1.0, weight=weight)
        torch.cuda.synchronize()
        assert want[3]
        for n, ref in zip(("w", "cw", "t_w"), want):  # alpha == 1: a widening, an fabs, one addition -- bit for bit
            assert np.array_equal(buf._t[n].cpu().numpy().view(np.uint64), ref.view(np.uint64)), (weight, n)


class _Recording(mx.DeviceReplayBuffer):
    """The device buffer, keeping a copy of what every update_priorities call was given."""
    calls = None

    def update_priorities(self, indices, priorities, **kw):
        self.calls = (self.calls or []) + [(indices[0].clone(), indices[1].clone(), priorities.clone(), kw)]
        return super().update_priorities(indices, priorities, **kw)


def _fit_vector_once(seed, iterations, **kw):
    """The arguments of test_gpu_priority.py's _fit_vector_once, plus `kw`."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    from cartpole_env import VectorCartPole
    g = torch.Generator().manual_seed(0)
    net = mx.nn.MZNetwork(mx.nn.Representation(8, generator=g), mx.nn.Prediction(2, 21, generator=g),
                          mx.nn.Dynamic(8, 2, 21, generator=g))
    model = mx.MuZero(net, optimizer=mx.optimizers.create_optimizer("adam", 5e-3))
    buf, rows = _Recording(64, 4096, random_seed=seed), []
    mx.fit_vector(model, VectorCartPole(16, seed=0), VectorCartPole(2, max_episode_steps=20, seed=1), n_step=3, buffer=buf,
                  iterations=iterations, steps_per_iteration=8, num_simulations=8, k_steps=3, num_trajectory=8,
                  sample_per_trajectory=2, num_update_per_iteration=2, test_interval=10, random_seed=3, metrics=rows, **kw)
    return model, buf, rows


def _comparable(rows):
    return [{k: repr(v) for k, v in r.items() if k != "collect_s"} for r in rows]  # (repr: a NaN equals a NaN)


def test_fit_vector_priority_steps():
    _, buf, rows = _fit_vector_once(13, 2, priority_update=True, priority_steps=3)
    losses = [r["loss"] for r in rows if "loss" in r]
    assert len(rows) == 2 and losses and np.isfinite(losses).all()
    assert len(buf.calls) == rows[-1]["training_step"] > 0
    assert all(p.shape == (16, 3) and p.dtype == torch.float32 for *_, p, _ in buf.calls)
    assert all(kw == {"alpha": 0.5, "weight": "mean"} for *_, kw in buf.calls)
    _, buf5, _ = _fit_vector_once(13, 1, priority_update=True, priority_steps=5)  # more than k_steps: k_steps
    assert all(p.shape == (16, 3) for *_, p, _ in buf5.calls)
    # None is the loop as it was: value_priorities, [B], and the rows of a run that never names the argument
    _, buf_none, rows_none = _fit_vector_once(13, 2, priority_update=True, priority_steps=None)
    _, buf_old, rows_old = _fit_vector_once(13, 2, priority_update=True)
    assert all(p.shape == (16,) for *_, p, _ in buf_none.calls)
    assert _comparable(rows_none) == _comparable(rows_old)
    assert all(torch.equal(x[2], y[2]) for x, y in zip(buf_none.calls, buf_old.calls))
    # ignored where the write-back is off
    _, buf_off, rows_off = _fit_vector_once(13, 2, priority_steps=3)
    _, _, rows_plain = _fit_vector_once(13, 2)
    assert buf_off.calls is None and _comparable(rows_off) == _comparable(rows_plain)
