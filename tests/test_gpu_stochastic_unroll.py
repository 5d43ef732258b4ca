"""GPU tests of the stochastic family's forward value unroll (mz_stoch_unroll_kernel in muax_amd/csrc/mz_unroll.cuh):
through the C ABI alone, every buffer a view between the 64-element guards of tests/replay_abi.py, against the chain
composed from the C oracle (tests/stochastic_unroll_reference.py); then through MuZero.unroll_values and fit_vector.

values, prio and codes are compared == on the bits: both sides are the one fp32 spec, so there is no tolerance and no
conditioning.  Shapes (A, C, E, support, obs_dim): the three of stochastic_train_reference.SHAPES; the narrowest; A + C =
64 with the widest embedding and support; an observation wider than E + one-hot (the scratch sizing); C and obs_dim one
past a 64-lane stride.  B in {1, 5}, (L, kp) in {(4, 1), (4, 2), (4, 4)}: kp < L exercises the row stride of the
observations, actions and returns.  Rows are independent and step i depends on columns <= i only, so ONE oracle chain per
shape (5 rows, 4 steps) is the reference of every (B, kp)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import muax_amd as mx
import priority_reference as pref
import stochastic_train_reference as stref
import stochastic_unroll_reference as suref
from muax_amd import _call, _lib
from replay_abi import Guarded

pytestmark = pytest.mark.gpu
SHAPES = list(stref.SHAPES) + [(2, 2, 1, 8, 1), (4, 60, 64, 31, 16), (3, 5, 4, 8, 128), (4, 33, 8, 8, 65)]
BATCHES = (1, 5)
L = 4
STEPS = (1, 2, L)


@functools.lru_cache(maxsize=None)
def _case(shape, B=5):
    from oracle import pyoracle
    A, Cn, E, support, od = shape
    c = suref.make_case(A, Cn, E, support, od, B, L)
    c["v"], c["p"], c["c"] = suref.oracle_chain(pyoracle, c["w"], c["obs"], c["a"], c["Rn"], A, Cn, E, support, L)
    return c


class Unroll:
    """The weights of one net as guarded device arrays, and the call."""

    def __init__(self, w, A, Cn, E, support):
        self.L = _lib.load()
        self.g = {n: Guarded.of(np.asarray(w[n], np.float32)) for n in _lib.STOCHASTIC_TRAIN_WEIGHT_NAMES}
        self.A, self.C, self.E, self.support, self.obs_dim = A, Cn, E, support, w["repr_w"].shape[0]

    def structs(self, obs, a, Rn, kp, out):
        """(weights, arguments) for guarded inputs and the guarded outputs `out` (values, prio, codes; None: NULL)."""
        B, L_ = a.t.shape
        w = _lib.args(_lib.MzsStochasticTrainWeights, obs_dim=self.obs_dim, support_size=self.support,
                      **{n: g.ptr for n, g in self.g.items()})
        u = _lib.args(_lib.MzsStochasticUnrollArgs, device=torch.cuda.current_device(), batch=B, row_steps=L_, k_prio=kp,
                      num_actions=self.A, num_chance_outcomes=self.C, embed_dim=self.E, obs=obs.ptr, actions=a.ptr,
                      returns=Rn.ptr, **{n: (g.ptr if g is not None else None) for n, g in zip(("values", "prio", "codes"), out)})
        return w, u

    def launch(self, w, u):
        return self.L.mzs_stochastic_mlp_unroll_values(C.byref(w), C.byref(u),
                                                       C.c_void_p(torch.cuda.current_stream().cuda_stream))

    @staticmethod
    def inputs(obs, a, Rn):
        obs = np.asarray(obs, np.float32)
        return (Guarded.of(obs.reshape(obs.shape[0], -1), torch.float32), Guarded.of(a, torch.int32),
                Guarded.of(Rn, torch.float32))

    @staticmethod
    def outputs(B, kp, on=(True, True, True)):
        return [Guarded(B, kp, dt, flat=False) if x else None
                for x, dt in zip(on, (torch.float32, torch.float32, torch.int32))]

    def __call__(self, obs, a, Rn, kp, on=(True, True, True)):
        """(status, values, prio, codes) as host arrays ([B, kp], or None where switched off); asserts that every guard,
        every input and every weight is bit-identical afterwards."""
        obs, a, Rn = self.inputs(obs, a, Rn)
        out = self.outputs(a.t.shape[0], kp, on)
        w, u = self.structs(obs, a, Rn, kp, out)
        inputs = [obs, a, Rn] + list(self.g.values())
        torch.cuda.synchronize()
        before = [g.bits.clone() for g in inputs]
        rc = self.launch(w, u)
        torch.cuda.synchronize()
        for g, was in zip(inputs, before):
            assert torch.equal(g.bits, was), "an input or a weight was written"
        for g in out:
            assert g is None or g.guards_intact(), "a guard of an output was overwritten"
        return (rc,) + tuple(g.host() if g is not None else None for g in out)


def _run(shape, w=None):
    A, Cn, E, support, _ = shape
    return Unroll(_case(shape)["w"] if w is None else w, A, Cn, E, support)


def _same(got, want, what):
    """values / prio on the float bits, codes as the integers they are"""
    got, want = (np.asarray(x) for x in (got, want))
    if want.dtype != np.int32:
        got, want = suref.bits(got), suref.bits(want)
    bad = np.argwhere(got != want)
    assert got.shape == want.shape and bad.size == 0, \
        f"{what}: {len(bad)} of {got.size} differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


# ---- 1. the C ABI against the oracle chain ----
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_values_priorities_and_codes_have_the_oracles_bits(shape):
    c, run = _case(shape), _run(shape)
    for B in BATCHES:
        for kp in STEPS:
            obs, a, Rn = c["obs"][:B], c["a"][:B], c["Rn"][:B]
            rc, v, p, codes = run(obs, a, Rn, kp)
            assert rc == _lib.MZS_OK, run.L.mzs_last_error(None)
            for got, want, name in ((v, c["v"], "values"), (p, c["p"], "prio"), (codes, c["c"], "codes")):
                _same(got, want[:B, :kp], (shape, B, kp, name))
            assert (codes[:, 0] == -1).all()
            rc, v2, p2, c2 = run(obs, a, Rn, kp)  # a second launch: the same bits
            assert rc == _lib.MZS_OK
            _same(v2, v, "second launch, values"), _same(p2, p, "second launch, prio"), _same(c2, codes, "second launch, codes")
    for off in range(3):  # each output NULL in turn
        on = tuple(i != off for i in range(3))
        rc, *got = run(c["obs"], c["a"], c["Rn"], L, on=on)
        assert rc == _lib.MZS_OK and got[off] is None
        for i, (want, name) in enumerate(((c["v"], "values"), (c["p"], "prio"), (c["c"], "codes"))):
            if i != off:
                _same(got[i], want, (shape, "without output", off, name))


@pytest.mark.parametrize("shape", [stref.SHAPES[0], (4, 33, 8, 8, 65)], ids=str)
def test_an_action_outside_the_range_is_the_all_zero_one_hot(oracle, shape):
    A, Cn, E, support, _ = shape
    c = _case(shape)
    a = c["a"].copy()
    a[1, 1], a[3, 0] = -1, A
    v, p, codes = suref.oracle_chain(oracle, c["w"], c["obs"], a, c["Rn"], A, Cn, E, support, L)
    rc, gv, gp, gc = _run(shape)(c["obs"], a, c["Rn"], L)
    assert rc == _lib.MZS_OK
    _same(gv, v, "values"), _same(gp, p, "prio"), _same(gc, codes, "codes")
    _same(gc, c["c"], "the codes do not depend on the actions")
    assert not np.array_equal(suref.bits(v[1, 2:]), suref.bits(c["v"][1, 2:]))
    assert not np.array_equal(suref.bits(v[3, 1:]), suref.bits(c["v"][3, 1:]))


# ---- 2. the argmax rule: the lowest index among equal maxima ----
def _with_encoder_bias(shape, bias):
    """The case's weights with en_w2 = 0, so that the logits ARE en_b2 = `bias` for every observation."""
    w = dict(_case(shape)["w"])
    w["en_w2"] = np.zeros_like(w["en_w2"])
    w["en_b2"] = np.asarray(bias, np.float32)
    return w


@pytest.mark.parametrize("shape,hot,want", [
    ((4, 17, 8, 8, 20), (2, 5), 2), ((4, 17, 8, 8, 20), (), 0),  # two equal maxima: the lower; all equal: 0
    ((4, 33, 8, 8, 65), (32,), 32), ((4, 60, 64, 31, 16), (59,), 59),  # the maximum in the last slot, C - 1
    ((4, 33, 8, 8, 65), (7, 32), 7), ((4, 60, 64, 31, 16), (0, 59), 0)])
def test_the_code_is_the_lowest_index_among_equal_maxima(oracle, shape, hot, want):
    A, Cn, E, support, _ = shape
    c = _case(shape)
    bias = np.full(Cn, 0.25, np.float32)
    bias[list(hot)] = 1.5
    w = _with_encoder_bias(shape, bias)
    v, p, codes = suref.oracle_chain(oracle, w, c["obs"], c["a"], c["Rn"], A, Cn, E, support, L)
    assert (codes[:, 1:] == want).all()  # (np.argmax: the first maximum)
    rc, gv, gp, gc = _run(shape, w)(c["obs"], c["a"], c["Rn"], L)
    assert rc == _lib.MZS_OK
    _same(gc, codes, "codes"), _same(gv, v, "values"), _same(gp, p, "prio")


# ---- 3. capturable ----
def test_a_captured_launch_replays_the_eager_bits():
    shape = stref.SHAPES[1]
    c, run = _case(shape), _run(shape)
    rc, v, p, codes = run(c["obs"], c["a"], c["Rn"], L)
    assert rc == _lib.MZS_OK
    obs, a, Rn = run.inputs(c["obs"], c["a"], c["Rn"])
    out = run.outputs(5, L)
    w, u = run.structs(obs, a, Rn, L, out)
    untouched = [g.bits.clone() for g in out]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with _call.capture(g):
        rc = run.launch(w, u)
    assert rc == _lib.MZS_OK, run.L.mzs_last_error(None)
    torch.cuda.synchronize()
    assert all(torch.equal(x.bits, was) for x, was in zip(out, untouched))  # captured, not run
    g.replay()
    torch.cuda.synchronize()
    assert all(x.guards_intact() for x in out)
    _same(out[0].host(), v, "values"), _same(out[1].host(), p, "prio"), _same(out[2].host(), codes, "codes")


# ---- 4. MuZero.unroll_values ----
def _device_batch(b, dev):
    return mx.Transition(obs=torch.as_tensor(np.asarray(b.obs, np.float32), device=dev),
                         a=torch.as_tensor(np.asarray(b.a, np.int32), device=dev), r=b.r,
                         Rn=torch.as_tensor(np.asarray(b.Rn, np.float32), device=dev), pi=b.pi)


def _oracle_of(oracle, m, b, shape, kp):
    A, Cn, E, support, _ = shape
    B_, L_ = np.asarray(b.a).shape[:2]
    return suref.oracle_chain(oracle, suref.model_weights(m), b.obs, np.asarray(b.a).reshape(B_, L_),
                              np.asarray(b.Rn, np.float32).reshape(B_, L_), A, Cn, E, support, kp)


def test_the_model_takes_the_kernel_route_and_follows_its_weights(oracle):
    shape = stref.SHAPES[1]
    A, Cn, E, support, od = shape
    m = stref.smz_model(A, Cn, E, support, od, seed=5, stochastic_unroll_values=True)
    assert m.device.type == "cuda" and m.unrolls_stochastic
    B_, L_ = 6, 5
    b = stref.smz_batch(B_, L_, A, od, seed=11)
    want_v, want_p, want_c = _oracle_of(oracle, m, b, shape, L_)
    v, p = m.unroll_values(b)
    assert v.shape == p.shape == (B_, L_) and v.dtype == p.dtype == torch.float32 and v.device == m.device
    _same(v.cpu().numpy(), want_v, "model, values"), _same(p.cpu().numpy(), want_p, "model, prio")
    fused = m._fused_unroll
    assert type(fused).__name__ == "StochasticFusedUnrollValues"
    _, _, codes = fused(b, L_, codes=True)
    _same(codes.cpu().numpy(), want_c, "model, codes")
    vh, ph = m.unroll_values(b, backend="hip")
    assert torch.equal(vh, v) and torch.equal(ph, p)
    vt, pt = m.unroll_values(b, backend="torch")
    worst = float((ph - pt).abs().max() / pt.max())
    print(f"[hip against torch: priorities within {worst:.2e} of the largest]", end=" ")
    # device tensors of the kernel's types pass through as they are; kp < L is the prefix
    dev_b = _device_batch(b, m.device)
    for kp in (1, 3):
        vk, pk = m.unroll_values(dev_b, k_prio=kp)
        assert torch.equal(vk, v[:, :kp]) and torch.equal(pk, p[:, :kp])
        obs_k, a_k, Rn_k, _ = fused._keep
        assert (obs_k.data_ptr(), a_k.data_ptr(), Rn_k.data_ptr()) == (dev_b.obs.data_ptr(), dev_b.a.data_ptr(), dev_b.Rn.data_ptr())
        assert torch.equal(mx.vector.unroll_value_priorities(m, dev_b, kp), p[:, :kp])
    with pytest.raises(ValueError, match="k_prio"):
        m.unroll_values(b, k_prio=L_ + 1)
    with pytest.raises(ValueError, match="needs every step's observation"):
        m.unroll_values(mx.Transition(**{**b.__dict__, "obs": np.asarray(b.obs)[:, :1]}))
    # the struct is kept between calls; an optimiser step (in place, or to new tensors) is followed
    kept = fused._w
    m.unroll_values(b)
    assert m._fused_unroll is fused and fused._w is kept
    m.update(b)
    want_v2, want_p2, _ = _oracle_of(oracle, m, b, shape, L_)
    v2, p2 = m.unroll_values(b)
    assert m._fused_unroll is fused and not torch.equal(v2, v)
    _same(v2.cpu().numpy(), want_v2, "after the step, values"), _same(p2.cpu().numpy(), want_p2, "after the step, prio")
    moved = [x.data_ptr() for x in fused.params] != [getattr(kept, n) for n in _lib.STOCHASTIC_TRAIN_WEIGHT_NAMES]
    assert (fused._w is not kept) == moved  # rebuilt exactly when a parameter tensor moved


def test_beyond_a_limit_hip_hands_on_the_librarys_refusal_and_auto_takes_torch():
    A, Cn, E, od = 3, 2, 4, 5
    b = stref.smz_batch(4, 3, A, od, seed=2)
    m = stref.smz_model(A, Cn, E, 7, od, seed=5, stochastic_unroll_values=True)
    with pytest.raises(ValueError, match="mzs_stochastic_mlp_unroll_values: support_size must be 8..31"):
        m.unroll_values(b, backend="hip")
    assert torch.equal(m.unroll_values(b)[0], m.unroll_values(b, backend="torch")[0])
    m = stref.smz_model(A, 62, E, 8, od, seed=5, stochastic_unroll_values=True)
    with pytest.raises(ValueError, match="num_actions . num_chance_outcomes must be <= 64"):
        m.unroll_values(b, backend="hip")
    assert torch.equal(m.unroll_values(b)[1], m.unroll_values(b, backend="torch")[1])
    off = stref.smz_model(A, Cn, E, 8, od, seed=5)
    with pytest.raises(NotImplementedError, match="not built for an SMZNetwork"):
        off.unroll_values(b)


# ---- 5. fit_vector ----
class _Recording(mx.DeviceReplayBuffer):
    """The device buffer, keeping the last batch it handed out and, of every update_priorities call, what it was given
    and the weights and live episodes it found."""
    calls = last = None

    @functools.wraps(mx.DeviceReplayBuffer.sample)  # (fit_vector reads the parameters: is_beta, all_obs)
    def sample(self, *a, **kw):
        got = super().sample(*a, **kw)
        self.last = got[0] if isinstance(got, tuple) else got
        return got

    def update_priorities(self, indices, priorities, **kw):
        before = {n: self._t[n].cpu().numpy().copy() for n in ("w", "cw", "t_w")}
        live = [(e.slot, e.start, e.length, e.serial) for e in self._eps]
        self.calls = (self.calls or []) + [(indices[0].clone(), indices[1].clone(), priorities.clone(), kw, before, live)]
        return super().update_priorities(indices, priorities, **kw)


def test_fit_vector_writes_the_kernels_priorities_back_for_a_stochastic_model():
    """The shape and sizes of tests/test_gpu_all_obs.py::_fit, with priority_steps=2."""
    A, Cn, E, support, od = stref.SHAPES[1]
    model = stref.smz_model(A, Cn, E, support, od, seed=5, policy="stochastic", stochastic_fused_update=True,
                            stochastic_unroll_values=True)
    buf, rows = _Recording(64, 4096, random_seed=13), []
    mx.fit_vector(model, mx.Device2048(8, max_episode_steps=6, seed=1, reward_shift=6),
                  mx.Device2048(2, max_episode_steps=5, seed=2, reward_shift=6), n_step=3, buffer=buf, iterations=2,
                  steps_per_iteration=6, num_simulations=4, k_steps=3, num_trajectory=8, sample_per_trajectory=2,
                  num_update_per_iteration=3, test_interval=10, random_seed=3, metrics=rows, device_collect=True,
                  device_plan=True, priority_update=True, priority_steps=2)
    assert len(rows) == 2 and all(np.isfinite(r["loss"]) for r in rows) and rows[-1]["training_step"] == 6
    assert len(buf.calls) == 6 and all(c[2].shape == (16, 2) and c[2].dtype == torch.float32 for c in buf.calls)
    assert all(c[3] == {"alpha": 0.5, "weight": "mean"} for c in buf.calls)
    assert type(model._fused_unroll).__name__ == "StochasticFusedUnrollValues"
    # the last batch: the model has not changed since its write-back, so unroll_values gives those priorities again
    serial, start, prio, _, before, live = buf.calls[-1]
    assert buf.last.obs.shape == (16, 3, od)
    v, p = model.unroll_values(buf.last, k_prio=2)
    assert torch.equal(p, prio) and torch.equal(p, (v - buf.last.Rn[:, :2]).abs())
    want_w, want_cw, want_tw, slots = pref.update(before["w"], before["cw"], before["t_w"], live, serial.cpu().numpy(),
                                                  start.cpu().numpy(), p.cpu().numpy(), 0.5, 0.0, "mean")
    assert slots
    got_w = buf._t["w"].cpu().numpy()
    changed = want_w != before["w"]
    assert changed.any() and np.array_equal(got_w[~changed], before["w"][~changed])
    # (|p| + eps) ** alpha in float64: the pow of the device and NumPy's may differ in the last places (1e-12 relative,
    # the bar of tests/test_gpu_priority.py for alpha != 1)
    assert (np.abs(got_w[changed] - want_w[changed]) <= 1e-12 * want_w[changed]).all()
