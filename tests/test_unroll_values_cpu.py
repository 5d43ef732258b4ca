"""CPU tests of the forward value unroll: the reference the GPU kernel is held to bit for bit
(unroll_reference.oracle_chain: the C oracle's root_inference / recurrent_inference chain) against an independent
float64 restatement (unroll_reference.fp64_chain, from oracle/mz_train_numpy.py), `MuZero.unroll_values(backend="torch")`
against the same restatement, the argument checks made before anything runs, the ABI declarations and
`fit_vector(priority_steps=)`.  No GPU.

Bar: 2e-5 of the case's largest priority.  The float32 chain (two to six layers of k-ordered fma sums, two normalisers,
a softmax and the decode, whose inverse-h amplifies an error of the expectation by up to 2 sqrt(|v| + 1) + ...) was
measured at 2.5e-6 of the largest priority on these cases (|v| up to 5.0, v within 1.5e-4 absolute; 2.7e-6 and 1.6e-4
with |v| up to 6.1 on other seeds); the bar is about eight times that."""
import ctypes as C

import numpy as np
import pytest
import torch

import muax_amd as mx
import unroll_reference as uref
from helpers import set_trio, train_model
from muax_amd import _build, _lib, vector

SHAPES = [(1, 15, 8, 1), (16, 1, 16, 17), (15, 17, 24, 128), (2, 8, 10, 4), (64, 64, 31, 16), (17, 33, 8, 17), (64, 1, 10, 1)]
B, L = 37, 5
BAR = 2e-5


def _worst(got_p, got_v, want_p, want_v):
    """(priority error / largest priority, absolute value error)"""
    return float(np.abs(got_p - want_p).max() / want_p.max()), float(np.abs(got_v - want_v).max())


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_oracle_chain_agrees_with_the_fp64_restatement(oracle, shape):
    A, E, support, obs_dim = shape
    c = uref.make_case(oracle, A, E, support, obs_dim, B, L)
    v, p = uref.oracle_chain(oracle, c["w"], c["obs"], c["a"], c["Rn"], support, L)
    v64, p64 = uref.fp64_chain(c["w"], c["obs"], c["a"], c["Rn"], support, L)
    assert v.shape == p.shape == (B, L) and v.dtype == p.dtype == np.float32
    rel, dv = _worst(p, v, p64, v64)
    print(f"[{shape}: priorities within {rel:.2e} of the largest, v within {dv:.2e} absolute, |v| up to {np.abs(v64).max():.2f}]", end=" ")
    assert rel <= BAR
    # the chain is a chain: its first column is root inference alone, and a shorter unroll is its prefix
    v2, p2 = uref.oracle_chain(oracle, c["w"], c["obs"], c["a"], c["Rn"], support, 2)
    assert np.array_equal(uref.bits(v2), uref.bits(v[:, :2])) and np.array_equal(uref.bits(p2), uref.bits(p[:, :2]))


def test_the_zero_row_net_is_the_all_zero_one_hot(oracle):
    """The out-of-range construction on the fp64 side: action A of the widened net gives what a zero one-hot gives."""
    A, E, support, obs_dim = 2, 8, 10, 4
    c = uref.make_case(oracle, A, E, support, obs_dim, 5, 4)
    a = c["a"].copy()
    a[1, 1], a[3, 1] = -1, A
    v, _ = uref.oracle_chain(oracle, c["w"], c["obs"], a, c["Rn"], support, 4)
    good, _ = uref.oracle_chain(oracle, c["w"], c["obs"], c["a"], c["Rn"], support, 4)
    rows = np.array([0, 2, 4])
    assert np.array_equal(uref.bits(v[rows]), uref.bits(good[rows]))  # the widened net changes no other row's bits
    assert np.array_equal(uref.bits(v[:, :2]), uref.bits(good[:, :2]))  # nor anything before the action is consumed
    from oracle import mz_train_numpy as ref
    w64 = {k: np.asarray(x, np.float64) for k, x in c["w"].items()}
    tr = {}
    ref.forward(w64, c["obs"], c["a"][:, :2], np.zeros((5, 2)), np.zeros((5, 2)), np.full((5, 2, A), 0.5), support, trace=tr)
    for row in (1, 3):  # fp64, by hand: the dynamics' hidden layer on s_1 with no one-hot row added at all
        s1 = tr["states"][1][row:row + 1]
        h = ref._elu(s1 @ w64["dn_w1"][:E] + w64["dn_b1"])
        s2 = ref._minmax(h @ w64["dn_w2"] + w64["dn_b2"])[0]
        lg, _ = ref._mlp(w64, "pv", s2)
        e = np.exp(lg - lg.max())
        want = float(uref._inv_h(((e / e.sum()) @ np.arange(-support, support + 1))[0]))
        assert abs(float(v[row, 2]) - want) <= BAR * 60, (row, v[row, 2], want)  # (the bar at the returns' range)


def _cpu_model(c):
    m = train_model(c["A"], c["E"], c["obs_dim"], seed=1, support=c["support"], device="cpu")
    set_trio(m, **c["w"])
    return m


def _batch(c, L_obs=None):
    B_, L_ = c["a"].shape
    obs = np.repeat(c["obs"][:, None], L_obs or L_, 1)
    obs[:, 1:] += 100.0  # only obs[:, 0] may be read
    return mx.Transition(obs=obs, a=c["a"], r=np.zeros((B_, L_), np.float32), Rn=c["Rn"],
                         pi=np.full((B_, L_, 1, c["A"]), 1.0 / c["A"], np.float32))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_torch_backend_agrees_with_the_fp64_restatement(oracle, shape):
    A, E, support, obs_dim = shape
    c = uref.make_case(oracle, A, E, support, obs_dim, B, L)
    m, b = _cpu_model(c), _batch(c)
    v, p = m.unroll_values(b, backend="torch")
    assert v.shape == p.shape == (B, L) and v.dtype == p.dtype == torch.float32 and v.device == m.device
    v64, p64 = uref.fp64_chain(c["w"], c["obs"], c["a"], c["Rn"], support, L)
    rel, dv = _worst(p.numpy(), v.numpy(), p64, v64)
    print(f"[{shape}: priorities within {rel:.2e} of the largest, v within {dv:.2e} absolute]", end=" ")
    assert rel <= BAR
    # "auto" on a CPU model is the torch route; the priorities alone are vector.unroll_value_priorities
    va, pa = m.unroll_values(b)
    assert torch.equal(va, v) and torch.equal(pa, p)
    assert torch.equal(vector.unroll_value_priorities(m, b, backend="torch"), p)
    # kp < L reads a, Rn with the row stride L: the prefix of the full unroll
    for kp in (1, 3):
        vk, pk = m.unroll_values(b, k_prio=kp, backend="torch")
        assert vk.shape == (B, kp) and torch.equal(vk, v[:, :kp]) and torch.equal(pk, p[:, :kp])
        assert torch.equal(vector.unroll_value_priorities(m, b, kp), p[:, :kp])
    # the first column is what value_priorities gives
    assert torch.equal(vector.value_priorities(m, b), p[:, 0])


def test_arguments_are_checked_before_anything_runs(oracle, monkeypatch):
    c = uref.make_case(oracle, 2, 8, 10, 4, 6, 5)
    m, b = _cpu_model(c), _batch(c)

    def never(*a, **k):
        raise AssertionError("the network was evaluated")
    monkeypatch.setattr(m, "repr_func", never)
    for kp in (6, 0, -1):
        with pytest.raises(ValueError, match="k_prio"):
            m.unroll_values(b, k_prio=kp, backend="torch")
        with pytest.raises(ValueError, match="k_prio"):
            vector.unroll_value_priorities(m, b, kp)
    with pytest.raises(ValueError, match="backend"):
        m.unroll_values(b, backend="triton")
    with pytest.raises(ValueError, match="GPU"):  # a CPU model: no kernel, and no quiet fall-back
        m.unroll_values(b, backend="hip")


def test_abi_declarations():
    """(The prototype, the member list and the layout against the header: tests/test_abi_cpu.py, for the whole ABI.)"""
    P = C.POINTER
    assert _lib.ENTRIES["mzs_mlp_unroll_values"] == (C.c_int, [P(_lib.MzsMlpWeights), P(_lib.MzsUnrollArgs), C.c_void_p])
    assert "mz_unroll.hip" in _build.UNITS and {"mz_unroll.cuh", "mz_mlp_generic.cuh"} <= set(_build.UNITS["mz_unroll.hip"])
    assert "mz_unroll.hip" not in _build.UNIT_FLAGS and "-ffp-contract=off" in _build.FLAGS  # built as mz_stepwise.hip is
    assert C.sizeof(_lib.MzsUnrollArgs) == 8 * 4 + 5 * 8
    assert _lib.MzsUnrollArgs.obs.offset == 32 and _lib.MzsUnrollArgs.prio.offset == 64


def test_fit_vector_rejects_priority_steps_below_one():
    for bad in (0, -2):
        with pytest.raises(ValueError, match="priority_steps"):
            mx.fit_vector(None, None, None, priority_update=True, priority_steps=bad)
        with pytest.raises(ValueError, match="priority_steps"):
            mx.fit_vector(None, None, None, priority_steps=bad)


def test_the_library_names_the_limit_before_it_looks_for_a_device():
    """The host checks of mzs_mlp_unroll_values come before the device is selected, so they answer without one."""
    lib = _lib.load()
    w = _lib.MzsMlpWeights()
    w.struct_size = C.sizeof(_lib.MzsMlpWeights)
    for n in _lib.MLP_WEIGHT_NAMES:
        setattr(w, n, 64)  # (never dereferenced on the host)
    cases = [({"obs_dim": 129}, _lib.MZS_E_UNSUPPORTED, "obs_dim must be 1..128"),
             ({"embed_dim": 65}, _lib.MZS_E_UNSUPPORTED, "embed_dim must be 1..64"),
             ({"num_actions": 65}, _lib.MZS_E_UNSUPPORTED, "num_actions must be 1..64"),
             ({"support_size": 7}, _lib.MZS_E_UNSUPPORTED, "support_size must be 8..31"),
             ({"support_size": 32}, _lib.MZS_E_UNSUPPORTED, "support_size must be 8..31"),
             ({"k_prio": 6}, _lib.MZS_E_INVALID, "k_prio must be in 1..row_steps"),
             ({"batch": 0}, _lib.MZS_E_INVALID, "batch must be >= 1"),
             ({"values": None, "prio": None}, _lib.MZS_E_INVALID, "at least one of values and prio"),
             ({"returns": None}, _lib.MZS_E_INVALID, "null obs, actions or returns")]
    for override, code, text in cases:
        u = _lib.MzsUnrollArgs()
        u.struct_size = C.sizeof(_lib.MzsUnrollArgs)
        u.batch, u.row_steps, u.k_prio, u.num_actions, u.embed_dim = 3, 5, 5, 2, 8
        u.obs = u.actions = u.returns = u.values = u.prio = 64
        w.obs_dim, w.support_size = 4, 10
        for k, x in override.items():
            setattr(w if k in ("obs_dim", "support_size") else u, k, x)
        assert lib.mzs_mlp_unroll_values(C.byref(w), C.byref(u), None) == code, override
        assert text in lib.mzs_last_error(None).decode(), override
