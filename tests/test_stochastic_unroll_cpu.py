"""CPU tests of the stochastic family's forward value unroll: the ABI rows and the host refusals of
mzs_stochastic_mlp_unroll_values, `MuZero(..., stochastic_unroll_values=True).unroll_values(backend="torch")` against the
chain composed from the C oracle (tests/stochastic_unroll_reference.py), the argument checks, and what
`fit_vector(priority_steps=)` asks of a stochastic model.  No GPU.

Bar: the trio's CPU bar, 2e-5 of the case's largest priority (tests/test_unroll_values_cpu.py).  Measured here on the three
shapes of stochastic_train_reference.SHAPES with B = 6, L = 5 (seed 1; every row well conditioned, none dropped): torch
float32 against the oracle chain 0, 0 and 4.9e-6 of the largest priority (values within 0, 0 and 2.6e-4 absolute), the
codes equal; torch float32 against the float64 copy of the same model 2.9e-6, 1.4e-6 and 3.7e-6 (values within 1.1e-4,
7.7e-5 and 2.0e-4).  The largest distance is a quarter of the trio's bar, which is kept as it is."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import muax_amd as mx
import stochastic_train_reference as stref
import stochastic_unroll_reference as suref
from muax_amd import _lib, unroll, vector

B, L = 6, 5
BAR = 2e-5
# one seed per shape of stref.SHAPES for which all B rows are well conditioned (checked below; no row may be dropped)
SEEDS = {stref.SHAPES[0]: 1, stref.SHAPES[1]: 1, stref.SHAPES[2]: 1}


def _model(shape, seed, on=True):
    A, Cn, E, support, od = shape
    return stref.smz_model(A, Cn, E, support, od, seed=seed, device="cpu", stochastic_unroll_values=on)


# ---- the ABI ----
def test_abi_declarations():
    """(The prototype, the member list and the layout against the header: tests/test_abi_cpu.py, for the whole ABI.)"""
    P, S = C.POINTER, _lib.MzsStochasticUnrollArgs
    assert _lib.ENTRIES["mzs_stochastic_mlp_unroll_values"] == (C.c_int, [P(_lib.MzsStochasticTrainWeights), P(S), C.c_void_p])
    assert _lib.STRUCTS["mzs_stochastic_unroll_args"] is S
    assert list(_lib.ENTRIES)[-1] == "mzs_stochastic_mlp_unroll_values" and list(_lib.STRUCTS)[-1] == "mzs_stochastic_unroll_args"
    assert [n for n, _ in S._fields_] == ["struct_size", "device", "batch", "row_steps", "k_prio", "num_actions",
                                          "num_chance_outcomes", "embed_dim", "obs", "actions", "returns", "values", "prio",
                                          "codes"]
    assert C.sizeof(S) == 8 * 4 + 6 * 8 and S.obs.offset == 32 and S.codes.offset == 72
    assert hasattr(_lib.load(), "mzs_stochastic_mlp_unroll_values")


REFUSED = [({"obs_dim": 129}, _lib.MZS_E_UNSUPPORTED, "obs_dim must be 1..128"),
           ({"obs_dim": 0}, _lib.MZS_E_UNSUPPORTED, "obs_dim must be 1..128"),
           ({"embed_dim": 65}, _lib.MZS_E_UNSUPPORTED, "embed_dim must be 1..64"),
           ({"embed_dim": 0}, _lib.MZS_E_UNSUPPORTED, "embed_dim must be 1..64"),
           ({"num_actions": 0}, _lib.MZS_E_UNSUPPORTED, "num_actions must be >= 1"),
           ({"num_chance_outcomes": 0}, _lib.MZS_E_UNSUPPORTED, "num_chance_outcomes must be >= 1"),
           ({"num_chance_outcomes": 63}, _lib.MZS_E_UNSUPPORTED, "num_actions + num_chance_outcomes must be <= 64"),
           ({"num_actions": 2 ** 31 - 1}, _lib.MZS_E_UNSUPPORTED, "num_actions + num_chance_outcomes must be <= 64"),
           ({"support_size": 7}, _lib.MZS_E_UNSUPPORTED, "support_size must be 8..31"),
           ({"support_size": 32}, _lib.MZS_E_UNSUPPORTED, "support_size must be 8..31"),
           ({"struct_size": C.sizeof(_lib.MzsStochasticUnrollArgs) - 8}, _lib.MZS_E_INVALID, "size mismatch"),
           ({"en_b2": None}, _lib.MZS_E_INVALID, "null weight pointer"),
           ({"repr_w": None}, _lib.MZS_E_INVALID, "null weight pointer"),
           ({"obs": None}, _lib.MZS_E_INVALID, "null obs, actions or returns"),
           ({"actions": None}, _lib.MZS_E_INVALID, "null obs, actions or returns"),
           ({"returns": None}, _lib.MZS_E_INVALID, "null obs, actions or returns"),
           ({"batch": 0}, _lib.MZS_E_INVALID, "batch must be >= 1"),
           ({"k_prio": 6}, _lib.MZS_E_INVALID, "k_prio must be in 1..row_steps"),
           ({"k_prio": 0}, _lib.MZS_E_INVALID, "k_prio must be in 1..row_steps"),
           ({"values": None, "prio": None, "codes": None}, _lib.MZS_E_INVALID, "at least one of values, prio and codes")]


def test_the_library_names_the_entry_and_the_limit_before_it_looks_for_a_device():
    """The host checks come before the device is selected, so they answer without one."""
    lib = _lib.load()
    weight_fields = {n for n, _ in _lib.MzsStochasticTrainWeights._fields_}
    for override, code, text in REFUSED:
        w = _lib.args(_lib.MzsStochasticTrainWeights, obs_dim=4, support_size=10,
                      **{n: 64 for n in _lib.STOCHASTIC_TRAIN_WEIGHT_NAMES})  # (never dereferenced on the host)
        u = _lib.args(_lib.MzsStochasticUnrollArgs, batch=3, row_steps=5, k_prio=5, num_actions=2, num_chance_outcomes=3,
                      embed_dim=8, obs=64, actions=64, returns=64, values=64, prio=64, codes=64)
        for k, x in override.items():
            setattr(w if k in weight_fields and k != "struct_size" else u, k, x)
        assert lib.mzs_stochastic_mlp_unroll_values(C.byref(w), C.byref(u), None) == code, override
        message = lib.mzs_last_error(None).decode()
        assert "mzs_stochastic_mlp_unroll_values" in message and text in message, (override, message)
    w = _lib.args(_lib.MzsStochasticTrainWeights, obs_dim=4, support_size=10)
    w.struct_size -= 8
    assert lib.mzs_stochastic_mlp_unroll_values(C.byref(w), None, None) == _lib.MZS_E_INVALID
    assert "size mismatch" in lib.mzs_last_error(None).decode()


def test_limits_of_the_python_side_are_the_headers():
    assert unroll.STOCHASTIC_LIMITS["obs_dim"] == (1, 128) and unroll.STOCHASTIC_LIMITS["embed_dim"] == (1, 64)
    assert unroll.STOCHASTIC_LIMITS["actions_and_outcomes"][1] == 64 and unroll.STOCHASTIC_LIMITS["support_size"] == (8, 31)
    assert unroll.within_stochastic_limits(_model(stref.SHAPES[0], 1))
    assert not unroll.within_stochastic_limits(stref.smz_model(4, 61, 8, 8, 5, seed=1, device="cpu"))  # A + C = 65
    assert not unroll.within_stochastic_limits(stref.smz_model(3, 2, 4, 7, 5, seed=1, device="cpu"))  # support 7


# ---- the torch route against the oracle chain ----
def _worst(got_p, got_v, want_p, want_v):
    """(priority error / largest priority, absolute value error)"""
    return float(np.abs(got_p - want_p).max() / want_p.max()), float(np.abs(got_v - want_v).max())


@pytest.mark.parametrize("shape", stref.SHAPES, ids=str)
def test_torch_backend_agrees_with_the_oracle_chain(oracle, shape):
    A, Cn, E, support, od = shape
    m = _model(shape, SEEDS[shape])
    b = stref.smz_batch(B, L, A, od, seed=SEEDS[shape] + 40)
    assert np.asarray(b.obs).shape == (B, L, od)
    cond = stref.conditions(m, b)
    assert stref.well_conditioned(cond), {k: float(v.min()) for k, v in cond.items() if v.size}  # every row, none dropped
    w = suref.model_weights(m)
    a, Rn = np.asarray(b.a).reshape(B, L), np.asarray(b.Rn, np.float32).reshape(B, L)
    want_v, want_p, want_c = suref.oracle_chain(oracle, w, b.obs, a, Rn, A, Cn, E, support, L)
    v, p = m.unroll_values(b, backend="torch")
    assert v.shape == p.shape == (B, L) and v.dtype == p.dtype == torch.float32 and v.device == m.device
    _, _, codes = unroll.torch_stochastic_unroll_values(m, b, L, with_codes=True)
    assert codes.dtype == torch.int32 and np.array_equal(codes.numpy(), want_c) and (want_c[:, 0] == -1).all()
    assert (want_c[:, 1:] >= 0).all() and (want_c[:, 1:] < Cn).all()
    rel, dv = _worst(p.numpy(), v.numpy(), want_p, want_v)
    m64 = stref.copy_model(m)  # (float64 modules: the torch route evaluates and returns float64)
    m64.stochastic_unroll_values = True
    v64, p64 = m64.unroll_values(b, backend="torch")
    assert v64.dtype == torch.float64
    rel64, dv64 = _worst(p.numpy(), v.numpy(), p64.numpy(), v64.numpy())
    print(f"[{shape}: torch fp32 against the oracle chain: priorities within {rel:.2e} of the largest, v within {dv:.2e} "
          f"absolute; against the float64 copy: {rel64:.2e}, {dv64:.2e}]", end=" ")
    assert rel <= BAR
    # "auto" on a CPU model is the torch route; the priorities alone are vector.unroll_value_priorities
    va, pa = m.unroll_values(b)
    assert torch.equal(va, v) and torch.equal(pa, p)
    assert torch.equal(vector.unroll_value_priorities(m, b, backend="torch"), p)
    # kp < L: the prefix of the full unroll; kp = L names the default
    for kp in (1, 3, L):
        vk, pk = m.unroll_values(b, k_prio=kp, backend="torch")
        assert vk.shape == (B, kp) and torch.equal(vk, v[:, :kp]) and torch.equal(pk, p[:, :kp])
        assert torch.equal(vector.unroll_value_priorities(m, b, kp), p[:, :kp])
    # the first column is what value_priorities gives
    assert torch.equal(vector.value_priorities(m, b), p[:, 0])


def test_the_oracle_chain_is_a_chain_and_its_zero_row_net_is_the_zero_one_hot(oracle):
    A, Cn, E, support, od = stref.SHAPES[0]
    c = suref.make_case(A, Cn, E, support, od, 5, 4)
    v, p, codes = suref.oracle_chain(oracle, c["w"], c["obs"], c["a"], c["Rn"], A, Cn, E, support, 4)
    v2, p2, c2 = suref.oracle_chain(oracle, c["w"], c["obs"], c["a"], c["Rn"], A, Cn, E, support, 2)
    assert np.array_equal(suref.bits(v2), suref.bits(v[:, :2])) and np.array_equal(suref.bits(p2), suref.bits(p[:, :2]))
    assert np.array_equal(c2, codes[:, :2])
    a = c["a"].copy()
    a[1, 1], a[3, 1] = -1, A
    vz, _, cz = suref.oracle_chain(oracle, c["w"], c["obs"], a, c["Rn"], A, Cn, E, support, 4)
    rows = np.array([0, 2, 4])
    assert np.array_equal(suref.bits(vz[rows]), suref.bits(v[rows]))  # the widened net changes no other row's bits
    assert np.array_equal(suref.bits(vz[:, :2]), suref.bits(v[:, :2])) and np.array_equal(cz, codes)
    assert not np.array_equal(suref.bits(vz[[1, 3], 2:]), suref.bits(v[[1, 3], 2:]))
    # the oracle compares the action with every index, so -1 handed over as it is gives the same all-zero one-hot
    after = suref.smref._trio(oracle, c["w"], None, "ad", None, None, E, A, support, 0.99, 0)
    wide = dict(c["w"], ad_w1=np.concatenate([c["w"]["ad_w1"], np.zeros((1, 16), np.float32)], 0))
    after_wide = suref.smref._trio(oracle, wide, None, "ad", None, None, E, A + 1, support, 0.99, 0)
    s = np.random.default_rng(0).uniform(0, 1, (3, E)).astype(np.float32)
    plain = oracle.recurrent_inference(after, np.full(3, -1), s)[4]
    assert np.array_equal(suref.bits(plain), suref.bits(oracle.recurrent_inference(after_wide, np.full(3, A), s)[4]))


def test_arguments_are_checked_before_anything_runs(monkeypatch):
    shape = stref.SHAPES[0]
    A, _, _, _, od = shape
    m = _model(shape, 1)
    b = stref.smz_batch(B, L, A, od, seed=3)

    def never(*a, **k):
        raise AssertionError("the network was evaluated")
    monkeypatch.setattr(m, "network", mx.nn.SMZNetwork(*([never] * 6)))
    for kp in (L + 1, 0, -1):
        with pytest.raises(ValueError, match="k_prio"):
            m.unroll_values(b, k_prio=kp, backend="torch")
        with pytest.raises(ValueError, match="k_prio"):
            vector.unroll_value_priorities(m, b, kp)
    with pytest.raises(ValueError, match="backend"):
        m.unroll_values(b, backend="triton")
    with pytest.raises(ValueError, match="GPU"):  # a CPU model: no kernel, and no quiet fall-back
        m.unroll_values(b, backend="hip")
    # one observation per window (the default of DeviceReplayBuffer.sample), or a 2-D obs: the loss's refusal
    flat = mx.Transition(**{**b.__dict__, "obs": np.asarray(b.obs)[:, 0]})
    one = mx.Transition(**{**b.__dict__, "obs": np.asarray(b.obs)[:, :1]})
    for bad in (flat, one):
        for backend in ("auto", "torch"):
            with pytest.raises(ValueError, match="needs every step's observation"):
                m.unroll_values(bad, backend=backend)


# ---- the flag ----
def test_flag_off_is_the_refusal_as_it_was():
    shape = stref.SHAPES[0]
    m = _model(shape, 1, on=False)
    assert m.trains_stochastic and m.stochastic_unroll_values is False and m.unrolls_stochastic is False
    assert _model(shape, 1).unrolls_stochastic is True
    b = stref.smz_batch(B, L, shape[0], shape[4], seed=3)
    for backend in ("auto", "torch", "hip"):
        with pytest.raises(NotImplementedError, match="not built for an SMZNetwork .its unroll needs every step's chance code."):
            m.unroll_values(b, backend=backend)
    with pytest.raises(ValueError, match="priority_steps needs MuZero.unroll_values, which is not built for an SMZNetwork"):
        mx.fit_vector(m, None, None, buffer=_Buffer(50, random_seed=4), priority_update=True, priority_steps=2)
    # a deterministic model has no stochastic unroll, flag or not
    g = torch.Generator().manual_seed(0)
    mz = mx.MuZero(mx.nn.MZNetwork(mx.nn.Representation(8, generator=g), mx.nn.Prediction(2, 21, generator=g),
                                   mx.nn.Dynamic(8, 2, 21, generator=g)), device="cpu", stochastic_unroll_values=True)
    assert mz.unrolls_stochastic is False


class _VecEnv:
    """Four environments with fixed episode lengths; observation = (env id, step)."""
    lengths = (5, 7, 6, 9)
    spec = SimpleNamespace(max_episode_steps=10)

    def reset(self):
        self.t = [0] * 4
        return np.array([[e, 0] for e in range(4)], np.float32)

    def step(self, actions):
        d = np.zeros(4, bool)
        for e in range(4):
            self.t[e] += 1
            if self.t[e] == self.lengths[e]:
                d[e], self.t[e] = True, 0
        return np.array([[e, self.t[e]] for e in range(4)], np.float32), 1.0 + np.asarray(actions, np.float64), d


class _Fake:
    """A model that trains stochastically; `unrolls`: whether it exposes `unrolls_stochastic` (None: not at all)."""
    device, _support_size, trains_stochastic = torch.device("cpu"), 10, True

    def __init__(self, unrolls):
        if unrolls is not None:
            self.unrolls_stochastic = unrolls
        self.unrolled = []

    def init(self, key, sample):
        pass

    def act(self, key, obs, with_pi=False, with_value=False, **kw):
        obs = np.asarray(obs, np.float32)
        a = (obs.sum(1) % 2).astype(np.int64)
        pi = np.stack([a == 0, a == 1], 1).astype(np.float32)
        return (a, pi, obs.sum(1).astype(np.float64)) if with_pi else a

    def update(self, batch):
        return {"loss": float(np.sum(batch.Rn))}

    def unroll_values(self, batch, k_prio=None, backend="auto"):
        Bn = np.asarray(batch.Rn).shape[0]
        self.unrolled.append((np.asarray(batch.obs).shape, k_prio))
        p = torch.full((Bn, k_prio), 0.5)
        return p, p


class _Buffer(mx.TrajectoryReplayBuffer):
    """The host buffer with the device buffer's `all_obs` parameter and write-back, recording what it is given."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.asked, self.written = [], []

    def sample(self, *a, with_indices=False, all_obs=False, **kw):
        self.asked.append(all_obs)
        batch = super().sample(*a, **kw)
        Bn = np.asarray(batch.Rn).shape[0]
        return (batch, (np.arange(Bn), np.zeros(Bn, np.int32))) if with_indices else batch

    def update_priorities(self, indices, priorities, alpha=1.0, eps=0.0, weight="mean"):
        self.written.append(tuple(priorities.shape))


def _fit(model, buffer, **kw):
    mx.fit_vector(model, _VecEnv(), _VecEnv(), n_step=2, gamma=0.9, buffer=buffer, iterations=2, steps_per_iteration=10,
                  num_simulations=2, k_steps=3, num_trajectory=4, num_update_per_iteration=3, test_interval=10,
                  random_seed=1, **kw)


def test_fit_vector_takes_priority_steps_from_a_model_that_unrolls_stochastically():
    model, buf = _Fake(True), _Buffer(50, random_seed=4)
    _fit(model, buf, priority_update=True, priority_steps=2)
    assert buf.asked == [True] * 6 and buf.written == [(4, 2)] * 6  # every observation asked for, [B, kp] written back
    assert [kp for _, kp in model.unrolled] == [2] * 6 and all(len(s) == 3 and s[1] == 3 for s, _ in model.unrolled)
    # without the property, or with it False, the refusal stands, before anything is sampled
    for unrolls in (None, False):
        buf = _Buffer(50, random_seed=4)
        with pytest.raises(ValueError, match="priority_steps.*SMZNetwork"):
            _fit(_Fake(unrolls), buf, priority_update=True, priority_steps=2)
        assert buf.asked == []
