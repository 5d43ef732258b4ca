"""CPU tests of the importance-sampling weights of prioritised replay: the plain-loop reference the GPU tests compare
the kernels with (tests/isweight_reference.py) on small buffers, the ABI declarations, the checks `sample(is_beta=)`
makes before it touches the device, `default_loss_fn(sample_weight=)` in float64 against the independent NumPy
reference of the training step, and `fit_vector(is_beta=)`.  No GPU, no kernel."""
import copy
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import isweight_reference as isref
import muax_amd as mx
import replay_reference as rr
from helpers import train_batch, train_model, trio_arrays
from muax_amd import _lib
from muax_amd._lib import MLP_WEIGHT_NAMES
from oracle import mz_train_numpy as oracle_train

# (lengths, k): the 3-step episode is ineligible, the 5-step one has m = 1; then two episodes of one window each
BUFFERS = [((3, 7, 12, 5), 4), ((9, 9), 8)]


def _episodes(lengths, seed, zero_frac=0.0, obs_dim=3, A=2):
    rng = np.random.default_rng(seed)
    return [rr.make_episode(rng, T, A, obs_dim, w=rr.dyadic_weights(rng, T, zero_frac) + (0.0 if zero_frac else 2.0 ** -10))
            for T in lengths]


def _windows(eps, k):
    return [(e, s) for e, ep in enumerate(eps) if len(ep["w"]) > k for s in range(len(ep["w"]) - k)]


# ---- the reference on small buffers ----
@pytest.mark.parametrize("lengths,k", BUFFERS)
def test_window_probabilities_sum_to_one_over_the_eligible_windows(lengths, k):
    """An N or a total that counts the ineligible 3-step episode (its buffer weight is positive) breaks both."""
    eps = _episodes(lengths, seed=k)
    assert all(ep["weight"] > 0 for ep in eps)
    wins = _windows(eps, k)
    assert len(wins) == isref.eligible_windows(lengths, k) == sum(T - k for T in lengths if T > k)
    assert isref.eligible_windows(lengths, k) == {4: 12, 8: 2}[k]
    q = [isref.window_probability(eps, e, s, k) for e, s in wins]
    assert abs(sum(q) - 1.0) <= 1e-12 and min(q) > 0
    # uniform weights: every window equally likely, every raw weight exactly 1
    for ep in eps:
        ep["w"] = np.ones_like(ep["w"])
        ep["weight"] = float(max(len(ep["w"]) - k, 0)) or 1.0
    N = isref.eligible_windows(lengths, k)
    for e, s in wins:
        assert isref.raw_weight(N, isref.window_probability(eps, e, s, k), 1.0) == pytest.approx(1.0, abs=1e-15)


def test_eligible_windows_follows_the_evictions_of_the_buffer():
    """DeviceReplayBuffer's own count (host bookkeeping) against the arena model, through wrap-around evictions."""
    b, model = mx.DeviceReplayBuffer(5, 60, random_seed=0), rr.ArenaModel(5, 60)
    rng = np.random.default_rng(3)
    for T in rng.integers(2, 25, 40):
        b._place(int(T))
        model.add(int(T))
        assert b.serials == model.serials
        for k in (1, 4, 10, 30):
            assert b.eligible_windows(k) == isref.eligible_windows([n for _, _, n in model.live], k)
    assert b._arena is None


@pytest.mark.parametrize("lengths,k", BUFFERS)
@pytest.mark.parametrize("spt", [1, 3])
def test_beta_zero_gives_ones_and_normalised_weights_lie_in_unit_interval(lengths, k, spt):
    eps = _episodes(lengths, seed=10 + k)
    key, B = [5, k], 67
    for normalize in (False, True):
        got = isref.weights(key, eps, B, k, spt, beta=0.0, normalize=normalize)
        assert (got["isw"] == 1.0).all() and (got["raw"] == 1.0).all()
    # over EVERY eligible window (dyadic weights without ties): one largest weight, and it is the 1
    wins = _windows(eps, k)
    N = isref.eligible_windows(lengths, k)
    for beta in (1.0, 0.4):
        raw = np.array([isref.raw_weight(N, isref.window_probability(eps, e, s, k), beta) for e, s in wins])
        assert len(np.unique(raw)) == len(raw)
        norm = raw / raw.max()
        assert (norm > 0).all() and (norm <= 1.0).all() and int((norm == 1.0).sum()) == 1
        # ... and in a batch: the maximum is exactly 1, reached by the rows of ONE window only (a min in the
        # normaliser's place gives weights above 1)
        got = isref.weights(key, eps, B, k, spt, beta=beta, normalize=True)
        isw = got["isw"]
        assert isw.dtype == np.float32 and (isw > 0).all() and (isw <= 1.0).all() and isw.max() == 1.0
        top = {(int(e), int(s)) for e, s, w in zip(got["e"], got["start"], isw) if w == 1.0}
        assert len(top) == 1
        assert np.array_equal(isw, (got["raw"] / got["raw"].max()).astype(np.float32))
        # the rows of one window carry one weight, whatever shares their episode (sample_per_trajectory = 3)
        by_window = {}
        for e, s, w in zip(got["e"], got["start"], isw):
            assert by_window.setdefault((int(e), int(s)), w) == w
        raw_b = isref.weights(key, eps, B, k, spt, beta=beta, normalize=False)
        assert np.array_equal(raw_b["isw"], got["raw"].astype(np.float32)) and np.array_equal(raw_b["e"], got["e"])


def test_zero_weight_transition_is_never_a_drawn_start():
    lengths, k = (3, 7, 12, 5), 4
    eps = _episodes(lengths, seed=2, zero_frac=0.4)
    eps[2]["w"][:3] = [0.0, 5.0, 0.0]
    eps[1]["w"][:3] = [1.0, 0.0, 2.0]   # (the possible starts of a 7-step episode with k = 4)
    eps[3]["w"][0] = 3.0
    zero_starts = sum(int(ep["w"][s] == 0) for e, ep in enumerate(eps) if len(ep["w"]) > k
                      for s in range(len(ep["w"]) - k))
    assert zero_starts >= 3
    seen = set()
    for seed in range(6):
        got = isref.weights([seed, 1], eps, 67, k, 1, beta=1.0, normalize=False)
        for e, s, q, raw in zip(got["e"], got["start"], got["q"], got["raw"]):
            assert eps[e]["w"][s] > 0 and q > 0 and np.isfinite(raw)
            seen.add((int(e), int(s)))
    assert 4 <= len(seen) <= isref.eligible_windows(lengths, k) - zero_starts  # (positive starts only)


def test_all_zero_transition_weights_draw_the_start_uniformly():
    """An episode whose transition weights are all zero but whose buffer weight is positive: p_s = 1 / m."""
    lengths, k = (3, 7, 12, 5), 4
    eps = _episodes(lengths, seed=4)
    eps[2]["w"] = np.zeros(12)
    m = 12 - k
    for s in range(m):
        assert isref.start_probability(eps[2]["w"], s, k) == 1.0 / m
    assert abs(sum(isref.window_probability(eps, e, s, k) for e, s in _windows(eps, k)) - 1.0) <= 1e-12
    key = [8, 8]
    got = isref.weights(key, eps, 67, k, 1, beta=1.0, normalize=False)
    _, u1 = rr.draws(key, 67)
    on = got["e"] == 2
    assert on.sum() >= 5 and np.array_equal(got["start"][on], np.floor(u1[on] * m).astype(int))
    p_e = isref.episode_probability(eps, 2, k)
    assert np.array_equal(got["raw"][on], np.full(on.sum(), 1.0 / (12 * (p_e * (1.0 / m)))))


def test_every_buffer_weight_zero():
    """The draw is deterministic (the newest episode): p_e = 1; a newest episode no longer than k gives zero rows."""
    eps = _episodes((9, 9), seed=6)
    for ep in eps:
        ep["weight"] = 0.0
    got = isref.weights([1, 2], eps, 19, 8, 1, beta=1.0, normalize=False)
    assert (got["e"] == 1).all() and (got["start"] == 0).all() and np.array_equal(got["raw"], np.full(19, 0.5))
    eps = _episodes((9, 5), seed=6)
    for ep in eps:
        ep["weight"] = 0.0
    for normalize in (False, True):
        got = isref.weights([1, 2], eps, 19, 8, 1, beta=0.4, normalize=normalize)
        assert (got["start"] == -1).all() and not got["isw"].any() and not got["raw"].any()


# ---- the ABI ----
def test_header_and_bindings_agree_on_the_new_entries():
    """(Declarations, member lists, sizes and offsets: tests/test_abi_cpu.py, for the whole ABI.)"""
    # as before this entry existed
    assert ctypes.sizeof(_lib.MzsReplaySampleArgs) == 112 and ctypes.sizeof(_lib.MzsTrainArgs) == 104
    lib = _lib.load(build_if_missing=True)
    for s in ("mzs_replay_sample_is", "mzs_mlp_loss_grad_weighted"):
        assert getattr(lib, s)(None, None, None, None) == _lib.MZS_E_INVALID  # null blocks are refused before any device call
    assert lib.mzs_abi_version() == 1


def test_sample_checks_is_beta_before_any_device_use():
    b = mx.DeviceReplayBuffer(4, 100, random_seed=0)
    for bad in (-0.1, 1.5, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="is_beta"):
            b.sample(4, k_steps=3, is_beta=bad)
    b._place(10)
    key = copy.deepcopy(b._key)
    for bad in (-1e-9, 1.0 + 1e-9, float("nan")):
        with pytest.raises(ValueError, match="is_beta"):
            b.sample(4, k_steps=3, is_beta=bad, is_normalize=False, with_indices=True)
    with pytest.raises((TypeError, ValueError)):
        b.sample(4, k_steps=3, is_beta="half")
    assert b._arena is None and b._is_scratch is None and np.array_equal(np.asarray(b._key), np.asarray(key))
    with pytest.raises(ValueError, match="empty"):
        mx.DeviceReplayBuffer(4, 100).sample(4, k_steps=3, is_beta=0.5)


# ---- the torch loss ----
A_, E_, SUPPORT, OBS_DIM, B_, L_ = 2, 8, 10, 4, 5, 3


def _fp64_model(seed):
    m = train_model(A_, E_, OBS_DIM, seed=seed, support=SUPPORT, device="cpu")
    mods = [copy.deepcopy(x).to(dtype=torch.float64) for x in m.network]
    m64 = mx.MuZero(mx.nn.MZNetwork(*mods), device="cpu")
    m64._params, m64._support_size = True, SUPPORT
    return m, m64


def _loss_and_grads(m64, b, **kw):
    for p in mx.nn.mlp_trio_weights(m64.network).values():
        p.grad = None
    loss = mx.loss.default_loss_fn(m64, b, **kw)
    assert loss.dtype == torch.float64
    loss.backward()
    w = mx.nn.mlp_trio_weights(m64.network)
    return loss.detach(), [w[n].grad.detach().clone() for n in MLP_WEIGHT_NAMES]


@pytest.mark.parametrize("divide_by_length", [False, True])
def test_weighted_loss_is_the_linear_combination_of_the_single_row_losses(divide_by_length):
    """default_loss_fn(sample_weight=) in float64 against oracle/mz_train_numpy.py row by row:
        loss = sum_b sw_b / B * (loss_b - l2) + l2,    grad = sum_b sw_b / B * (grad_b - 1e-4 w) + 1e-4 w
    (loss_b, grad_b: the oracle on row b alone, whose mean is over one row).  Bars: those of the fp64 autograd against
    the oracle in tests/test_train_reference_cpu.py -- 1e-12 relative on the loss, 1e-9 of an array's largest entry.
    A weight on the loss alone, or on the L2 term as well, misses both."""
    m, m64 = _fp64_model(seed=21)
    b = train_batch(B_, L_, A_, OBS_DIM, seed=21)
    sw = np.array([0.25, 1.0, 0.0, 0.618, 0.875])
    w = trio_arrays(m)
    l2 = 1e-4 * 0.5 * sum(float((w[n].astype(np.float64) ** 2).sum()) for n in MLP_WEIGHT_NAMES)
    want_l, want_g = l2, {n: 1e-4 * w[n].astype(np.float64) for n in MLP_WEIGHT_NAMES}
    for i in range(B_):
        row = slice(i, i + 1)
        l_b, g_b = oracle_train.loss_and_grads(w, b.obs[row, 0], b.a[row], b.r[row], b.Rn[row], b.pi[row], SUPPORT,
                                               divide_by_length=divide_by_length)
        want_l += sw[i] / B_ * (l_b - l2)
        for n in MLP_WEIGHT_NAMES:
            want_g[n] += sw[i] / B_ * (g_b[n] - 1e-4 * w[n].astype(np.float64))
    got_l, got_g = _loss_and_grads(m64, b, sample_weight=sw, divide_by_length=divide_by_length)
    errs = [float(np.abs(x.numpy() - want_g[n]).max() / max(np.abs(want_g[n]).max(), 1e-6))
            for n, x in zip(MLP_WEIGHT_NAMES, got_g)]
    print(f"[weighted autograd fp64 against NumPy rows: loss {abs(float(got_l) - want_l) / abs(want_l):.1e} "
          f"grad {max(errs):.1e}]", end=" ")
    assert abs(float(got_l) - want_l) <= 1e-12 * abs(want_l)
    for n, e in zip(MLP_WEIGHT_NAMES, errs):
        assert e <= 1e-9, (n, e)
    # the weights matter (the unweighted loss is elsewhere), tensors and float32 weights are taken as well
    plain_l, _ = _loss_and_grads(m64, b, divide_by_length=divide_by_length)
    assert abs(float(plain_l) - want_l) > 1e-3 * abs(want_l)
    t_l, _ = _loss_and_grads(m64, b, sample_weight=torch.as_tensor(sw), divide_by_length=divide_by_length)
    assert torch.equal(t_l, got_l)


def test_weights_of_one_are_the_unweighted_loss_and_all_pairs_is_refused():
    m, m64 = _fp64_model(seed=22)
    b = train_batch(B_, L_, A_, OBS_DIM, seed=22)
    for model in (m, m64):
        l0, g0 = _loss_and_grads(model, b) if model is m64 else _grads32(model, b)
        l1, g1 = _loss_and_grads(model, b, sample_weight=np.ones(B_)) if model is m64 else \
            _grads32(model, b, sample_weight=np.ones(B_, np.float32))
        assert torch.equal(l0, l1) and all(torch.equal(x, y) for x, y in zip(g0, g1))
    with pytest.raises(ValueError, match="pi_all_pairs"):
        mx.loss.default_loss_fn(m, b, pi_all_pairs=True, sample_weight=np.ones(B_))
    for bad in (np.ones(B_ + 1), np.ones((B_, 1)), np.float64(1.0)):
        with pytest.raises(ValueError, match="sample_weight"):
            mx.loss.default_loss_fn(m, b, sample_weight=bad)
        with pytest.raises(ValueError, match="sample_weight"):
            m.update(b, sample_weight=bad, backend="torch")


def _grads32(m, b, **kw):
    for p in mx.nn.mlp_trio_weights(m.network).values():
        p.grad = None
    loss = mx.loss.default_loss_fn(m, b, **kw)
    assert loss.dtype == torch.float32
    loss.backward()
    w = mx.nn.mlp_trio_weights(m.network)
    return loss.detach(), [w[n].grad.detach().clone() for n in MLP_WEIGHT_NAMES]


def test_update_hands_the_weights_to_the_torch_route_and_to_a_custom_loss():
    """backend="torch" on the CPU: the step with weights equals the step default_loss_fn(sample_weight=) defines; a
    custom loss_fn sees the keyword only when weights were given."""
    b = train_batch(B_, L_, A_, OBS_DIM, seed=23)
    sw = np.array([0.5, 0.0, 1.0, 0.25, 0.75], np.float32)
    m1 = train_model(A_, E_, OBS_DIM, seed=23, device="cpu", optimizer=("sgd", 1e-1))
    m2 = train_model(A_, E_, OBS_DIM, seed=23, device="cpu", optimizer=("sgd", 1e-1))
    want, _ = _grads32(m2, b, sample_weight=sw)
    assert m1.update(b, sample_weight=sw, backend="torch")["loss"] == float(want)
    assert m1.update(b, backend="auto")["loss"] != float(want)
    seen = []
    m3 = train_model(A_, E_, OBS_DIM, seed=23, device="cpu")

    def loss_fn(model, batch, **kw):
        seen.append(sorted(kw))
        return mx.loss.default_loss_fn(model, batch, **kw)
    m3.loss_fn = loss_fn
    m3.update(b)
    m3.update(b, sample_weight=sw)
    assert seen == [[], ["sample_weight"]]


# ---- the loop ----
class _VecEnv:
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


class _Model:
    device, _support_size = torch.device("cpu"), 10

    def __init__(self):
        self.calls = []

    def init(self, key, sample):
        pass

    def act(self, key, obs, with_pi=False, with_value=False, **kw):
        obs = np.asarray(obs, np.float32)
        a = (obs.sum(1) % 2).astype(np.int64)
        pi = np.stack([a == 0, a == 1], 1).astype(np.float32)
        return (a, pi, obs.sum(1).astype(np.float64)) if with_pi else a

    def update(self, batch, **kw):
        self.calls.append(kw)
        return {"loss": float(np.sum(batch.Rn))}


class _WeightingBuffer(mx.TrajectoryReplayBuffer):
    """The host buffer with the device buffer's extras, recording what the loop asks for."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.betas, self.written = [], []

    def sample(self, *a, with_indices=False, is_beta=None, **kw):
        batch = super().sample(*a, **kw)
        B = np.asarray(batch.Rn).shape[0]
        out = (batch,) + (((np.arange(B), np.zeros(B, np.int32)),) if with_indices else ())
        if is_beta is None:
            return out if with_indices else batch
        self.betas.append(is_beta)
        return out + (("isw", len(self.betas)),)

    def update_priorities(self, indices, priorities, **kw):
        self.written.append(indices)


def _fit(model, buffer, **kw):
    rows = []
    mx.fit_vector(model, _VecEnv(), _VecEnv(), n_step=2, gamma=0.9, buffer=buffer, iterations=2, steps_per_iteration=10,
                  num_simulations=2, k_steps=3, num_trajectory=4, num_update_per_iteration=3, test_interval=10,
                  random_seed=1, metrics=rows, max_training_steps=100, **kw)
    return rows


def test_fit_vector_refuses_is_beta_on_a_buffer_without_it():
    assert "is_beta" not in mx.TrajectoryReplayBuffer.sample.__code__.co_varnames
    model = _Model()
    with pytest.raises(ValueError, match="is_beta"):
        _fit(model, mx.TrajectoryReplayBuffer(50, random_seed=4), is_beta=0.5)
    with pytest.raises(ValueError, match="is_beta"):
        _fit(model, None, is_beta=lambda **kw: 0.5)
    assert model.calls == []
    for bad in (-0.5, 2.0):
        with pytest.raises(ValueError, match="is_beta"):
            _fit(model, _WeightingBuffer(50, random_seed=4), is_beta=bad)


def test_fit_vector_samples_with_is_beta_and_updates_with_the_weights(monkeypatch):
    from muax_amd import vector
    monkeypatch.setattr(vector, "value_priorities", lambda model, batch: "p")
    model, buf = _Model(), _WeightingBuffer(50, random_seed=4)
    _fit(model, buf, is_beta=0.4)
    assert buf.betas == [0.4] * 6 and [c["sample_weight"] for c in model.calls] == [("isw", i + 1) for i in range(6)]
    # a schedule, called before every batch as temperature_fn is; composes with the priority write-back
    model, buf, asked = _Model(), _WeightingBuffer(50, random_seed=4), []

    def schedule(training_steps, max_training_steps):
        asked.append((training_steps, max_training_steps))
        return min(1.0, 0.4 + 0.1 * training_steps)
    _fit(model, buf, is_beta=schedule, priority_update=True)
    assert asked == [(i, 100) for i in range(6)] and buf.betas == pytest.approx([0.4, 0.5, 0.6, 0.7, 0.8, 0.9])
    assert len(buf.written) == 6 and all(len(c["sample_weight"]) == 2 for c in model.calls)
    # None: update() gets no keyword, the buffer no is_beta, and the metrics are those of a run without the argument
    m0, m1, b0, b1 = _Model(), _Model(), _WeightingBuffer(50, random_seed=4), _WeightingBuffer(50, random_seed=4)
    rows0, rows1 = _fit(m0, b0), _fit(m1, b1, is_beta=None)
    for r in rows0 + rows1:
        r.pop("collect_s")
    assert rows0 == rows1 and m1.calls == [{}] * 6 and b1.betas == []
