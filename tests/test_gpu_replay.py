"""GPU tests of the device-resident trajectory replay (muax_amd/replay_device.py, muax_amd/csrc/mz_replay.cuh)
against tests/replay_reference.py, the NumPy float64 restatement of its sampling rules.

Where every weight is a multiple of 2^-10 below 2^10 all partial sums are exact in float64, so the drawn indices must
equal the reference's; with general weights each draw must fall between the reference's neighbouring prefix sums to
1e-12 relative (any correct float64 scan order passes, no row is left out)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import muax_amd as mx
import replay_reference as ref
from helpers import train_model
from muax_amd import vector

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 5
FIELDS = ("obs", "a", "r", "Rn", "v", "done", "pi", "w")


def _trajectory(ep, stepwise=False, pi_row=True):
    """The episode as a Trajectory: array-backed (pi as [T, 1, A], the reference's layout, or [T, A]) or filled step by
    step."""
    pi = ep["pi"][:, None, :] if pi_row else ep["pi"]
    if not stepwise:
        return mx.Trajectory.from_arrays(ep["obs"], ep["a"], ep["r"], ep["done"], ep["Rn"], ep["v"], pi, ep["w"])
    tr = mx.Trajectory()
    for t in range(len(ep["w"])):
        tr.add(mx.Transition(obs=ep["obs"][t], a=ep["a"][t], r=ep["r"][t], done=ep["done"][t], Rn=ep["Rn"][t],
                             v=ep["v"][t], pi=pi[t], w=ep["w"][t]))
    return tr


def _fill(buf, eps):
    """First episode by add() step-filled, second by add() array-backed, the rest by one add_many()."""
    buf.add(_trajectory(eps[0], stepwise=True), eps[0]["weight"])
    if len(eps) > 1:
        buf.add(_trajectory(eps[1], pi_row=False), eps[1]["weight"])
    if len(eps) > 2:
        buf.add_many([_trajectory(e) for e in eps[2:]], [e["weight"] for e in eps[2:]])
    return buf


def _host(batch):
    return {n: getattr(batch, n).cpu().numpy() for n in FIELDS}


def _assert_batch(batch, want):
    got = _host(batch)
    for n in FIELDS:
        assert got[n].dtype == want[n].dtype and got[n].shape == want[n].shape, (n, got[n].dtype, got[n].shape)
        assert np.array_equal(got[n], want[n]), n


@functools.lru_cache(maxsize=None)
def _exact_case(A, obs_dim):
    rng = np.random.default_rng(100 * A + obs_dim)
    eps = [ref.make_episode(rng, T, A, obs_dim) for T in (K + 1, K + 2, 37, 64, 65, 200)]
    return eps, _fill(mx.DeviceReplayBuffer(8, 512, random_seed=0), eps)


# ---- 1. exact draws ----
@pytest.mark.parametrize("spt", [1, 3])
@pytest.mark.parametrize("B", [1, 64, 257])
@pytest.mark.parametrize("A,obs_dim", [(3, 4), (18, 8), (64, 128)])
def test_exact_draws_and_windows(A, obs_dim, B, spt):
    eps, buf = _exact_case(A, obs_dim)
    key = [1000 + B, spt]
    batch, (serial, start) = buf.sample(num_trajectory=B, sample_per_trajectory=spt, k_steps=K, key=key, with_indices=True)
    e, s = ref.sample_indices(key, eps, B * spt, K, spt)
    assert serial.dtype == torch.int64 and start.dtype == torch.int32 and batch.done.dtype == torch.bool
    assert np.array_equal(serial.cpu().numpy(), e) and np.array_equal(start.cpu().numpy(), s)  # serial == index here
    _assert_batch(batch, ref.batch_fields(eps, e, s, K))
    assert batch.obs.shape == (B * spt, 1, obs_dim) and batch.pi.shape == (B * spt, K, A)


# ---- 2. edges ----
def test_edges_of_the_two_draws():
    rng = np.random.default_rng(2)
    A, od, rows = 3, 4, 4096
    one_hot = np.zeros(30)
    one_hot[7] = 0.25
    eps = [ref.make_episode(rng, K + 1, A, od, weight=2.0),          # 0: one possible start
           ref.make_episode(rng, K, A, od, weight=1000.0),           # 1: too short: no probability
           ref.make_episode(rng, 20, A, od, weight=0.0),             # 2: weight zero
           ref.make_episode(rng, 30, A, od, w=one_hot, weight=3.0),  # 3: one non-zero transition weight
           ref.make_episode(rng, 25, A, od, w=np.zeros(25), weight=4.0)]  # 4: all-zero transition weights
    buf = _fill(mx.DeviceReplayBuffer(8, 256), eps)
    key = [7, 7]
    batch, (serial, start) = buf.sample(rows, k_steps=K, key=key, with_indices=True)
    serial, start = serial.cpu().numpy(), start.cpu().numpy()
    e, s = ref.sample_indices(key, eps, rows, K)
    assert np.array_equal(serial, e) and np.array_equal(start, s)
    _assert_batch(batch, ref.batch_fields(eps, e, s, K))
    assert set(np.unique(serial)) == {0, 3, 4}
    assert (start[serial == 0] == 0).all() and (start[serial == 3] == 7).all()
    _, u1 = ref.draws(key, rows)
    on4 = serial == 4
    assert np.array_equal(start[on4], np.floor(u1[on4] * 20).astype(np.int32)) and len(np.unique(start[on4])) == 20


def test_single_episode_buffer():
    rng = np.random.default_rng(3)
    ep = ref.make_episode(rng, 40, 18, 8)
    buf = _fill(mx.DeviceReplayBuffer(1, 40), [ep])
    assert len(buf) == 1 and buf.steps == 40
    batch, (serial, start) = buf.sample(300, k_steps=K, key=5, with_indices=True)
    e, s = ref.sample_indices(mx.prng.PRNGKey(5), [ep], 300, K)
    assert not serial.any() and not e.any() and np.array_equal(start.cpu().numpy(), s)
    _assert_batch(batch, ref.batch_fields([ep], e, s, K))
    with pytest.raises(ValueError, match="longer than k_steps"):
        buf.sample(4, k_steps=40)
    with pytest.raises(ValueError, match="max_steps"):
        buf.add(_trajectory(ref.make_episode(rng, 41, 18, 8)), 1.0)
    assert len(buf) == 1
    with pytest.raises(ValueError, match="obs_dim"):
        buf.add(_trajectory(ref.make_episode(rng, 10, 18, 9)), 1.0)


# ---- 3. general weights ----
def test_general_weights_fall_between_the_reference_prefix_sums():
    rng = np.random.default_rng(4)
    A, od, rows, tol = 3, 4, 4096, 1e-12
    eps = []
    for T in rng.integers(K - 1, 60, 50):
        w = np.abs(rng.standard_normal(T)) ** 0.5
        eps.append(ref.make_episode(rng, int(T), A, od, w=w, weight=w.mean()))
    buf = _fill(mx.DeviceReplayBuffer(64, 4096), eps)
    key = [11, 12]
    batch, (serial, start) = buf.sample(rows, k_steps=K, key=key, with_indices=True)
    e, s = serial.cpu().numpy(), start.cpu().numpy()
    u0, u1 = ref.draws(key, rows)
    lengths = np.array([len(ep["w"]) for ep in eps])
    CW = ref.episode_cw([ep["weight"] for ep in eps], lengths, K)
    below = np.concatenate([[0.0], CW])[e]
    assert (lengths[e] > K).all()
    assert (below * (1 - tol) <= u0 * CW[-1]).all() and (u0 * CW[-1] <= CW[e] * (1 + tol)).all()
    for j in range(rows):
        m = lengths[e[j]] - K
        cw = np.cumsum(eps[e[j]]["w"])[:m]
        assert 0 <= s[j] < m
        t = u1[j] * cw[-1]
        assert (cw[s[j] - 1] if s[j] else 0.0) * (1 - tol) <= t <= cw[s[j]] * (1 + tol), j
    _assert_batch(batch, ref.batch_fields(eps, e, s, K))
    # sequential fp64 sums on both sides: in fact the very same indices
    e2, s2 = ref.sample_indices(key, eps, rows, K)
    print(f"[rows whose indices differ from the sequential reference: {int((e != e2).sum() + (s != s2).sum())}]", end=" ")


# ---- 4. eviction and wrap ----
def test_eviction_and_wrap_follow_the_host_model():
    rng = np.random.default_rng(5)
    A, od = 3, 4
    buf, model, kept = mx.DeviceReplayBuffer(5, 300, random_seed=1), ref.ArenaModel(5, 300), {}
    cycle = (30, 45, 60, 75, 90, 105, 120)
    wrapped = False
    for i in range(40):
        ep = ref.make_episode(rng, cycle[i % len(cycle)], A, od)
        kept[i] = ep
        buf.add(_trajectory(ep), ep["weight"])
        model.add(len(ep["w"]))
        assert len(buf) == len(model.live) and buf.steps == model.steps and buf.serials == model.serials
        wrapped |= model.live[-1][1] < model.live[0][1]
        if i % 5 == 4:
            batch, (serial, start) = buf.sample(512, k_steps=K, with_indices=True)
            serial, start = serial.cpu().numpy(), start.cpu().numpy()
            assert set(serial.tolist()) <= set(model.serials)
            want = ref.batch_fields(kept, serial, start, K)
            _assert_batch(batch, want)
            live = [kept[s] for s in model.serials]
    assert wrapped and len(buf) < 5 + 1
    buf.clear()
    assert len(buf) == 0 and buf.steps == 0 and not buf
    buf.add(_trajectory(live[0]), 1.0)
    assert buf.serials == [40] and int(buf.sample(8, k_steps=K, with_indices=True)[1][0][0]) == 40


def test_a_collection_larger_than_the_buffer_keeps_its_tail():
    rng = np.random.default_rng(6)
    eps = [ref.make_episode(rng, 50, 3, 4) for _ in range(9)]
    buf = mx.DeviceReplayBuffer(4, 120)
    buf.add_many([_trajectory(e) for e in eps], [e["weight"] for e in eps])
    model = ref.ArenaModel(4, 120)
    for e in eps:
        model.add(50)
    assert buf.serials == model.serials == [7, 8] and buf.steps == 100
    batch, (serial, start) = buf.sample(256, k_steps=K, key=3, with_indices=True)
    serial, start = serial.cpu().numpy(), start.cpu().numpy()
    assert set(serial.tolist()) == {7, 8}
    _assert_batch(batch, ref.batch_fields(dict(enumerate(eps)), serial, start, K))


# ---- 5. add_raw ----
def _raw_stream(rng, lengths, A, od, dyadic=False):
    M = sum(lengths)
    if dyadic:
        r = rng.integers(-16, 17, M) / 8.0
        v = (rng.integers(-64, 65, M) / 8.0).astype(np.float32)
    else:
        r, v = rng.uniform(-2, 3, M), rng.uniform(-30, 60, M).astype(np.float32)
    return dict(obs=rng.uniform(-1, 1, (M, od)).astype(np.float32), a=rng.integers(0, A, M), r=r,
                v=v.astype(np.float64), pi=rng.dirichlet(np.ones(A), M).astype(np.float32))


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("alpha", [0.5, None])
def test_add_raw_computes_the_nstep_fields(alpha, on_device):
    n, gamma, A, od = 10, 0.997, 3, 4
    lengths = [1, n - 1, n, n + 1, 3 * n + 2]
    st = _raw_stream(np.random.default_rng(7), lengths, A, od)
    buf = mx.DeviceReplayBuffer(8, 128)
    x = {k: torch.as_tensor(val).cuda() for k, val in st.items()} if on_device else st
    buf.add_raw(x["obs"], x["a"], x["r"], x["v"], x["pi"], lengths, n, gamma, alpha, weight="mean")
    assert len(buf) == 5 and buf.steps == sum(lengths)
    first = 0
    for serial, T in enumerate(lengths):
        s = slice(first, first + T)
        first += T
        Rn, done = vector.nstep_returns(st["r"][s], st["v"][s], n, gamma)
        got = buf.episode(serial)
        assert np.array_equal(got.Rn.cpu().numpy(), Rn.astype(np.float32)), T
        assert np.array_equal(got.done.cpu().numpy().astype(bool), done), T
        assert np.array_equal(got.r.cpu().numpy(), st["r"][s].astype(np.float32))
        assert np.array_equal(got.v.cpu().numpy(), st["v"][s].astype(np.float32))
        assert np.array_equal(got.a.cpu().numpy(), st["a"][s]) and np.array_equal(got.obs.cpu().numpy(), st["obs"][s])
        assert np.array_equal(got.pi.cpu().numpy(), st["pi"][s])
        w = got.w.cpu().numpy()
        assert w.dtype == np.float64
        if alpha is None:
            assert (w == 1.0).all()
        else:
            want = np.abs(st["v"][s] - Rn) ** alpha
            err = np.abs(w - want) / want
            print(f"[T {T}: w relative error {err.max():.1e}]", end=" ")
            assert (err <= 1e-12).all(), (T, err.max())


def test_sampling_after_add_raw_equals_add_of_episode_trajectory():
    """Dyadic rewards, values and gamma = 0.5: every return is exact, so both routes store the same numbers."""
    n, gamma, A, od = 3, 0.5, 3, 4
    lengths = [K + 2, 12, 33, K, 70]
    st = _raw_stream(np.random.default_rng(8), lengths, A, od, dyadic=True)
    raw, cooked = mx.DeviceReplayBuffer(8, 256), mx.DeviceReplayBuffer(8, 256)
    raw.add_raw(st["obs"], st["a"], st["r"], st["v"], st["pi"], lengths, n, gamma, None, weight="sum")
    first = 0
    for T in lengths:
        s = slice(first, first + T)
        first += T
        tr = vector.episode_trajectory(st["obs"][s], st["a"][s], st["r"][s], st["v"][s], st["pi"][s], n, gamma, None)
        cooked.add(tr, tr.weights.sum())
    for key in (1, 2):
        b0, i0 = raw.sample(num_trajectory=100, sample_per_trajectory=2, k_steps=K, key=key, with_indices=True)
        b1, i1 = cooked.sample(num_trajectory=100, sample_per_trajectory=2, k_steps=K, key=key, with_indices=True)
        assert torch.equal(i0[0], i1[0]) and torch.equal(i0[1], i1[1]) and len(torch.unique(i0[0])) == 4
        for name in FIELDS:
            assert torch.equal(getattr(b0, name), getattr(b1, name)), name


# ---- 6. feeds update() in place ----
@pytest.mark.parametrize("A,support", [(2, 10), (18, 31)])
def test_device_batch_feeds_update_in_place(A, support):
    E, od, B = 8, 4, 64
    rng = np.random.default_rng(9)
    eps = [ref.make_episode(rng, T, A, od) for T in (20, 33, 64)]
    buf = _fill(mx.DeviceReplayBuffer(4, 128), eps)
    dev = buf.sample(B, k_steps=K, key=21)
    h = _host(dev)
    host = mx.Transition(obs=np.tile(h["obs"], (1, K, 1)), a=h["a"], r=h["r"], done=h["done"], Rn=h["Rn"], v=h["v"],
                         pi=h["pi"].reshape(B, K, 1, A), w=h["w"])
    m_dev, m_host = (train_model(A, E, od, seed=5, support=support) for _ in range(2))
    ptrs = {n: getattr(dev, n).data_ptr() for n in ("a", "r", "Rn", "pi", "obs")}
    for step in range(2):
        l_dev, l_host = m_dev.update(dev, backend="hip")["loss"], m_host.update(host, backend="hip")["loss"]
        assert np.isfinite(l_dev) and l_dev == l_host, (step, l_dev, l_host)
    for p, q in zip((p for mod in m_dev.network for p in mod.parameters()),
                    (p for mod in m_host.network for p in mod.parameters())):
        assert torch.equal(p, q)
    obs, a, r, Rn, pi, _ = m_dev._fused_train._keep  # what the kernel read: the batch's own storage
    assert (a.data_ptr(), r.data_ptr(), Rn.data_ptr(), pi.data_ptr(), obs.data_ptr()) == \
        tuple(ptrs[n] for n in ("a", "r", "Rn", "pi", "obs"))
    assert all(getattr(dev, n).data_ptr() == ptrs[n] for n in ptrs)


# ---- 7. no host contact ----
def test_sample_is_captured_in_a_graph():
    eps, buf = _exact_case(3, 4)
    eager, (serial, start) = buf.sample(64, k_steps=K, key=[4, 2], with_indices=True)  # (no pending adds afterwards)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, (serial_g, start_g) = buf.sample(64, k_steps=K, key=[4, 2], with_indices=True)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(serial, serial_g) and torch.equal(start, start_g)
    for n in FIELDS:
        assert torch.equal(getattr(eager, n), getattr(out, n)), n


# ---- 8. fit_vector ----
def _fit_vector_once(seed):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from cartpole_env import VectorCartPole
    g = torch.Generator().manual_seed(0)
    net = mx.nn.MZNetwork(mx.nn.Representation(8, generator=g), mx.nn.Prediction(2, 21, generator=g),
                          mx.nn.Dynamic(8, 2, 21, generator=g))
    model = mx.MuZero(net, optimizer=mx.optimizers.create_optimizer("adam", 5e-3))
    buf, rows = mx.DeviceReplayBuffer(64, 4096, random_seed=seed), []
    mx.fit_vector(model, VectorCartPole(16, seed=0), VectorCartPole(2, max_episode_steps=20, seed=1), n_step=3, buffer=buf,
                  iterations=3, steps_per_iteration=8, num_simulations=8, k_steps=3, num_trajectory=8,
                  sample_per_trajectory=2, num_update_per_iteration=2, test_interval=10, random_seed=3, metrics=rows)
    return model, buf, rows


def test_fit_vector_runs_on_the_device_buffer():
    model, buf, rows = _fit_vector_once(seed=13)
    assert len(rows) == 3 and len(buf) > 0 and buf.steps > 0
    losses = [r["loss"] for r in rows if "loss" in r]
    assert losses and np.isfinite(losses).all() and model._fused_train is not None
    _, buf2, rows2 = _fit_vector_once(seed=13)
    assert [r.get("loss") for r in rows2] == [r.get("loss") for r in rows] and buf2.serials == buf.serials
    for _ in range(2):  # the same seed and the same adds: the same batches, call after call
        b1, b2 = buf.sample(16, k_steps=3, with_indices=True), buf2.sample(16, k_steps=3, with_indices=True)
        assert torch.equal(b1[1][0], b2[1][0]) and torch.equal(b1[1][1], b2[1][1]) and torch.equal(b1[0].pi, b2[0].pi)
    other = mx.DeviceReplayBuffer(64, 4096, random_seed=14)
    assert not np.array_equal(other._key, mx.DeviceReplayBuffer(64, 4096, random_seed=13)._key)
