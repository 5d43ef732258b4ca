"""GPU tests of reanalysis on the device (DeviceReplayBuffer.reanalyse / stalest, mzs_replay_gather_obs,
mzs_replay_reanalyse) against tests/reanalyse_reference.py and the public MuZero.act.

The expected search results come from `model.act` on NumPy observations (the one-call host route), chunk by chunk on
the zero-padded concatenation of the stored observations with `prng.split(key, n_chunks)`; the fields that follow from
them from the NumPy restatement.  pi, v, Rn, done and cw must be equal bit for bit, w to 1e-12 relative (the two
libms' pow: the bar of test_add_raw_computes_the_nstep_fields)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import muax_amd as mx
import reanalyse_reference as rref
from helpers import train_model
from muax_amd import prng

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, GAMMA, S, R = 10, 0.997, 8, 64
LENGTHS = [1, N - 1, N, N + 1, 3 * N + 2, 70]  # 133 rows: three chunks of 64, the last with 59 padding rows
SHAPES = {"narrow": (2, 8, 4), "wide": (18, 8, 5)}  # (A, E, obs_dim): a listed fused instance; the wide-action kernel
FIELDS = ("obs", "a", "r", "Rn", "v", "done", "pi", "w")
KEY = 77


@functools.lru_cache(maxsize=None)
def _model(kind):
    A, E, od = SHAPES[kind]
    return train_model(A, E, od, seed=3, support=10)


@functools.lru_cache(maxsize=None)
def _stream(kind, lengths=tuple(LENGTHS)):
    A, _, od = SHAPES[kind]
    rng = np.random.default_rng(17 + A)
    M = sum(lengths)
    return dict(obs=rng.uniform(-1, 1, (M, od)).astype(np.float32), a=rng.integers(0, A, M), r=rng.uniform(-2, 3, M),
                v=rng.uniform(-30, 60, M).astype(np.float32).astype(np.float64),
                pi=rng.dirichlet(np.ones(A), M).astype(np.float32))


def _filled(kind, alpha, weight, lengths=tuple(LENGTHS), capacity=8, max_steps=256):
    st = _stream(kind, lengths)
    buf = mx.DeviceReplayBuffer(capacity, max_steps)
    buf.add_raw(st["obs"], st["a"], st["r"], st["v"], st["pi"], list(lengths), N, GAMMA, alpha, weight=weight)
    return buf


def _rows(buf, serial):
    e = next(e for e in buf._eps if e.serial == serial)
    return e, slice(e.start, e.start + e.length)


def _episode(buf, serial):
    """Host copies of every stored field of an episode, cw and its table weight included."""
    e, rows = _rows(buf, serial)
    out = {n: getattr(buf.episode(serial), n).cpu().numpy().copy() for n in FIELDS}
    out["cw"] = buf._t["cw"][rows].cpu().numpy().copy()
    out["t_w"] = float(buf._t["t_w"][e.slot].cpu())
    return out


def _arenas(buf):
    return {n: t.clone() for n, t in buf._t.items() if not n.startswith("c_")}  # (c_*: the compact table of sample())


def _searched(model, buf, serials, key):
    """{serial: (pi [T, A], v [T])} by the public act(), NumPy in and out, on the padded stream of these episodes."""
    obs = np.concatenate([buf.episode(s).obs.cpu().numpy() for s in serials])
    M = len(obs)
    chunks = -(-M // R)
    obs = np.concatenate([obs, np.zeros((chunks * R - M, obs.shape[1]), np.float32)])
    keys = prng.split(prng.as_key(key), chunks)
    pi, v = [], []
    for c in range(chunks):
        _, p, x = model.act(keys[c], obs[c * R:(c + 1) * R], with_pi=True, with_value=True, obs_from_batch=True,
                            num_simulations=S)
        assert isinstance(p, np.ndarray) and p.dtype == np.float32 and x.dtype == np.float32
        pi.append(p), v.append(x)
    pi, v = np.concatenate(pi), np.concatenate(v)
    out, first = {}, 0
    for s in serials:
        T = len(buf.episode(s).a)
        out[s] = (pi[first:first + T], v[first:first + T])
        first += T
    return out


def _assert_reanalysed(got, before, pi, v, alpha, weight):
    T = len(v)
    assert np.array_equal(got["pi"], pi) and np.array_equal(got["v"], v), T
    assert not np.array_equal(got["pi"], before["pi"]) and not np.array_equal(got["v"], before["v"])
    Rn, done, w, _, _ = rref.targets(before["r"], pi, v, N, GAMMA, alpha, weight)
    assert got["Rn"].dtype == np.float32 and np.array_equal(got["Rn"], Rn), T
    assert np.array_equal(got["done"].astype(bool), done), T
    assert got["w"].dtype == np.float64
    nz = w != 0
    err = np.abs(got["w"][nz] - w[nz]) / w[nz]
    print(f"[T {T}: w relative error {err.max() if err.size else 0.0:.1e}]", end=" ")
    assert (err <= 1e-12).all() and np.array_equal(got["w"][~nz], w[~nz]), T
    if alpha is None:
        assert (got["w"] == 1.0).all()
    cw = np.cumsum(got["w"])
    assert np.array_equal(got["cw"], cw), T
    assert got["t_w"] == (cw[-1] / T if weight == "mean" else cw[-1]), T
    for n in ("obs", "a", "r"):
        assert np.array_equal(got[n], before[n]), n


def _assert_untouched(got, before):
    for n in before:
        assert np.array_equal(got[n], before[n]), n


# ---- 1. every field ----
@pytest.mark.parametrize("kind,alpha,weight", [("narrow", 0.5, "mean"), ("narrow", 0.5, "sum"), ("narrow", None, "mean"),
                                               ("narrow", None, "sum"), ("wide", 0.5, "mean")])
def test_fields_after_reanalysis_bit_for_bit(kind, alpha, weight):
    model, buf = _model(kind), _filled(kind, alpha, weight)
    serials = buf.serials
    assert serials == list(range(len(LENGTHS)))
    before = {s: _episode(buf, s) for s in serials}
    want = _searched(model, buf, serials, KEY)
    assert buf.reanalyse(model, KEY, N, GAMMA, alpha, weight, chunk_rows=R, num_simulations=S) == sum(LENGTHS)
    assert buf.serials == serials and buf.steps == sum(LENGTHS) and buf._dirty
    for s in serials:
        _assert_reanalysed(_episode(buf, s), before[s], *want[s], alpha, weight)


# ---- 2. only what was asked ----
def test_only_the_selected_episodes_change():
    model, buf = _model("narrow"), _filled("narrow", 0.5, "mean")
    before = {s: _episode(buf, s) for s in buf.serials}
    arenas = _arenas(buf)
    want = _searched(model, buf, [4, 1], KEY)  # stream order: episode 4, then episode 1 (one chunk, key split in one)
    assert buf.reanalyse(model, KEY, N, GAMMA, 0.5, "mean", serials=[4, 1], chunk_rows=R, num_simulations=S) == 32 + 9
    for s in (0, 2, 3, 5):
        _assert_untouched(_episode(buf, s), before[s])
    for s in (4, 1):
        _assert_reanalysed(_episode(buf, s), before[s], *want[s], 0.5, "mean")
    # the rest of the arenas and of the table, the never-used rows included
    changed = torch.zeros(buf.max_steps, dtype=torch.bool, device="cuda")
    slots = torch.zeros(buf.capacity, dtype=torch.bool, device="cuda")
    for s in (4, 1):
        e, rows = _rows(buf, s)
        changed[rows], slots[e.slot] = True, True
    for n, was in arenas.items():
        keep = ~(slots if n.startswith("t_") else changed)
        assert torch.equal(buf._t[n][keep], was[keep]), n
    for n in ("t_start", "t_len", "t_serial"):
        assert torch.equal(buf._t[n], arenas[n]), n


# ---- 3. the same buffer as a fresh add_raw of the new results ----
@pytest.mark.parametrize("alpha,weight", [(0.5, "mean"), (0.5, "sum")])
def test_sampling_after_reanalysis_equals_a_fresh_add_raw(alpha, weight):
    model, buf = _model("narrow"), _filled("narrow", alpha, weight)
    buf.sample(4, k_steps=5, key=0)  # the compact table is built from the OLD weights: reanalyse must mark it stale
    buf.reanalyse(model, KEY, N, GAMMA, alpha, weight, chunk_rows=R, num_simulations=S)
    eps = [buf.episode(s) for s in buf.serials]
    cat = {n: torch.cat([getattr(e, n) for e in eps]) for n in ("obs", "a", "r", "v", "pi")}
    fresh = mx.DeviceReplayBuffer(8, 256)
    fresh.add_raw(cat["obs"], cat["a"], cat["r"], cat["v"].to(torch.float64), cat["pi"], LENGTHS, N, GAMMA, alpha,
                  weight=weight)
    for key in (1, 2):
        b0, i0 = buf.sample(num_trajectory=100, sample_per_trajectory=2, k_steps=5, key=key, with_indices=True)
        b1, i1 = fresh.sample(num_trajectory=100, sample_per_trajectory=2, k_steps=5, key=key, with_indices=True)
        assert torch.equal(i0[0], i1[0]) and torch.equal(i0[1], i1[1]) and len(torch.unique(i0[0])) > 1
        for n in FIELDS:
            assert torch.equal(getattr(b0, n), getattr(b1, n)), n


# ---- 4. wrapped arena, evicted serials ----
def test_wrapped_arena_and_refused_serials():
    model = _model("narrow")
    lengths = (30, 30, 40, 25)
    st = _stream("narrow", lengths)
    buf = mx.DeviceReplayBuffer(8, 100)
    for lo, hi, ls in ((0, 100, [30, 30, 40]), (100, 125, [25])):  # the fourth wraps: episode 0 goes, it lands at row 0
        buf.add_raw(st["obs"][lo:hi], st["a"][lo:hi], st["r"][lo:hi], st["v"][lo:hi], st["pi"][lo:hi], ls, N, GAMMA, 0.5)
    assert buf.serials == [1, 2, 3]
    (e2, _), (e3, _) = _rows(buf, 2), _rows(buf, 3)
    assert e3.start == 0 and e2.start + e2.length == buf.max_steps
    arenas = _arenas(buf)
    with pytest.raises(KeyError):
        buf.reanalyse(model, KEY, N, GAMMA, 0.5, serials=[3, 0], chunk_rows=R, num_simulations=S)
    with pytest.raises(ValueError):
        buf.reanalyse(model, KEY, N, GAMMA, 0.5, serials=[2, 3, 2], chunk_rows=R, num_simulations=S)
    for n, was in arenas.items():
        assert torch.equal(buf._t[n], was), n
    before = {s: _episode(buf, s) for s in buf.serials}
    want = _searched(model, buf, [3, 2], KEY)  # 65 rows: episode 2 straddles the two chunks
    assert buf.reanalyse(model, KEY, N, GAMMA, 0.5, serials=[3, 2], chunk_rows=R, num_simulations=S) == 65
    for s in (3, 2):
        _assert_reanalysed(_episode(buf, s), before[s], *want[s], 0.5, "mean")
    _assert_untouched(_episode(buf, 1), before[1])


# ---- 5. stalest ----
def test_stalest_orders_by_the_last_write():
    model = _model("narrow")
    buf = _filled("narrow", 0.5, "mean", lengths=(12, 12, 12, 12, 12), capacity=5, max_steps=128)
    assert buf.stalest(5) == [0, 1, 2, 3, 4] and buf.stalest(2) == [0, 1]
    assert buf.reanalyse(model, KEY, N, GAMMA, 0.5, serials=[1, 3], chunk_rows=R, num_simulations=S) == 24
    assert buf.stalest(5) == [0, 2, 4, 1, 3] and buf.stalest(3) == [0, 2, 4]
    buf._evict()  # (what the next add does to the oldest episode)
    assert buf.serials == [1, 2, 3, 4] and buf.stalest(5) == [2, 4, 1, 3]
    st = _stream("narrow", (12,))
    buf.add_raw(st["obs"], st["a"], st["r"], st["v"], st["pi"], [12], N, GAMMA, 0.5)
    assert buf.stalest(5) == [2, 4, 1, 3, 5] and buf.stalest(4) == [2, 4, 1, 3]


# ---- 6. fit_vector ----
def _fit_vector_once(seed, **kw):
    """The arguments of test_gpu_replay.py's _fit_vector_once, plus `kw`."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from cartpole_env import VectorCartPole
    g = torch.Generator().manual_seed(0)
    net = mx.nn.MZNetwork(mx.nn.Representation(8, generator=g), mx.nn.Prediction(2, 21, generator=g),
                          mx.nn.Dynamic(8, 2, 21, generator=g))
    model = mx.MuZero(net, optimizer=mx.optimizers.create_optimizer("adam", 5e-3))
    buf, rows = mx.DeviceReplayBuffer(64, 4096, random_seed=seed), []
    mx.fit_vector(model, VectorCartPole(16, seed=0), VectorCartPole(2, max_episode_steps=20, seed=1), n_step=3, buffer=buf,
                  iterations=3, steps_per_iteration=8, num_simulations=8, k_steps=3, num_trajectory=8,
                  sample_per_trajectory=2, num_update_per_iteration=2, test_interval=10, random_seed=3, metrics=rows, **kw)
    return model, buf, rows


def test_fit_vector_reanalyses_before_its_updates():
    _, buf, rows = _fit_vector_once(13, reanalyse_every=1)
    losses = [r["loss"] for r in rows if "loss" in r]
    assert len(rows) == 3 and losses and np.isfinite(losses).all() and len(buf) > 0
    _, buf2, rows2 = _fit_vector_once(13, reanalyse_every=1)
    assert [r.get("loss") for r in rows2] == [r.get("loss") for r in rows] and buf2.serials == buf.serials
    for s in buf.serials:
        assert torch.equal(buf.episode(s).pi, buf2.episode(s).pi) and torch.equal(buf.episode(s).w, buf2.episode(s).w)
    _, _, rows0 = _fit_vector_once(13, reanalyse_every=0)
    losses0 = [r["loss"] for r in rows0 if "loss" in r]
    assert losses0 != losses
    # up to the first iteration with updates both runs collected the same episodes with the same keys: that loss
    # differs through the refreshed targets alone
    assert ["loss" in r for r in rows0] == ["loss" in r for r in rows] and losses0[0] != losses[0]
