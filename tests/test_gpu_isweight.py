"""GPU tests of the importance-sampling weights of prioritised replay: mzs_replay_sample_is called directly on guarded
buffers (the harness of tests/replay_abi.py, plus the one call it lacks) against the plain-loop reference
(tests/isweight_reference.py); the fused training step with a weight per row (mzs_mlp_loss_grad_weighted) at a listed, a
narrow on-demand and a wide on-demand instance against fp64 autograd of `default_loss_fn(sample_weight=)`; the public
route `DeviceReplayBuffer.sample(is_beta=)` -> `MuZero.update(sample_weight=)`; and `fit_vector(is_beta=)`.

Bars: isw bit for bit at beta 0 and 1 (divisions and one product in fp64, one rounding to float32), within one float32
ulp at beta 0.4 (one fp64 pow, held to 1e-12 in test_gpu_priority.py: the rounding to float32 can move the last bit);
the training step's own bars -- loss 1e-5 relative, each gradient array 2e-4 of its largest fp64 entry."""
import copy
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

import isweight_reference as isref
import muax_amd as mx
import replay_reference as rr
from helpers import train_batch, train_model
from muax_amd import _jit, _lib
from muax_amd._lib import MLP_WEIGHT_NAMES
from replay_abi import Guarded, Replay, layout

pytestmark = pytest.mark.gpu
F32 = np.float32
OBS_DIM, ACTIONS, BATCH = 3, 2, 67  # 67 rows: 17 workgroups of kReplayWaves = 4, the last one partly filled
FIELDS = ("obs", "a", "r", "Rn", "v", "done", "pi", "w", "serial", "start")


# ---- 1. the sample entry on guarded buffers ----
def sample_is(rp, count, B, k, spt, key, beta, num_windows, normalize, with_scratch=True):
    """mzs_replay_sample_is through Replay._call: (status, {field: host array, "isw": [B] float32}); every output and
    the scratch start as the pattern and keep their guards."""
    shapes = dict(obs=(B, rp.obs_dim, torch.float32), a=(B, k, torch.int32), r=(B, k, torch.float32),
                  Rn=(B, k, torch.float32), v=(B, k, torch.float32), done=(B, k, torch.uint8),
                  pi=(B, k * rp.A, torch.float32), w=(B, k, torch.float32), serial=(B, 1, torch.int64),
                  start=(B, 1, torch.int32))
    out = {n: Guarded(rows, width, dt, flat=False) for n, (rows, width, dt) in shapes.items()}
    isw, scratch = Guarded(B, 1, torch.float32), Guarded(B, 1, torch.float64)
    s = _lib.MzsReplaySampleArgs()
    s.struct_size = C.sizeof(_lib.MzsReplaySampleArgs)
    s.count, s.batch, s.k_steps, s.sample_per_trajectory = int(count), int(B), int(k), int(spt)
    s.key[0], s.key[1] = int(key[0]), int(key[1])
    for n, g in out.items():
        setattr(s, n, g.ptr)
    q = _lib.MzsReplayIsArgs()
    q.struct_size = C.sizeof(_lib.MzsReplayIsArgs)
    q.normalize, q.beta, q.num_windows = int(normalize), float(beta), float(num_windows)
    q.isw, q.scratch = isw.ptr, scratch.ptr if with_scratch else None
    was = scratch.bits.clone()
    rc = rp._call(rp.L.mzs_replay_sample_is, (C.byref(rp.arena), C.byref(s), C.byref(q)), {},
                  [(g, True) for g in list(out.values()) + [isw, scratch]])
    if not normalize or rc != _lib.MZS_OK:
        assert torch.equal(scratch.bits, was), "the scratch was written without a normalisation pass"
    got = {n: g.host() for n, g in out.items()}
    got["pi"] = got["pi"].reshape(B, k, rp.A)
    got["serial"], got["start"] = got["serial"][:, 0], got["start"][:, 0]
    got["isw"] = isw.host()
    return rc, got


def _stored(lengths, k, seed, variant="dyadic"):
    """The episodes (oldest first, table slots from head 1 on) stored by the copy branch and refreshed for k.
    "zero_episode": the longest episode has all-zero transition weights and a large buffer weight (uniform start);
    "zero_buffer": every buffer weight is zero."""
    rng = np.random.default_rng(seed)
    eps = [rr.make_episode(rng, T, ACTIONS, OBS_DIM, w=rr.dyadic_weights(rng, T) + 2.0 ** -10) for T in lengths]
    if variant == "zero_episode":
        j = int(np.argmax(lengths))
        eps[j]["w"], eps[j]["weight"] = np.zeros(lengths[j]), 4096.0
    if variant == "zero_buffer":
        for ep in eps:
            ep["weight"] = 0.0
    count, cap, head = len(lengths), len(lengths) + 2, 1
    rp = Replay(sum(lengths) + 3 * count, cap, OBS_DIM, ACTIONS)
    desc = layout(list(lengths), rp.max_steps, cap, seed=seed)
    desc[:, 3] = (head + np.arange(count)) % cap
    cat = {n: np.concatenate([ep[n] for ep in eps]) for n in ("obs", "a", "r", "Rn", "v", "done", "pi", "w")}
    serial = 40 + np.arange(count)
    assert rp.store(desc, serial, cat["obs"], cat["a"], cat["pi"], cat["r"], cat["v"], raw=False,
                    ep_w=[ep["weight"] for ep in eps], Rn=cat["Rn"], done=cat["done"].astype(np.uint8),
                    w=cat["w"]) == _lib.MZS_OK
    assert rp.refresh(head, count, k) == _lib.MZS_OK
    return rp, eps, serial


@functools.lru_cache(maxsize=None)
def _case(lengths, k, variant):
    return _stored(lengths, k, seed=len(lengths) + k, variant=variant)


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("spt", [1, 3])
@pytest.mark.parametrize("lengths,k,variant", [((3, 7, 12, 5), 4, "dyadic"), ((3, 7, 12, 5), 4, "zero_episode"),
                                               ((9, 9), 8, "dyadic")])
def test_sample_is_keeps_the_batch_and_adds_the_reference_weights(lengths, k, variant, spt):
    rp, eps, serial = _case(lengths, k, variant)
    count, key = len(lengths), [300 + k, spt]
    N = isref.eligible_windows(lengths, k)
    assert N == sum(T - k for T in lengths if T > k) < sum(lengths)  # (not the count over all episodes)
    rc, plain = rp.sample(count, BATCH, k, spt, key)
    assert rc == _lib.MZS_OK
    hit_uniform = 0
    for beta in (1.0, 0.4, 0.0):
        for normalize in (True, False):
            rc, got = sample_is(rp, count, BATCH, k, spt, key, beta, N, normalize)
            assert rc == _lib.MZS_OK
            for n in FIELDS:  # the draws and every field: those of mzs_replay_sample, byte for byte
                assert got[n].dtype == plain[n].dtype and got[n].tobytes() == plain[n].tobytes(), (n, beta, normalize)
            want = isref.weights(key, eps, BATCH, k, spt, beta=beta, normalize=normalize)
            assert np.array_equal(got["serial"], serial[want["e"]]) and np.array_equal(got["start"], want["start"])
            isw = got["isw"]
            assert isw.dtype == F32 and np.isfinite(isw).all() and (isw > 0).all()
            worst = int(_ulps(isw, want["isw"]).max())
            print(f"[beta {beta} normalize {int(normalize)}: worst {worst} ulp]", end=" ")
            if beta in (0.0, 1.0):
                assert np.array_equal(isw.view(np.uint32), want["isw"].view(np.uint32)), (beta, normalize)
            else:
                assert worst <= 1, (beta, normalize, worst)
            if beta == 0.0:
                assert (isw == 1.0).all()
            if normalize:  # (a min in the maximum's place gives weights above 1)
                assert isw.max() == 1.0 and (isw <= 1.0).all()
            if variant == "zero_episode":  # the uniform-start path: p_s = 1 / m
                on = want["e"] == int(np.argmax(lengths))
                hit_uniform += int(on.sum())
                if beta == 1.0 and not normalize:
                    m, p_e = max(lengths) - k, isref.episode_probability(eps, int(np.argmax(lengths)), k)
                    assert np.array_equal(isw[on], np.full(on.sum(), F32(1.0 / (N * (p_e * (1.0 / m))))))
    assert hit_uniform or variant != "zero_episode"


@pytest.mark.parametrize("lengths,zero_rows", [((9, 5), True), ((9, 9), False)])
def test_every_buffer_weight_zero(lengths, zero_rows):
    """The draw lands on the newest episode (p_e = 1); when that one is no longer than k the rows are zero-filled and
    their weights are 0, normalised or not."""
    k = 8
    rp, eps, serial = _case(lengths, k, "zero_buffer")
    assert not rp.host("c_CW")[:2].any()
    N = isref.eligible_windows(lengths, k)
    for beta in (1.0, 0.4):
        for normalize in (True, False):
            rc, got = sample_is(rp, 2, BATCH, k, 1, [9, 9], beta, N, normalize)
            assert rc == _lib.MZS_OK
            want = isref.weights([9, 9], eps, BATCH, k, 1, beta=beta, normalize=normalize)
            if zero_rows:
                assert (got["serial"] == -1).all() and (got["start"] == -1).all()
                assert not got["isw"].view(np.uint32).any() and not want["isw"].any()
                for n in FIELDS[:8]:
                    assert not got[n].view(np.uint8).any(), n
            else:
                assert (got["serial"] == serial[1]).all() and np.array_equal(got["start"], want["start"])
                assert _ulps(got["isw"], want["isw"]).max() <= (0 if beta == 1.0 else 1)


def test_sample_is_refuses_bad_arguments_and_writes_nothing():
    rp, eps, serial = _case((9, 9), 8, "dyadic")
    for beta, N, normalize, scratch in ((-0.25, 2, 1, True), (1.5, 2, 1, True), (float("nan"), 2, 0, True),
                                        (float("inf"), 2, 0, True), (0.5, 0, 1, True), (0.5, float("nan"), 1, True),
                                        (0.5, float("inf"), 0, True), (0.5, 2, 1, False)):
        rc, got = sample_is(rp, 2, 5, 8, 1, [1, 1], beta, N, normalize, with_scratch=scratch)
        assert rc == _lib.MZS_E_INVALID, (beta, N, normalize, scratch)
        assert (got["isw"].view(np.uint32) == 0x7FC5A5A5).all() and (got["start"].view(np.uint32) == 0x5A5A5A5A).all()
    rc, got = sample_is(rp, 2, 5, 8, 1, [1, 1], 0.5, 2, 0, with_scratch=False)  # no normalisation: no scratch needed
    assert rc == _lib.MZS_OK and np.isfinite(got["isw"]).all()


# ---- 2. the fused step with a weight per row ----
STEP_SHAPES = {"listed": (2, 8, 4, 19, 3), "narrow on demand": (5, 8, 4, 17, 2), "wide on demand": (17, 8, 4, 19, 2)}
SUPPORT = 10  # F = 21


def _fused(m):
    f = mx.loss.FusedLossGrad(m)
    shape = (f.A, f.E, 2 * f.S + 1)
    if shape != (2, 8, 21):
        ok = _jit.ensure_wide_train_instance(*shape) if f.A > 16 else _jit.ensure_train_instance(*shape)
        assert ok, _jit.build_log_tail()
    return f


def _autograd64(m, b, sw):
    """fp64 autograd of default_loss_fn(sample_weight=) on a float64 copy of the nets, on the CPU."""
    mods = [copy.deepcopy(x).to(device="cpu", dtype=torch.float64) for x in m.network]
    m64 = mx.MuZero(mx.nn.MZNetwork(*mods), device="cpu")
    m64._params, m64._support_size = True, m._support_size
    loss = mx.loss.default_loss_fn(m64, b, sample_weight=sw)
    assert loss.dtype == torch.float64
    loss.backward()
    w = mx.nn.mlp_trio_weights(m64.network)
    return float(loss.detach()), [w[n].grad.numpy() for n in MLP_WEIGHT_NAMES]


def _call(fused, b, sw=None):
    loss, flat = fused(b, sample_weight=sw)
    torch.cuda.synchronize()
    return loss.clone(), flat.clone()


@pytest.mark.parametrize("name", list(STEP_SHAPES))
def test_weighted_step(name):
    A, E, obs_dim, B, L = STEP_SHAPES[name]
    m = train_model(A, E, obs_dim, seed=A + B, support=SUPPORT)
    b = train_batch(B, L, A, obs_dim, seed=A + B)
    fused = _fused(m)
    rng = np.random.default_rng(B)
    sw = rng.permutation(np.linspace(0.05, 1.0, B)).astype(F32)  # distinct: row 16 + i must not read row i's weight
    assert len(set(sw[:3]) | set(sw[16:19][:B - 16])) == 3 + min(3, B - 16)

    # (a) weights of one: the unweighted entry's bits
    loss0, flat0 = _call(fused, b)
    loss1, flat1 = _call(fused, b, torch.ones(B, device="cuda"))
    assert torch.equal(loss0, loss1) and torch.equal(flat0, flat1)

    # (b) against fp64 autograd of the weighted torch loss; NumPy weights are uploaded, device ones read in place
    loss, flat = _call(fused, b, sw)
    loss_d, flat_d = _call(fused, b, torch.as_tensor(sw, device="cuda"))
    assert torch.equal(loss, loss_d) and torch.equal(flat, flat_d) and not torch.equal(flat, flat0)
    views = [v.detach().cpu().double().numpy() for v in fused.views]
    l64, g64 = _autograd64(m, b, sw)
    lk = abs(float(loss) - l64) / abs(l64)
    errs = [float(np.abs(g - d).max() / max(np.abs(d).max(), 1e-6)) for g, d in zip(views, g64)]
    l64_plain, _ = _autograd64(m, b, None)
    print(f"[{name}: loss {lk:.1e} grad {max(errs):.1e}; unweighted loss is {abs(l64_plain - l64) / abs(l64):.1e} away]",
          end=" ")
    assert abs(l64_plain - l64) > 1e-2 * abs(l64)
    assert lk <= 1e-5, (float(loss), l64)
    for n, e in zip(MLP_WEIGHT_NAMES, errs):
        assert e <= 2e-4, (n, e)

    # (c) weight 0 on the last live row: whatever finite data it holds, it adds exact zeros
    sw0 = sw.copy()
    sw0[B - 1] = 0.0
    loss_a, flat_a = _call(fused, b, sw0)
    other = train_batch(B, L, A, obs_dim, seed=1000 + B)
    b2 = mx.Transition(**{f: np.array(getattr(b, f)) for f in ("obs", "a", "r", "Rn", "pi")})
    for f in ("obs", "a", "r", "Rn", "pi"):
        getattr(b2, f)[B - 1] = getattr(other, f)[B - 1]
    assert not np.array_equal(b2.obs[B - 1], b.obs[B - 1]) and np.array_equal(b2.obs[:B - 1], b.obs[:B - 1])
    loss_b, flat_b = _call(fused, b2, sw0)
    assert torch.equal(loss_a, loss_b) and torch.equal(flat_a.view(torch.int32), flat_b.view(torch.int32))
    loss_c, flat_c = _call(fused, b2, sw)  # (with its weight back, the row's data matters)
    assert not torch.equal(flat_c, flat)

    # a shape other than [B] is refused before any launch
    for bad in (np.ones(B + 1, F32), torch.ones(B, 1, device="cuda"), 1.0):
        with pytest.raises(ValueError, match="sample_weight"):
            fused(b, sample_weight=bad)


def test_weighted_entry_refuses_null_weights():
    m = train_model(2, 8, 4, seed=1, support=SUPPORT)
    b = train_batch(4, 2, 2, 4, seed=1)
    fused = mx.loss.FusedLossGrad(m)
    fused(b)
    L = _lib.load()
    assert L.mzs_mlp_loss_grad_weighted(None, None, None, None) == _lib.MZS_E_INVALID
    assert b"sample_weight" in L.mzs_last_error(None)


# ---- 3. the public route ----
def _buffer(lengths, seed, obs_dim=4, A=2):
    rng = np.random.default_rng(seed)
    trs, eps = [], []
    for T in lengths:
        ep = rr.make_episode(rng, T, A, obs_dim, w=rr.dyadic_weights(rng, T) + 2.0 ** -10)
        eps.append(ep)
        trs.append(mx.Trajectory.from_arrays(ep["obs"], ep["a"].astype(np.int64), ep["r"].astype(np.float64), ep["done"],
                                             ep["Rn"].astype(np.float64), ep["v"].astype(np.float64), ep["pi"][:, None],
                                             ep["w"]))
    buf = mx.DeviceReplayBuffer(8, 64, random_seed=seed)
    buf.add_many(trs, [ep["weight"] for ep in eps])
    return buf, eps


def test_sample_is_beta_returns_the_same_batch_and_the_key_stream_is_unchanged():
    lengths, k = (3, 7, 12, 5), 4
    buf, eps = _buffer(lengths, seed=5)
    twin, _ = _buffer(lengths, seed=5)
    assert buf.eligible_windows(k) == 12
    key = [11, 12]
    plain, (serial, start) = buf.sample(num_trajectory=7, sample_per_trajectory=3, k_steps=k, key=key, with_indices=True)
    for beta, normalize in ((1.0, True), (0.4, True), (0.0, False), (1.0, False)):
        got = buf.sample(num_trajectory=7, sample_per_trajectory=3, k_steps=k, key=key, with_indices=True, is_beta=beta,
                         is_normalize=normalize)
        assert len(got) == 3
        batch, (serial2, start2), isw = got
        assert torch.equal(serial, serial2) and torch.equal(start, start2)
        for f in ("obs", "a", "r", "done", "Rn", "v", "pi", "w"):
            assert torch.equal(getattr(batch, f), getattr(plain, f)), f
        assert isw.shape == (21,) and isw.dtype == torch.float32 and isw.is_cuda
        want = isref.weights(key, eps, 21, k, 3, beta=beta, normalize=normalize)
        assert np.array_equal(start.cpu().numpy(), want["start"])
        assert _ulps(isw.cpu().numpy(), want["isw"]).max() <= (1 if beta == 0.4 else 0)
        pair = buf.sample(num_trajectory=7, sample_per_trajectory=3, k_steps=k, key=key, is_beta=beta,
                          is_normalize=normalize)
        assert len(pair) == 2 and torch.equal(pair[1], isw) and torch.equal(pair[0].Rn, plain.Rn)
    # the buffer's own key: a call with is_beta advances it exactly as one without
    a1 = buf.sample(5, k_steps=k, is_beta=0.5)[0]
    a2 = twin.sample(5, k_steps=k)
    b1, b2 = buf.sample(5, k_steps=k), twin.sample(5, k_steps=k)
    assert torch.equal(a1.obs, a2.obs) and torch.equal(b1.obs, b2.obs) and torch.equal(b1.Rn, b2.Rn)


def test_update_with_the_sampled_weights_matches_the_torch_route():
    """(d): sample(is_beta=1.0) -> update(sample_weight=isw) on the kernel against the torch route, the step's bars."""
    buf, _ = _buffer((3, 7, 12, 5, 9), seed=6)
    batch, isw = buf.sample(num_trajectory=19, k_steps=3, key=[2, 3], is_beta=1.0)
    assert 0 < float(isw.min()) < float(isw.max()) == 1.0
    res = {}
    for backend in ("hip", "torch"):
        m = train_model(2, 8, 4, seed=31, support=SUPPORT, optimizer=("sgd", 1e-2))
        w, seen = mx.nn.mlp_trio_weights(m.network), []
        # (the optimiser's step clears the gradients: read them in its place)
        m._optimizer.step = lambda: seen.extend(w[n].grad.detach().cpu().double().numpy().copy() for n in MLP_WEIGHT_NAMES)
        loss = m.update(batch, sample_weight=isw, backend=backend)["loss"]
        assert len(seen) == len(MLP_WEIGHT_NAMES)
        res[backend] = (loss, seen)
    plain = train_model(2, 8, 4, seed=31, support=SUPPORT, optimizer=("sgd", 1e-2)).update(batch, backend="hip")["loss"]
    (lh, gh), (lt, gt) = res["hip"], res["torch"]
    errs = [float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-6)) for x, y in zip(gh, gt)]
    print(f"[update hip against torch: loss {abs(lh - lt) / abs(lt):.1e} grad {max(errs):.1e}]", end=" ")
    assert np.isfinite(lh) and abs(lh - lt) <= 1e-5 * abs(lt) and abs(plain - lt) > 1e-3 * abs(lt)
    for n, e in zip(MLP_WEIGHT_NAMES, errs):
        assert e <= 2e-4, (n, e)
    m = train_model(2, 8, 4, seed=31, support=SUPPORT)
    with pytest.raises(ValueError, match="sample_weight"):
        m.update(batch, sample_weight=isw[:-1], backend="hip")


# ---- 4. the loop ----
def _fit_vector_once(seed, **kw):
    """The arguments of test_gpu_replay.py's _fit_vector_once with two iterations, plus `kw`."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    from cartpole_env import VectorCartPole
    g = torch.Generator().manual_seed(0)
    net = mx.nn.MZNetwork(mx.nn.Representation(8, generator=g), mx.nn.Prediction(2, 21, generator=g),
                          mx.nn.Dynamic(8, 2, 21, generator=g))
    model = mx.MuZero(net, optimizer=mx.optimizers.create_optimizer("adam", 5e-3))
    buf, rows = mx.DeviceReplayBuffer(64, 4096, random_seed=seed), []
    mx.fit_vector(model, VectorCartPole(16, seed=0), VectorCartPole(2, max_episode_steps=20, seed=1), n_step=3, buffer=buf,
                  iterations=2, steps_per_iteration=8, num_simulations=8, k_steps=3, num_trajectory=8,
                  sample_per_trajectory=2, num_update_per_iteration=2, test_interval=10, random_seed=3, metrics=rows, **kw)
    for r in rows:
        r.pop("collect_s")
    return model, buf, rows


def test_fit_vector_with_is_beta():
    _, buf, rows = _fit_vector_once(13, is_beta=0.4, priority_update=True)
    losses = [r["loss"] for r in rows if "loss" in r]
    assert len(rows) == 2 and losses and np.isfinite(losses).all() and len(buf) > 0
    _, _, rows0 = _fit_vector_once(13)
    _, _, rows1 = _fit_vector_once(13, is_beta=None)
    assert rows0 == rows1 and [r.get("loss") for r in rows0] != [r.get("loss") for r in rows]
