"""GPU tests of per-step observations through the public interface: `DeviceReplayBuffer.sample(all_obs=True)` against
the call without it and against the stored episodes; the fused stochastic training step on a device-sampled batch
against the same rows handed over as the host buffer hands them; and `fit_vector` with a stochastic `MuZero` on
`Device2048` and a `DeviceReplayBuffer`, which the loss refused before the buffer had every step's observation.

Everything sampled is a copy and is compared with ==; the two update() calls read the same float32 numbers (dyadic
rewards and values, gamma 0.5: every return is exact on both routes) and must return the same loss bits."""
import numpy as np
import pytest
import torch

import muax_amd as mx
import stochastic_train_reference as stref

pytestmark = pytest.mark.gpu
K, N_STEP, GAMMA = 5, 3, 0.5
SHIFT = 6


def _stream(rng, lengths, A, od):
    M = sum(lengths)
    return dict(obs=rng.uniform(-1, 1, (M, od)).astype(np.float32), a=rng.integers(0, A, M),
                r=rng.integers(-16, 17, M) / 8.0, v=rng.integers(-64, 65, M) / 8.0,
                pi=rng.dirichlet(np.ones(A), M).astype(np.float32))


def _filled(lengths, A, od, seed):
    st = _stream(np.random.default_rng(seed), lengths, A, od)
    buf = mx.DeviceReplayBuffer(16, 1024, random_seed=seed)
    buf.add_raw(st["obs"], st["a"], st["r"], st["v"], st["pi"], lengths, N_STEP, GAMMA, 0.5, weight="sum")
    return buf, st


@pytest.mark.parametrize("od", [3, 16, 65])
@pytest.mark.parametrize("num_trajectory,spt", [(9, 1), (3, 3), (1, 1)])
def test_sample_all_obs_changes_obs_alone(num_trajectory, spt, od):
    buf, _ = _filled([K + 1, 30, K, 71, 2], 3, od, seed=od)
    kw = dict(num_trajectory=num_trajectory, k_steps=K, sample_per_trajectory=spt, key=(12, od))
    B = num_trajectory * spt
    plain = buf.sample(**kw)
    assert plain.obs.shape == (B, 1, od)  # the default return value
    for extra in ({}, {"with_indices": True}, {"is_beta": 0.5}, {"with_indices": True, "is_beta": 1.0}):
        a, b = buf.sample(**kw, **extra), buf.sample(**kw, **extra, all_obs=True)
        a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
        assert len(a) == len(b)
        assert b[0].obs.shape == (B, K, od) and b[0].obs.dtype == torch.float32 and b[0].obs.is_cuda
        assert torch.equal(b[0].obs[:, 0], a[0].obs[:, 0]) and torch.equal(a[0].obs, plain.obs)
        for n in ("a", "r", "done", "Rn", "v", "pi", "w"):
            x, y = getattr(a[0], n), getattr(b[0], n)
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), n
        if "with_indices" in extra:
            assert torch.equal(a[1][0], b[1][0]) and torch.equal(a[1][1], b[1][1])
        if "is_beta" in extra:
            assert torch.equal(a[-1].view(torch.int32), b[-1].view(torch.int32))
    batch, (serial, start) = buf.sample(**kw, with_indices=True, all_obs=True)
    obs = batch.obs.cpu().numpy()
    for j, (s, i) in enumerate(zip(serial.tolist(), start.tolist())):
        want = buf.episode(s).obs[i:i + K].cpu().numpy()
        assert want.shape == (K, od) and np.array_equal(obs[j].view(np.uint32), want.view(np.uint32)), j


def test_fused_stochastic_update_device_batch_equals_host_batch():
    """The listed instance (A, C, E, F) = (3, 2, 4, 17), obs_dim 5: update() on a batch sampled on the device with every
    observation, and on the same rows cut from host Trajectories the way TrajectoryReplayBuffer.sample cuts them."""
    A, Cn, E, support, od = stref.SHAPES[0]
    assert (A, Cn, E, 2 * support + 1) == (3, 2, 4, 17)
    lengths = [K + 1, 30, 9, 17]
    buf, st = _filled(lengths, A, od, seed=4)
    first = np.concatenate([[0], np.cumsum(lengths)])
    trajs = [mx.episode_trajectory(*(st[n][first[e]:first[e + 1]] for n in ("obs", "a", "r", "v", "pi")), N_STEP, GAMMA, 0.5)
             for e in range(len(lengths))]
    batch, (serial, start) = buf.sample(num_trajectory=17, k_steps=K, key=3, with_indices=True, all_obs=True)
    assert batch.obs.shape == (17, K, od)
    rows = [tuple(c[:, i:i + K] for c in tuple(trajs[s].batched_transitions))  # (serials count from 0 in a new buffer)
            for s, i in zip(serial.tolist(), start.tolist())]
    host = mx.Transition(*(np.concatenate(c) for c in zip(*rows)))
    assert np.asarray(host.obs).shape == (17, K, od)
    assert np.array_equal(np.asarray(host.obs, np.float32), batch.obs.cpu().numpy())
    assert np.array_equal(np.asarray(host.Rn, np.float32).reshape(17, K), batch.Rn.cpu().numpy())
    out = []
    for b in (batch, host):
        m = stref.smz_model(A, Cn, E, support, od, seed=21, stochastic_fused_update=True)
        loss = m.update(b)["loss"]
        assert m._last_update_route == "hip_stochastic_fused"
        out.append((loss, torch.cat([p.detach().reshape(-1) for mod in m.network for p in mod.parameters()])))
    assert np.isfinite(out[0][0]) and out[0][0] == out[1][0]
    assert torch.equal(out[0][1], out[1][1])  # ... and the same step
    with pytest.raises(ValueError, match="needs every step's observation"):
        stref.smz_model(A, Cn, E, support, od, seed=21, stochastic_fused_update=True).update(
            buf.sample(num_trajectory=17, k_steps=K, key=3))


def _fit(device_plan, rows, fused=True, **kw):
    A, Cn, E, support, od = stref.SHAPES[1]  # 4 actions, obs_dim 16: Device2048's; a listed training instance
    model = stref.smz_model(A, Cn, E, support, od, seed=5, policy="stochastic", stochastic_fused_update=fused)
    buf = mx.DeviceReplayBuffer(64, 4096, random_seed=13)
    mx.fit_vector(model, mx.Device2048(8, max_episode_steps=6, seed=1, reward_shift=SHIFT),
                  mx.Device2048(2, max_episode_steps=5, seed=2, reward_shift=SHIFT), n_step=3, buffer=buf, iterations=2,
                  steps_per_iteration=6, num_simulations=4, k_steps=3, num_trajectory=8, sample_per_trajectory=2,
                  num_update_per_iteration=3, test_interval=10, random_seed=3, metrics=rows, device_collect=True,
                  device_plan=device_plan, **kw)
    return model, buf


@pytest.mark.parametrize("device_plan", [False, True])
def test_fit_vector_trains_a_stochastic_model_from_the_device_buffer(device_plan):
    rows = []
    model, buf = _fit(device_plan, rows)
    assert len(rows) == 2 and all(np.isfinite(r["loss"]) for r in rows) and rows[-1]["training_step"] == 6
    assert all(r["episodes"] == 8 for r in rows) and np.isfinite(rows[0]["test_G"])
    assert model._last_route in ("hip_stochastic_mlp", "hip_stochastic_one_launch")
    assert model._last_update_route == "hip_stochastic_fused"
    assert len(buf) == 16


def test_fit_vector_stochastic_with_reanalysis_priorities_and_weights():
    """reanalyse_every (the environment's masks), the priority write-back and is_beta, on the autograd route."""
    rows = []
    model, buf = _fit(True, rows, fused=False, reanalyse_every=1, priority_update=True, is_beta=0.5)
    assert len(rows) == 2 and all(np.isfinite(r["loss"]) for r in rows)
    assert model._last_route == "hip_stochastic_mlp" and model._last_update_route == "torch"
    with pytest.raises(ValueError, match="priority_steps.*SMZNetwork"):
        _fit(True, [], priority_update=True, priority_steps=2)
