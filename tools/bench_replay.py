"""Replay sampling beside the training step: `TrajectoryReplayBuffer.sample` + `update()` (host lists and NumPy
slices, five uploads per batch) against `DeviceReplayBuffer.sample` + `update()` (one launch, the batch read in place),
and each `sample` on its own.  Default MLP trio on CartPole shapes, 500 stored episodes of about 200 steps.

    python tools/bench_replay.py [--iters 200] [--episodes 500] [--shape NUM_TRAJECTORY,K ...] [--all-obs] [--obs-dim 4]
    python tools/bench_replay.py --reanalyse [--iters 200] [--episodes 500]
    python tools/bench_replay.py --priorities [--prio-steps KP] [--iters 200] [--episodes 500] [--shape NUM_TRAJECTORY,K ...]
    python tools/bench_replay.py --is-weights [--is-beta 0.4] [--iters 200] [--episodes 500] [--shape NUM_TRAJECTORY,K ...]

`--all-obs` (the default mode): the device columns sample with `all_obs=True`, every step's observation
([B, k, obs_dim]) in the same launch; `--obs-dim` sets the observation width of the stored episodes and the model (16 is
2048's).  The host buffer returns every row anyway.

`--reanalyse` times, on the same device buffer and with 50 simulations, (a) `DeviceReplayBuffer.reanalyse()` of the
whole buffer, (b) the same work through the host -- `episode().obs` downloaded, `act` NumPy in / out in the same
chunks, `vector.episode_trajectory`, `add_many` into a second buffer -- and (c) the `act()` chunks of (a) alone.

`--priorities` times, on the device buffer alone, the training step with the priority write-back --
`sample(with_indices=True)` + `update()` + `vector.value_priorities` + `update_priorities` -- beside `sample`,
`sample` + `update()` and `update()` as the default mode times them, and the two new parts on their own.  Side by side
with it, for `--prio-steps` kp (default: k) priorities per window: `MuZero.unroll_values` on the torch modules and as one
kernel launch (`backend="torch"` / `"hip"`), the write-back of [B, kp] priorities, and the whole step with each.

`--is-weights` times, on the device buffer alone, `sample(is_beta=)` (the sample launch and the normalisation pass)
beside `sample()`, and `update(sample_weight=)` beside `update()` on one fixed batch, both on the fused kernel.

Every figure is the median of `--iters` iterations, each ending in a device synchronise, after 30 ms of untimed
iterations of the same work (clocks settled).  The two routes alternate shape by shape in one process."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import muax_amd as mx  # noqa: E402
from muax_amd.utils import warm_runtime  # noqa: E402

A, E, OBS, SUPPORT = 2, 8, 4, 10


def median_ms(fn, iters, settle_ms=30.0):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < settle_ms:
        fn()
        torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def model():
    g = torch.Generator().manual_seed(0)
    net = mx.nn.MZNetwork(mx.nn.Representation(E, generator=g), mx.nn.Prediction(A, 2 * SUPPORT + 1, generator=g),
                          mx.nn.Dynamic(E, A, 2 * SUPPORT + 1, generator=g))
    m = mx.MuZero(net, support_size=SUPPORT)
    m.init(0, np.zeros((1, OBS)))
    return m


def episodes(n, rng):
    out = []
    for T in rng.integers(150, 251, n):
        w = np.abs(rng.standard_normal(T)) ** 0.5
        out.append(mx.Trajectory.from_arrays(rng.uniform(-1, 1, (T, OBS)).astype(np.float32), rng.integers(0, A, T),
                                             np.ones(T), rng.uniform(size=T) < 0.05, rng.uniform(0, 20, T),
                                             rng.uniform(0, 20, T), rng.dirichlet(np.ones(A), T).astype(np.float32)[:, None],
                                             w))
    return out


def reanalyse_figures(dev, iters, simulations=50, chunk_rows=4096, n=10, gamma=0.997, alpha=0.5):
    from muax_amd import prng, vector
    from muax_amd.replay_device import reanalyse_plan
    m = model()
    serials = dev.serials
    lengths = [len(dev.episode(s).a) for s in serials]
    plan = reanalyse_plan(lengths, chunk_rows)
    keys = prng.split(prng.PRNGKey(0), plan.n_chunks)
    act_kw = dict(with_pi=True, with_value=True, obs_from_batch=True, num_simulations=simulations)
    stream = torch.zeros((plan.rows_padded, OBS), device="cuda")
    stream[:plan.stream_rows] = torch.cat([dev.episode(s).obs for s in serials])

    def on_device():
        dev.reanalyse(m, 0, n, gamma, alpha, chunk_rows=chunk_rows, num_simulations=simulations)

    def acts_alone():
        for c in range(plan.n_chunks):
            m.act(keys[c], stream[c * chunk_rows:(c + 1) * chunk_rows], device_outputs=True, **act_kw)

    def through_the_host():
        eps = [dev.episode(s) for s in serials]
        obs = [e.obs.cpu().numpy() for e in eps]
        flat = np.concatenate(obs + [np.zeros((plan.rows_padded - plan.stream_rows, OBS), np.float32)])
        pi, v = [], []
        for c in range(plan.n_chunks):
            _, p, x = m.act(keys[c], flat[c * chunk_rows:(c + 1) * chunk_rows], **act_kw)
            pi.append(p), v.append(x)
        pi, v = np.concatenate(pi), np.concatenate(v)
        trs = []
        for e, o, first, T in zip(eps, obs, plan.offsets, lengths):
            trs.append(vector.episode_trajectory(o, e.a.cpu().numpy(), e.r.cpu().numpy(), v[first:first + T],
                                                 pi[first:first + T], n, gamma, alpha))
        second = mx.DeviceReplayBuffer(len(eps), plan.stream_rows)
        second.add_many(trs, [t.weights.mean() for t in trs])

    ta = median_ms(on_device, iters)
    tc = median_ms(acts_alone, iters)
    tb = median_ms(through_the_host, max(3, iters // 20), settle_ms=0.0)
    print(f"reanalysis of {len(serials)} episodes, {plan.stream_rows} transitions: {plan.n_chunks} act() chunks of "
          f"{chunk_rows} roots, {simulations} simulations; median of {iters} synchronised iterations "
          f"({max(3, iters // 20)} for the host route), ms")
    print(f"(a) reanalyse() on the device          {ta:9.3f}")
    print(f"(b) through the host and a second buffer {tb:7.3f}   ({tb / ta:.1f}x (a))")
    print(f"(c) the act() chunks alone             {tc:9.3f}   ({tc / plan.n_chunks:.3f} per chunk)")
    print(f"(a) - (c): gather, copies, write-back  {ta - tc:9.3f}   ({100 * (ta - tc) / ta:.1f} % of (a))", flush=True)


def priority_figures(dev, shapes, iters, prio_steps=None, alpha=0.5):
    from muax_amd.vector import unroll_value_priorities, value_priorities
    print(f"{'num_trajectory x k':>18} | {'dev sample':>10} {'dev s+upd':>9} {'update':>7} | {'value_prio':>10} "
          f"{'update_prio':>11} | {'s+upd+prio':>10} | {'s+upd+prio / s+upd':>18}")
    unrolled = []
    for n, k in shapes:
        m_dev, m_pri = model(), model()
        fixed, indices = dev.sample(num_trajectory=n, k_steps=k, with_indices=True)
        prio = value_priorities(m_pri, fixed)
        kp = min(prio_steps or k, k)
        prio_kp = unroll_value_priorities(m_pri, fixed, kp, backend="hip")

        def step_with_priorities():
            batch, idx = dev.sample(num_trajectory=n, k_steps=k, with_indices=True)
            m_pri.update(batch, backend="hip")
            dev.update_priorities(idx, value_priorities(m_pri, batch), alpha=alpha)

        def step_unrolled(backend):
            def step():
                batch, idx = dev.sample(num_trajectory=n, k_steps=k, with_indices=True)
                m_pri.update(batch, backend="hip")
                dev.update_priorities(idx, unroll_value_priorities(m_pri, batch, kp, backend=backend), alpha=alpha)
            return step

        res = {
            "ds": median_ms(lambda: dev.sample(num_trajectory=n, k_steps=k), iters),
            "du": median_ms(lambda: m_dev.update(dev.sample(num_trajectory=n, k_steps=k), backend="hip"), iters),
            "u": median_ms(lambda: m_dev.update(fixed, backend="hip"), iters),
            "vp": median_ms(lambda: value_priorities(m_pri, fixed), iters),
            "up": median_ms(lambda: dev.update_priorities(indices, prio, alpha=alpha), iters),
            "dp": median_ms(step_with_priorities, iters),
        }
        print(f"{n:>13} x {k:<2} | {res['ds']:10.3f} {res['du']:9.3f} {res['u']:7.3f} | {res['vp']:10.3f} "
              f"{res['up']:11.3f} | {res['dp']:10.3f} | {res['dp'] / res['du']:17.2f}x", flush=True)
        unrolled.append((n, k, kp, res["vp"], res["dp"], res["du"], {
            "ut": median_ms(lambda: m_pri.unroll_values(fixed, kp, backend="torch"), iters),
            "uh": median_ms(lambda: m_pri.unroll_values(fixed, kp, backend="hip"), iters),
            "upk": median_ms(lambda: dev.update_priorities(indices, prio_kp, alpha=alpha), iters),
            "st": median_ms(step_unrolled("torch"), iters),
            "sh": median_ms(step_unrolled("hip"), iters),
        }))
    print(f"\n{'num_trajectory x k':>18} | {'kp':>2} | {'value_prio [B]':>14} {'unroll torch':>12} {'unroll hip':>10} | "
          f"{'update_prio kp':>14} | {'step [B]':>8} {'step torch':>10} {'step hip':>8} | {'step hip / s+upd':>16}")
    for n, k, kp, vp, dp, du, r in unrolled:
        print(f"{n:>13} x {k:<2} | {kp:>2} | {vp:14.3f} {r['ut']:12.3f} {r['uh']:10.3f} | {r['upk']:14.3f} | "
              f"{dp:8.3f} {r['st']:10.3f} {r['sh']:8.3f} | {r['sh'] / du:15.2f}x", flush=True)


def is_weight_figures(dev, shapes, iters, beta):
    print(f"{'num_trajectory x k':>18} | {'sample':>8} {'sample is':>9} {'is, raw':>8} | {'update':>8} {'update w':>8} | "
          f"{'sample is - sample':>18} {'update w - update':>17}")
    for n, k in shapes:
        m_plain, m_w = model(), model()
        fixed, isw = dev.sample(num_trajectory=n, k_steps=k, is_beta=beta)
        res = {
            "s": median_ms(lambda: dev.sample(num_trajectory=n, k_steps=k), iters),
            "si": median_ms(lambda: dev.sample(num_trajectory=n, k_steps=k, is_beta=beta), iters),
            "sr": median_ms(lambda: dev.sample(num_trajectory=n, k_steps=k, is_beta=beta, is_normalize=False), iters),
            "u": median_ms(lambda: m_plain.update(fixed, backend="hip"), iters),
            "uw": median_ms(lambda: m_w.update(fixed, sample_weight=isw, backend="hip"), iters),
        }
        print(f"{n:>13} x {k:<2} | {res['s']:8.3f} {res['si']:9.3f} {res['sr']:8.3f} | {res['u']:8.3f} {res['uw']:8.3f} | "
              f"{res['si'] - res['s']:18.3f} {res['uw'] - res['u']:17.3f}", flush=True)


def main():
    global OBS
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reanalyse", action="store_true", help="time reanalysis instead of sampling")
    ap.add_argument("--priorities", action="store_true", help="time the training step with the priority write-back")
    ap.add_argument("--prio-steps", type=int, default=None, metavar="KP",
                    help="with --priorities: priorities per window of the unrolled routes (default: k)")
    ap.add_argument("--is-weights", action="store_true",
                    help="time sample(is_beta=) beside sample() and update(sample_weight=) beside update()")
    ap.add_argument("--is-beta", type=float, default=0.4, help="with --is-weights: the exponent (default 0.4)")
    ap.add_argument("--all-obs", action="store_true",
                    help="default mode: the device columns sample every step's observation (all_obs=True)")
    ap.add_argument("--obs-dim", type=int, default=OBS, help="observation width (default 4, CartPole's)")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--episodes", type=int, default=500)
    ap.add_argument("--shape", action="append", default=[], metavar="NUM_TRAJECTORY,K")
    a = ap.parse_args()
    OBS = a.obs_dim
    obs_kw = {"all_obs": True} if a.all_obs else {}
    shapes = [tuple(int(x) for x in s.split(",")) for s in a.shape] or [(32, 10), (4096, 10)]
    warm_runtime()
    eps = episodes(a.episodes, np.random.default_rng(0))
    host = mx.TrajectoryReplayBuffer(a.episodes, random_seed=0)
    dev = mx.DeviceReplayBuffer(a.episodes, sum(len(t) for t in eps), random_seed=0)
    for t in eps:
        host.add(t, t.weights.mean())
    t0 = time.perf_counter()
    dev.add_many(eps, [t.weights.mean() for t in eps])
    torch.cuda.synchronize()
    print(f"{a.episodes} episodes, {dev.steps} transitions; add_many: {(time.perf_counter() - t0) * 1e3:.1f} ms "
          f"(one upload, one launch); median of {a.iters} synchronised iterations, ms")
    if a.reanalyse:
        reanalyse_figures(dev, a.iters)
        return
    if a.priorities:
        priority_figures(dev, shapes, a.iters, a.prio_steps)
        return
    if a.is_weights:
        is_weight_figures(dev, shapes, a.iters, a.is_beta)
        return
    if a.all_obs:
        print(f"device columns with all_obs=True: obs [B, k, {OBS}]")
    print(f"{'num_trajectory x k':>18} | {'host sample':>11} {'host s+upd':>10} | {'dev sample':>10} {'dev s+upd':>9} | "
          f"{'update':>7} | {'s+upd host/dev':>14} {'sample host/dev':>15}")
    for n, k in shapes:
        m_host, m_dev = model(), model()
        fixed = dev.sample(num_trajectory=n, k_steps=k, **obs_kw)
        res = {
            "hs": median_ms(lambda: host.sample(num_trajectory=n, k_steps=k), a.iters),
            "hu": median_ms(lambda: m_host.update(host.sample(num_trajectory=n, k_steps=k), backend="hip"), a.iters),
            "ds": median_ms(lambda: dev.sample(num_trajectory=n, k_steps=k, **obs_kw), a.iters),
            "du": median_ms(lambda: m_dev.update(dev.sample(num_trajectory=n, k_steps=k, **obs_kw), backend="hip"), a.iters),
            "u": median_ms(lambda: m_dev.update(fixed, backend="hip"), a.iters),
        }
        print(f"{n:>13} x {k:<2} | {res['hs']:11.3f} {res['hu']:10.3f} | {res['ds']:10.3f} {res['du']:9.3f} | "
              f"{res['u']:7.3f} | {res['hu'] / res['du']:13.1f}x {res['hs'] / res['ds']:14.1f}x", flush=True)


if __name__ == "__main__":
    main()
