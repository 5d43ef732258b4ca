"""2048 with Stochastic MuZero: `muax.Device2048` stepped on the device, every act() the stochastic search over chance
nodes (4 actions + 32 chance codes) on the default stochastic MLP family -- the decision and the chance function
evaluated by the library, one launch per simulation --, training with `loss.stochastic_loss_fn` (on torch autograd, or
with --fused-update on the fused training kernel of this shape).

The default route is the project's own loop: `fit_vector(device_collect=True, device_plan=True)` on a
`DeviceReplayBuffer`.  The episodes are cut and stored on the device, every batch is one `sample(all_obs=True)` launch
-- the loss encodes a chance code from EVERY step's observation -- and only the rows of the finished-episode plan come
to the host.  `update_s` is the time from an iteration's first sample() to the end of its last update().

--host-buffer is the comparison route, a short loop of this file's own: the step loop runs on the device with no
per-step host copy (observation, mask, action, search policy, value, reward and flag stay device tensors), the
iteration's stream comes down once, is cut into finished episodes (`episode_trajectory`) and goes into a host
`TrajectoryReplayBuffer`, whose batches are uploaded again.

Nothing here has been run to a result: whether this recipe learns 2048 is not known.

    python examples/fit_2048_stochastic.py [--envs 256] [--steps 64] [--iterations 3] [--updates 20] [--one-launch]
                                           [--root-in-kernel] [--fused-update] [--priority-steps K] [--host-buffer]

--priority-steps K (the device route): after every update() the value errors of the first K transitions of every sampled
window are written back as priorities (`fit_vector(priority_update=True, priority_steps=K)`), from
`MuZero(stochastic_unroll_values=True).unroll_values`: one launch for this family.
"""
import argparse
import functools
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import muax_amd as muax  # noqa: E402


def collect(model, venv, obs, key, steps, num_simulations, pending, n_step, gamma):
    """`steps` lock-step device steps -> (finished episodes as Trajectories, the next observation, the key)."""
    N, dev = venv.n, venv.device
    r_d = torch.empty(N, dtype=torch.float64, device=dev)
    done_d = torch.empty(N, dtype=torch.uint8, device=dev)
    rows = []
    for _ in range(steps):
        key, sub = muax.prng.split(key)
        a, pi, v = model.act(sub, obs, with_pi=True, with_value=True, obs_from_batch=True, num_simulations=num_simulations,
                             invalid_actions=venv.invalid_actions_device(), device_outputs=True)
        seen = obs.clone()  # (the environment rewrites its observation buffer in place)
        obs = venv.step_device(a, r_d, done_d)
        rows.append((seen, a, r_d.clone(), v, pi, done_d.clone()))
    O, A, R, V, P, D = (torch.stack(x).cpu().numpy() for x in zip(*rows))  # one synchronisation per iteration
    out = []
    for e in range(N):
        lo = 0
        for t in np.flatnonzero(D[:, e]).tolist() + [steps]:
            part = [x[lo:t + 1, e] if t < steps else x[lo:, e] for x in (O, A, R, V, P)]
            if pending[e] is not None:
                part = [np.concatenate([p, q]) for p, q in zip(pending[e], part)]
                pending[e] = None
            if t < steps:
                out.append(muax.episode_trajectory(*part, n_step, gamma, alpha=0.5))
            elif len(part[0]):
                pending[e] = part
            lo = t + 1
    return out, obs, key


class _Report(list):
    """fit_vector's metrics rows, printed as they arrive in the form of the host route's lines."""

    def __init__(self, model, buffer, scale):
        super().__init__()
        self.model, self.buffer, self.scale, self.first, self.last = model, buffer, scale, None, None
        sample, update = buffer.sample, model.update

        @functools.wraps(sample)  # (fit_vector reads sample's signature)
        def timed_sample(*a, **kw):
            self.first = time.perf_counter() if self.first is None else self.first
            return sample(*a, **kw)

        @functools.wraps(update)
        def timed_update(*a, **kw):
            out = update(*a, **kw)  # (returns the loss as a float: the step has run)
            self.last = time.perf_counter()
            return out
        buffer.sample, model.update = timed_sample, timed_update

    def append(self, row):
        super().append(row)
        score = row["G"] * self.scale
        line = {"iteration": row["iteration"], "route": self.model._last_route,
                "update_route": self.model._last_update_route, "episodes": row["episodes"], "buffer": len(self.buffer),
                "mean_score": round(score, 1) if np.isfinite(score) else None, "loss": round(row.get("loss", float("nan")), 4),
                "collect_s": round(row["collect_s"], 3),
                "update_s": round(self.last - self.first, 3) if self.first is not None else 0.0}
        if "test_G" in row:
            line["test_score"] = round(row["test_G"] * self.scale, 1)
        self.first = self.last = None
        print(json.dumps(line), flush=True)


def fit_on_device(model, venv, args, discount, k_steps):
    buffer = muax.DeviceReplayBuffer(2000, 2000 * args.max_episode_steps, random_seed=args.seed)
    test_env = muax.Device2048(args.test_envs, max_episode_steps=args.max_episode_steps, seed=args.seed + 1,
                               reward_shift=args.reward_shift)
    muax.fit_vector(model, venv, test_env, n_step=10, gamma=discount, alpha=0.5, buffer=buffer, iterations=args.iterations,
                    steps_per_iteration=args.steps, num_simulations=args.sims, k_steps=k_steps, num_trajectory=32,
                    num_update_per_iteration=args.updates, test_interval=max(args.iterations, 1), random_seed=args.seed,
                    trajectory_weight="sum", metrics=_Report(model, buffer, 2 ** args.reward_shift), device_collect=True,
                    device_plan=True, priority_update=args.priority_steps is not None, priority_steps=args.priority_steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=64, help="lock-step env steps per iteration")
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--updates", type=int, default=20, help="updates per iteration")
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--max-episode-steps", type=int, default=200)
    ap.add_argument("--reward-shift", type=int, default=6)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--one-launch", action="store_true",
                    help="act() with the whole search in one launch (MuZero(stochastic_one_launch=True)): the same bits")
    ap.add_argument("--root-in-kernel", action="store_true",
                    help="act() with root inference by the library too (MuZero(stochastic_root_in_kernel=True)): no torch "
                         "module in an act(); with --one-launch an act() is one launch")
    ap.add_argument("--noise-in-kernel", action="store_true",
                    help="with --one-launch: the root's Dirichlet noise drawn inside that launch "
                         "(MuZero(stochastic_noise_in_kernel=True)) instead of by a launch of its own: the same bits")
    ap.add_argument("--train-on-demand", action="store_true",
                    help="with --fused-update: build an instance of the training kernel for a shape the library does not list "
                         "(MuZero(stochastic_train_on_demand=True)); a shape whose instance would spill stays on autograd")
    ap.add_argument("--fused-update", action="store_true",
                    help="update() on the fused training kernel (MuZero(stochastic_fused_update=True)) instead of autograd")
    ap.add_argument("--priority-steps", type=int, default=None, metavar="K",
                    help="write the value errors of the first K transitions of every window back as priorities "
                         "(MuZero(stochastic_unroll_values=True), fit_vector(priority_update=True, priority_steps=K)); "
                         "the device route only")
    ap.add_argument("--host-buffer", action="store_true",
                    help="this file's own loop on a host TrajectoryReplayBuffer instead of fit_vector on the device buffer")
    ap.add_argument("--test-envs", type=int, default=16, help="greedy test episodes after the first iteration (fit_vector)")
    args = ap.parse_args()

    support_size, E, Cn, discount, k_steps = 31, 32, 32, 0.997, 5
    venv = muax.Device2048(args.envs, max_episode_steps=args.max_episode_steps, seed=args.seed, reward_shift=args.reward_shift)
    net = muax.create_stochastic_muzero_network(E, venv.num_actions, Cn, 2 * support_size + 1)
    model = muax.MuZero(net, policy="stochastic", discount=discount, support_size=support_size,
                        optimizer=muax.optimizers.create_optimizer("adam", 2e-3), stochastic_one_launch=args.one_launch,
                        stochastic_fused_update=args.fused_update, stochastic_train_on_demand=args.train_on_demand, stochastic_root_in_kernel=args.root_in_kernel,
                        stochastic_unroll_values=args.priority_steps is not None,
                        stochastic_noise_in_kernel=args.noise_in_kernel)
    if args.priority_steps is not None and args.host_buffer:
        ap.error("--priority-steps needs the device route (fit_vector on a DeviceReplayBuffer), not --host-buffer")
    if not args.host_buffer:
        fit_on_device(model, venv, args, discount, k_steps)
        return
    obs = venv.reset_device()
    model.init(args.seed, np.zeros((1, obs.shape[1]), np.float32))
    buffer = muax.TrajectoryReplayBuffer(2000, random_seed=args.seed)
    key, pending = muax.prng.PRNGKey(args.seed), [None] * args.envs
    for it in range(args.iterations):
        t0 = time.perf_counter()
        episodes, obs, key = collect(model, venv, obs, key, args.steps, args.sims, pending, 10, discount)
        for tr in episodes:
            if len(tr) >= k_steps:
                buffer.add(tr, float(np.sum(tr.batched_transitions.w)))
        t1 = time.perf_counter()
        loss = float("nan")
        if len(buffer):
            for _ in range(args.updates):
                loss = model.update(buffer.sample(num_trajectory=32, k_steps=k_steps))["loss"]
        scores = [float(np.sum(tr.batched_transitions.r)) * 2 ** args.reward_shift for tr in episodes]
        print(json.dumps({"iteration": it, "route": model._last_route, "update_route": model._last_update_route, "episodes": len(episodes), "buffer": len(buffer),
                          "mean_score": round(float(np.mean(scores)), 1) if scores else None, "loss": round(loss, 4),
                          "collect_s": round(t1 - t0, 3), "update_s": round(time.perf_counter() - t1, 3)}), flush=True)


if __name__ == "__main__":
    main()
