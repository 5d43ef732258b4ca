"""2048 with Stochastic MuZero: `muax.Device2048` stepped on the device, every act() the stochastic search over chance
nodes (4 actions + 32 chance codes) on the default stochastic MLP family -- the decision and the chance function
evaluated by the library, one launch per simulation --, training with `loss.stochastic_loss_fn` from a host
`TrajectoryReplayBuffer` (on torch autograd, or with --fused-update on the fused training kernel of this shape).

The loss encodes a chance code from EVERY step's observation, which `DeviceReplayBuffer.sample` does not hand out (it
keeps the first row of a window), and `fit_vector(device_collect=True)` stores into that buffer only.  So this example
has its own short loop: the step loop runs on the device with no per-step host copy (observation, mask, action, search
policy, value, reward and flag stay device tensors), the iteration's stream comes down once, is cut into finished
episodes (`episode_trajectory`) and goes into the host buffer.

Nothing here has been run to a result: whether this recipe learns 2048 is not known.

    python examples/fit_2048_stochastic.py [--envs 256] [--steps 64] [--iterations 3] [--updates 20] [--one-launch]
                                           [--fused-update]
"""
import argparse
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
    ap.add_argument("--fused-update", action="store_true",
                    help="update() on the fused training kernel (MuZero(stochastic_fused_update=True)) instead of autograd")
    args = ap.parse_args()

    support_size, E, Cn, discount, k_steps = 31, 32, 32, 0.997, 5
    venv = muax.Device2048(args.envs, max_episode_steps=args.max_episode_steps, seed=args.seed, reward_shift=args.reward_shift)
    net = muax.create_stochastic_muzero_network(E, venv.num_actions, Cn, 2 * support_size + 1)
    model = muax.MuZero(net, policy="stochastic", discount=discount, support_size=support_size,
                        optimizer=muax.optimizers.create_optimizer("adam", 2e-3), stochastic_one_launch=args.one_launch,
                        stochastic_fused_update=args.fused_update)
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
                          "collect_s": round(t1 - t0, 2), "update_s": round(time.perf_counter() - t1, 2)}), flush=True)


if __name__ == "__main__":
    main()
