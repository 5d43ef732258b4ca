"""Acrobot with the whole acting half AND the greedy test on the device: `fit_cartpole_device.py` on
`muax.DeviceAcrobot` (Gym's Acrobot-v1 dynamics, one Runge-Kutta launch per step; 6 observations, 3 actions, reward -1
per step and 0 on the step that swings the tip above the bar), a `DeviceReplayBuffer` and `device_collect=True`.  The
test environment is a second DeviceAcrobot: `fit_vector` evaluates it with `test_vector_device`, so the greedy episodes
run without a host hop per step as well (one "all finished" check every 16 steps, one download of the returns at the
end).  An untrained agent scores -500 (the episode limit); anything above it has learnt to swing up.  With
--device-plan the episodes are also cut and their returns summed on the device.

    python examples/fit_acrobot_device.py [--envs 1024] [--steps 128] [--iterations 100] [--updates 300] [--device-plan]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import muax_amd as muax  # noqa: E402
from muax_amd import nn  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=128, help="lock-step env steps per iteration")
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--updates", type=int, default=300, help="updates per iteration")
    ap.add_argument("--buffer", type=int, default=4000, help="trajectories kept")
    ap.add_argument("--rows", type=int, default=1 << 21, help="transitions kept (the arenas' rows)")
    ap.add_argument("--test-envs", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--traj-weight", default="sum", choices=["mean", "sum"])
    ap.add_argument("--device-plan", action="store_true", help="cut the episodes and sum their returns on the device")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    support_size, embedding_size, discount = 10, 8, 0.99
    venv = muax.DeviceAcrobot(args.envs, seed=args.seed)
    test_env = muax.DeviceAcrobot(args.test_envs, seed=10_000 + args.seed)
    net = muax.create_muzero_network(nn.Representation, nn.Prediction, nn.Dynamic, embedding_dim=embedding_size,
                                     num_actions=venv.num_actions, full_support_size=2 * support_size + 1)
    total = args.iterations * args.updates
    opt = muax.model.optimizer(init_value=0.02, peak_value=0.02, end_value=0.002, warmup_steps=total // 6,
                               transition_steps=total // 6)
    model = muax.MuZero(net, discount=discount, optimizer=opt, support_size=support_size)
    marks = [time.perf_counter()]

    class Timed(list):  # wall-clock mark per iteration
        def append(self, row):
            marks.append(time.perf_counter())
            row["wall_s"] = round(marks[-1] - marks[0], 2)
            super().append(row)

    metrics = Timed()
    muax.fit_vector(model, venv, test_env, n_step=10, gamma=discount, alpha=0.5,
                    buffer=muax.DeviceReplayBuffer(args.buffer, args.rows), device_collect=True,
                    device_plan=args.device_plan, num_simulations=50, iterations=args.iterations,
                    steps_per_iteration=args.steps, k_steps=10, num_trajectory=32, sample_per_trajectory=1,
                    num_update_per_iteration=args.updates, max_training_steps=total, test_interval=5,
                    random_seed=args.seed, metrics=metrics, trajectory_weight=args.traj_weight)
    wall = time.perf_counter() - marks[0]
    for r in metrics:
        print(f"iteration {r['iteration']:3d}  t {r['wall_s']:6.1f}s  episodes {r['episodes']:5d}  mean G {r['G']:7.1f}  "
              f"loss {r.get('loss', float('nan')):.4f}  updates {r['training_step']:6d}"
              + (f"  test_G {r['test_G']:.1f}" if "test_G" in r else ""), flush=True)
    env_steps = int(sum(r["env_steps"] for r in metrics))
    summary = {"recipe": f"fit_vector(device_collect{', device_plan' if args.device_plan else ''}), {args.envs} Acrobots on "
                         f"the device, greedy test on the device, {args.steps} steps/iteration, S=50, k_steps=10, "
                         f"buffer {args.buffer}, trajectory weight {args.traj_weight}",
               "iterations": len(metrics), "updates": metrics[-1]["training_step"], "env_steps": env_steps,
               "wall_s": round(wall, 1), "env_steps_per_s_whole_loop": round(env_steps / wall),
               "env_steps_per_s_acting_half": round(env_steps / sum(r["collect_s"] for r in metrics)),
               "test_G_curve": [[r["iteration"], r["test_G"]] for r in metrics if "test_G" in r]}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
