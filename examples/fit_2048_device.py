"""2048 with the whole acting half, the legal-move masks AND the greedy test on the device: `fit_acrobot_device.py` on
`muax.Device2048` (one integer launch per step; 16 observations = exponent / 16, 4 actions, reward = the tiles a move
merges, spawns from a threefry stream), a `DeviceReplayBuffer` and `device_collect=True`.  The environment's own mask
tensor goes into every act() of the collection and of the greedy test, and every reanalysis (`--reanalyse-every`)
searches the stored observations under `venv.invalid_actions_of`, so no search policy in the buffer puts weight on a
move that would leave the board unchanged.  The search of THIS example is the deterministic MuZero one: the spawn is
chance the model has to average over.  (`StochasticMuZeroPolicy` -- the search over chance nodes, at 2048's 4 actions +
32 chance codes among others -- is built, but it takes decision and chance functions, which the default network trio
trained here does not have.)

Scale.  The value head is a categorical over -support_size .. support_size of h(x) = sign(x)(sqrt(|x| + 1) - 1) + 0.001 x,
so support_size 31 (the widest the fused kernels take) holds |x| up to 962.  Rewards are the merged tiles times
2^-reward_shift; with the default --reward-shift 6 a 2048 merge is worth 32 and the support covers returns up to
962 * 64 = 61 568 points of the game's own score.  What would clip: the return of a game that scores more than that from
some state on (roughly, one that goes on well past the 4096 tile), and with it the n-step targets there, which are ten
rewards plus 0.997^10 of a value that is itself at most 962.  A random player scores about a thousand points (16 after
the shift), so early training is far from the edge; --reward-shift 8 (support up to 246 272 points) is the setting for
an agent that gets further, at the price of small merges becoming hard to tell apart (a 4 is worth 1 / 64).

Nothing here has been run to a result: whether this recipe learns 2048 is not known.

    python examples/fit_2048_device.py [--envs 1024] [--steps 128] [--iterations 100] [--updates 300] [--device-plan]
                                       [--reward-shift 6] [--reanalyse-every 0]
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
    ap.add_argument("--max-episode-steps", type=int, default=2000)
    ap.add_argument("--reward-shift", type=int, default=6, help="rewards are the merged tiles times 2^-shift (0..11)")
    ap.add_argument("--reanalyse-every", type=int, default=0, help="reanalyse the buffer every this many iterations")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--traj-weight", default="sum", choices=["mean", "sum"])
    ap.add_argument("--device-plan", action="store_true", help="cut the episodes and sum their returns on the device")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    support_size, embedding_size, discount = 31, 32, 0.997
    venv = muax.Device2048(args.envs, max_episode_steps=args.max_episode_steps, seed=args.seed,
                           reward_shift=args.reward_shift)
    test_env = muax.Device2048(args.test_envs, max_episode_steps=args.max_episode_steps, seed=10_000 + args.seed,
                               reward_shift=args.reward_shift)
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
                    random_seed=args.seed, metrics=metrics, trajectory_weight=args.traj_weight,
                    reanalyse_every=args.reanalyse_every)
    wall = time.perf_counter() - marks[0]
    points = float(2 ** args.reward_shift)  # G and test_G are in shifted rewards; printed in the game's own points
    for r in metrics:
        print(f"iteration {r['iteration']:3d}  t {r['wall_s']:6.1f}s  episodes {r['episodes']:5d}  "
              f"mean score {r['G'] * points:8.1f}  loss {r.get('loss', float('nan')):.4f}  updates {r['training_step']:6d}"
              + (f"  test score {r['test_G'] * points:.1f}" if "test_G" in r else ""), flush=True)
    env_steps = int(sum(r["env_steps"] for r in metrics))
    summary = {"recipe": f"fit_vector(device_collect{', device_plan' if args.device_plan else ''}), {args.envs} games of 2048 "
                         f"on the device with legal-move masks, greedy test on the device, {args.steps} steps/iteration, "
                         f"S=50, k_steps=10, reward_shift {args.reward_shift}, support_size {support_size}, buffer "
                         f"{args.buffer}, trajectory weight {args.traj_weight}, reanalyse_every {args.reanalyse_every}",
               "iterations": len(metrics), "updates": metrics[-1]["training_step"], "env_steps": env_steps,
               "wall_s": round(wall, 1), "env_steps_per_s_whole_loop": round(env_steps / wall),
               "env_steps_per_s_acting_half": round(env_steps / sum(r["collect_s"] for r in metrics)),
               "test_score_curve": [[r["iteration"], r["test_G"] * points] for r in metrics if "test_G" in r]}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
