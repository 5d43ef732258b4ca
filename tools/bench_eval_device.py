"""Greedy evaluation through the host protocol against evaluation on the device: `test_vector` (act() NumPy in / out and
three synchronising copies per environment step) against `test_vector_device` (nothing leaves the device inside the
loop but one "all finished" check every 16 steps) on the same device environment, same model, same key -- the two
values are asserted equal.

    python tools/bench_eval_device.py [--env acrobot] [--envs 64] [--max-episode-steps 200] [--simulations 50] [--iters 5]

Every figure is the median of `--iters` whole evaluations, each ending in a device synchronise, after one untimed one."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import muax_amd as mx  # noqa: E402
from muax_amd.utils import warm_runtime  # noqa: E402

ENVS = {"cartpole": (mx.DeviceCartPole, 2, 4), "acrobot": (mx.DeviceAcrobot, 3, 6), "mountaincar": (mx.DeviceMountainCar, 3, 2)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--env", default="acrobot", choices=list(ENVS))
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--max-episode-steps", type=int, default=200)
    ap.add_argument("--simulations", type=int, default=50)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    cls, actions, obs_dim = ENVS[a.env]
    g = torch.Generator().manual_seed(0)
    net = mx.nn.MZNetwork(mx.nn.Representation(8, generator=g), mx.nn.Prediction(actions, 21, generator=g),
                          mx.nn.Dynamic(8, actions, 21, generator=g))
    model = mx.MuZero(net, support_size=10)
    model.init(0, np.zeros((1, obs_dim)))
    warm_runtime()
    key, out = mx.prng.PRNGKey(0), {}
    for name, fn in (("test_vector", mx.test_vector), ("test_vector_device", mx.test_vector_device)) * 2:  # alternating
        times = []
        for i in range(a.iters + 1):
            env = cls(a.envs, max_episode_steps=a.max_episode_steps, seed=1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            value = fn(model, env, key, a.simulations)
            torch.cuda.synchronize()
            if i:
                times.append((time.perf_counter() - t0) * 1e3)
        out.setdefault(name, []).append((float(np.median(times)), value))
    (h1, v1), (h2, v2) = out["test_vector"]
    (d1, w1), (d2, w2) = out["test_vector_device"]
    assert v1 == v2 == w1 == w2, (v1, v2, w1, w2)
    print(f"{a.env}, {a.envs} environments, max_episode_steps {a.max_episode_steps}, {a.simulations} simulations; median "
          f"of {a.iters} evaluations, ms, two alternating passes; value {v1}")
    print(f"  test_vector (host protocol)   {h1:9.2f} {h2:9.2f}")
    print(f"  test_vector_device            {d1:9.2f} {d2:9.2f}   host / device {h1 / d1:.2f}x {h2 / d2:.2f}x")


if __name__ == "__main__":
    main()
