"""Collection on the host against collection on the device, on the vector CartPole of examples/ with the default MLP
trio and 50 simulations per step:

  host    `VectorCollector.collect` (act() NumPy in / out at every step, episodes cut and n-step returns in NumPy)
          followed by `DeviceReplayBuffer.add_many` of the episodes of at least k steps, as `fit_vector` does;
  device  `DeviceVectorCollector.collect` (act() on device tensors, one staging launch per step, only the actions
          come down; the rewards go up once and the episodes are cut into the arenas in one launch).

  with --device-env, two more columns:
  dev env `DeviceVectorCollector.collect` on `muax_amd.DeviceCartPole`: the environment is stepped on the device too
          (act() on its observation tensor, the staging launch, one environment launch per step; the rewards and the
          `done` flags come down once per collect).  Its start states are its own threefry draws, so its episodes are
          not the other routes' episodes;
  act()   STEPS x act() alone on a fixed device tensor with device outputs, one synchronise at the end: the search
          launches every route pays.

  with --device-plan, one more column and one more split line:
  dev plan the same collector with `device_plan=True`: the episodes are cut and their returns summed on the device
          (`mzs_replay_plan_steps`); per collect the counts and one row per finished episode come down.

  with --env acrobot or --env mountaincar (default cartpole: everything above, unchanged) the device-environment
  columns run on `muax_amd.DeviceAcrobot` / `DeviceMountainCar` (3 actions, 6 / 2 observations) and, there being no host
  implementation of them, the host and device columns step a second instance of the same class through its HOST
  protocol (three synchronising copies per step), which is what a user without the device route would do.
  --env 2048 does the same on `muax_amd.Device2048` (4 actions, 16 observations).  Its device-environment columns search
  with the environment's legal-move mask (`invalid_actions_device()`, handed to every act() by the collector), and so
  does the act()-alone column, on the mask of a freshly reset environment; the host columns go through
  `VectorCollector`, which has no per-step mask, and search without one: the same launches, not the same episodes.

    python tools/bench_collect.py [--iters 20] [--shape ENVS,STEPS ...] [--simulations 50] [--device-env] [--device-plan]
                                  [--env cartpole|acrobot|mountaincar|2048]

Every figure is the median of `--iters` repetitions of one whole collect (+ add), each ending in a device synchronise,
after three untimed ones.  The two routes alternate shape by shape in one process; each keeps its own environment,
collector and buffer, so episodes run on from one repetition to the next as they do in training."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import muax_amd as mx  # noqa: E402
from cartpole_env import VectorCartPole  # noqa: E402
from muax_amd.utils import warm_runtime  # noqa: E402

A, E, OBS, SUPPORT, N_STEP, GAMMA, ALPHA, K = 2, 8, 4, 10, 10, 0.997, 0.5, 10
# --env: (actions, observations, host-protocol environment, device environment)
ENVS = {"cartpole": (A, OBS, lambda n: VectorCartPole(n, seed=0), lambda n: mx.DeviceCartPole(n, seed=0)),
        "acrobot": (3, 6, lambda n: mx.DeviceAcrobot(n, seed=0), lambda n: mx.DeviceAcrobot(n, seed=0)),
        "mountaincar": (3, 2, lambda n: mx.DeviceMountainCar(n, seed=0), lambda n: mx.DeviceMountainCar(n, seed=0)),
        "2048": (4, 16, lambda n: mx.Device2048(n, seed=0, reward_shift=6), lambda n: mx.Device2048(n, seed=0, reward_shift=6))}


def model(actions=A, obs_dim=OBS):
    g = torch.Generator().manual_seed(0)
    net = mx.nn.MZNetwork(mx.nn.Representation(E, generator=g), mx.nn.Prediction(actions, 2 * SUPPORT + 1, generator=g),
                          mx.nn.Dynamic(E, actions, 2 * SUPPORT + 1, generator=g))
    m = mx.MuZero(net, support_size=SUPPORT)
    m.init(0, np.zeros((1, obs_dim)))
    return m


def median_ms(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def split_ms(collector, fn, iters, plan=False):
    """Where one collect() of the device-environment route spends its time: the step loop up to and including the
    download of the call's rewards and flags (which waits for the device), `add_steps` (upload, store launch, then a
    synchronise added here) and the rest (ring_plan, the returns and the bookkeeping, on the host).  Medians, ms.
    `plan` (a collector with device_plan): the step loop downloads nothing and does not wait; the plan launches and the
    downloads of the counts and the episode rows (which wait for the device) are timed as a fourth part, and the rest
    is the two list comprehensions that build the episode list.  Returns (total, loop, add_steps[, plan])."""
    spent = {"loop": [], "add_steps": [], "plan": []}

    def timed(obj, name, key, sync):
        inner = getattr(obj, name)

        def outer(*args, **kw):
            t0 = time.perf_counter()
            out = inner(*args, **kw)
            if sync:
                torch.cuda.synchronize()
            spent[key][-1] += (time.perf_counter() - t0) * 1e3
            return out
        setattr(obj, name, outer)
        return lambda: setattr(obj, name, inner)

    undo = [timed(collector, "_steps", "loop", False), timed(collector.buffer, "add_steps", "add_steps", True)]
    if plan:  # from the plan call to the end of the collector's downloads: counts, then (if any episode ended) ep, ret
        L, cpu = collector.buffer._L, torch.Tensor.cpu
        inner_plan, mark = L.mzs_replay_plan_steps, {}

        def plan_call(*args):
            mark["t0"], mark["left"] = time.perf_counter(), 1  # (the counts come first and say whether more follows)
            return inner_plan(*args)

        def plan_cpu(t, *args, **kw):
            out = cpu(t, *args, **kw)
            if mark.get("left"):
                if t is collector._plan["counts"]:
                    mark["left"] = 3 if int(out[0]) else 1
                mark["left"] -= 1
                spent["plan"][-1] = (time.perf_counter() - mark["t0"]) * 1e3  # a later .cpu() of the call is not counted
            return out

        def restore():
            L.mzs_replay_plan_steps = inner_plan
            del torch.Tensor.cpu  # (the wrapper sat in Tensor's own dict, in front of the base class's method)
        L.mzs_replay_plan_steps, torch.Tensor.cpu = plan_call, plan_cpu
        undo.append(restore)
    total = []
    for _ in range(iters):
        for v in spent.values():
            v.append(0.0)
        t0 = time.perf_counter()
        if plan:
            mark.clear()
        fn()
        torch.cuda.synchronize()
        total.append((time.perf_counter() - t0) * 1e3)
    for u in undo:
        u()
    loop, add = float(np.median(spent["loop"])), float(np.median(spent["add_steps"]))
    if plan:
        return float(np.median(total)), loop, add, float(np.median(spent["plan"]))
    return float(np.median(total)), loop, add


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--simulations", type=int, default=50)
    ap.add_argument("--shape", action="append", default=[], metavar="ENVS,STEPS")
    ap.add_argument("--device-env", action="store_true", help="also time collection on DeviceCartPole and act() alone")
    ap.add_argument("--device-plan", action="store_true",
                    help="also time collection on DeviceCartPole with the episodes cut on the device (device_plan=True)")
    ap.add_argument("--env", default="cartpole", choices=list(ENVS),
                    help="the environment; acrobot and mountaincar run the host columns on the device class's host protocol")
    a = ap.parse_args()
    actions, obs_dim, host_env, device_env = ENVS[a.env]
    shapes = [tuple(int(x) for x in s.split(",")) for s in a.shape] or [(64, 64), (1024, 64)]
    warm_runtime()
    print(f"vector {'CartPole' if a.env == 'cartpole' else a.env}, {a.simulations} simulations, n_step {N_STEP}, episodes of at least {K} steps stored; "
          f"median of {a.iters} synchronised repetitions, ms")
    print(f"{'envs x steps':>12} | {'host collect':>12} {'host collect+add_many':>21} | {'device collect (incl. add)':>26} | "
          f"{'host / device':>13}" + (f" | {'dev env collect (incl. add)':>27} {'steps x act()':>13}" if a.device_env else "")
          + (f" | {'dev plan collect (incl. add)':>28}" if a.device_plan else ""))
    for envs, steps in shapes:
        m = model(actions, obs_dim)
        state = {"hk": mx.prng.PRNGKey(0), "dk": mx.prng.PRNGKey(0)}
        cap, rows = 8 * envs, 8 * envs * steps + 4096
        host_buf, dev_buf = mx.DeviceReplayBuffer(cap, rows), mx.DeviceReplayBuffer(cap, rows)
        host = mx.VectorCollector(host_env(envs), N_STEP, GAMMA, ALPHA)
        host_only = mx.VectorCollector(host_env(envs), N_STEP, GAMMA, ALPHA)
        dev = mx.DeviceVectorCollector(host_env(envs), dev_buf, N_STEP, GAMMA, ALPHA, min_length=K)

        def host_collect():
            _, state["hk"], _ = host_only.collect(m, state["hk"], steps, a.simulations)

        def host_route():
            trajs, state["hk"], _ = host.collect(m, state["hk"], steps, a.simulations)
            keep = [t for t in trajs if len(t) >= K]
            host_buf.add_many(keep, [t.weights.mean() for t in keep])

        def device_route():
            _, state["dk"], _ = dev.collect(m, state["dk"], steps, a.simulations)

        hc = median_ms(host_collect, a.iters)
        hr = median_ms(host_route, a.iters)
        dr = median_ms(device_route, a.iters)
        line = f"{envs:>7} x {steps:<2} | {hc:12.3f} {hr:21.3f} | {dr:26.3f} | {hr / dr:12.2f}x"
        if a.device_env:
            env_buf = mx.DeviceReplayBuffer(cap, rows)
            env_dev = mx.DeviceVectorCollector(device_env(envs), env_buf, N_STEP, GAMMA, ALPHA, min_length=K)
            state["ek"] = state["ak"] = mx.prng.PRNGKey(0)
            fixed_env = host_env(envs)
            fixed = torch.from_numpy(fixed_env.reset()).to(m.device)
            mask = ({"invalid_actions": fixed_env.invalid_actions_device()}
                    if hasattr(fixed_env, "invalid_actions_device") else {})

            def env_route():
                _, state["ek"], _ = env_dev.collect(m, state["ek"], steps, a.simulations)

            def act_alone():
                for _ in range(steps):
                    state["ak"], sub = mx.prng.split(state["ak"])
                    m.act(sub, fixed, with_pi=True, with_value=True, obs_from_batch=True, device_outputs=True,
                          num_simulations=a.simulations, **mask)

            line += f" | {median_ms(env_route, a.iters):27.3f} {median_ms(act_alone, a.iters):13.3f}"
        if a.device_plan:
            plan_buf = mx.DeviceReplayBuffer(cap, rows)
            plan_dev = mx.DeviceVectorCollector(device_env(envs), plan_buf, N_STEP, GAMMA, ALPHA,
                                                min_length=K, device_plan=True)
            state["pk"] = mx.prng.PRNGKey(0)

            def plan_route():
                _, state["pk"], _ = plan_dev.collect(m, state["pk"], steps, a.simulations)

            line += f" | {median_ms(plan_route, a.iters):28.3f}"
        print(line, flush=True)
        if a.device_env:
            total, loop, add = split_ms(env_dev, env_route, a.iters)
            print(f"{'':>12}   dev env collect, split: {total:.3f} = step loop and download {loop:.3f} + add_steps "
                  f"{add:.3f} + host tail {total - loop - add:.3f}", flush=True)
        if a.device_plan:
            total, loop, add, plan = split_ms(plan_dev, plan_route, a.iters, plan=True)
            print(f"{'':>12}   dev plan collect, split: {total:.3f} = step loop {loop:.3f} + plan and download {plan:.3f} "
                  f"+ add_steps {add:.3f} + host tail {total - loop - plan - add:.3f}", flush=True)


if __name__ == "__main__":
    main()
