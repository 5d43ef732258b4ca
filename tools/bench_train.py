"""Training step (BASELINE config 5 shape: 4096 trajectories, k_steps=10, default MLP trio): the fused HIP
forward+backward (mzs_mlp_loss_grad) vs the torch autograd route, loss+gradients only and whole update().

    python tools/bench_train.py [B] [L] [--wide] [--shape A,E,OBS ...] [--runs N]

--wide adds the shapes of the wide training instances (17 to 64 actions, observations up to 128 wide; built on demand
by muax_amd/_jit.py::ensure_wide_train_instance) after config 5's, and the pair (16, 8, 4) / (17, 8, 4): almost the
same work on a narrow and on a wide instance, which re-reads its weights from LDS in every unroll step.  --shape adds
any other.  --runs N takes every timing (update() under both backends, the loss+grad device time) N times and prints the
median with min and max (default 1)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import muax_amd as mx  # noqa: E402
from muax_amd.utils import warm_runtime  # noqa: E402

warm_runtime()  # (the runtime's signal pool grown before anything is timed: tools/diag_stall.py)


def timeit(fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


# (num_actions, embedding_dim, obs_dim): config 5's shape, then the wide ones
NARROW = (2, 8, 4)
WIDE_SHAPES = [(18, 8, 128), (18, 32, 8), (64, 64, 16), (16, 8, 4), (17, 8, 4)]


def device_us(f, batch, runs, calls=50):
    """Device time per loss+grad call (event-timed over `calls` back-to-back calls), `runs` times."""
    out = []
    for _ in range(runs):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(calls):
            f(batch)
        ev1.record()
        torch.cuda.synchronize()
        out.append(ev0.elapsed_time(ev1) / calls * 1e3)
    return out


def spread(v, scale, unit):
    v = [x * scale for x in v]
    return f"{float(np.median(v)):9.3f} {unit}" + (f" (median of {len(v)}, {min(v):.3f} .. {max(v):.3f})" if len(v) > 1 else "")


def bench_shape(A, E, obs_dim, B, L, runs):
    g = torch.Generator().manual_seed(0)
    rng = np.random.default_rng(0)
    batch = mx.Transition(obs=torch.rand(B, L, obs_dim).cuda(), a=torch.randint(0, A, (B, L)).cuda(),
                          r=torch.rand(B, L).cuda(), Rn=(torch.rand(B, L) * 20).cuda(),
                          pi=torch.as_tensor(rng.dirichlet([1] * A, (B, L)).astype(np.float32)).cuda())
    res = {}
    print(f"-- A={A} E={E} obs_dim={obs_dim} support=10 B={B} L={L}")
    for backend in ("hip", "torch"):
        net = mx.nn.MZNetwork(mx.nn.Representation(E, generator=g), mx.nn.Prediction(A, 21, generator=g),
                              mx.nn.Dynamic(E, A, 21, generator=g))
        m = mx.MuZero(net)
        m.init(0, np.zeros((1, obs_dim)))
        t = [timeit(lambda: m.update(batch, backend=backend)) for _ in range(runs)]
        res[backend] = float(np.median(t))
        print(f"update() backend={backend:5s}: {spread(t, 1e3, 'ms/step')} {B * L / res[backend] / 1e6:8.2f} M transitions/s")
        if backend == "hip":
            f = m._fused_train
            th = timeit(lambda: f(batch), n=50)
            print(f"  loss+grad kernels only: host-timed {th * 1e6:8.1f} us/call, device {spread(device_us(f, batch, runs), 1.0, 'us/call')}")
    print(f"  update() torch / hip: {res['torch'] / res['hip']:.1f}x")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("B", nargs="?", type=int, default=4096)
    ap.add_argument("L", nargs="?", type=int, default=10)
    ap.add_argument("--wide", action="store_true")
    ap.add_argument("--shape", action="append", default=[], metavar="A,E,OBS")
    ap.add_argument("--runs", type=int, default=1)
    a = ap.parse_args()
    shapes = [NARROW] + (WIDE_SHAPES if a.wide else []) + [tuple(int(x) for x in s.split(",")) for s in a.shape]
    for A, E, obs_dim in shapes:
        bench_shape(A, E, obs_dim, a.B, a.L, a.runs)


if __name__ == "__main__":
    main()
