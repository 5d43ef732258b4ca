"""What the chance rule and the merged expansion cost per simulation: one act of the stochastic step-wise search
(4 actions + 32 chance outcomes, Stochastic MuZero's 2048 shape) beside the deterministic walking search (MZS_STEP_WALK=1)
at 36 actions -- the same slots per node, simulations and roots, scripted net outputs (fixed tensors: no net time), two
tree launches per simulation on either side.  Runs alternate between the two; medians and ranges over `--repeats`.

    python tools/bench_stochastic.py [--sims 50] [--repeats 15] [--out FILE]

--mlp: the default stochastic MLP family (E = 16) searched three ways from the same root outputs -- the callable route
(search_stochastic with the torch modules: both functions on every root, a few dozen small torch launches per simulation),
the step-wise library route (search_stochastic_mlp: one launch for the functions, three launches per simulation) and the
one-launch route (search_stochastic_mlp(one_launch=True): the whole search in one launch, tree in LDS) -- at 64, 1024 and
4096 roots, eager and graph=True, alternating.

--train: the training step of the default family at (A, C, E, F) = (4, 32, 16, 21) and (4, 32, 32, 63), obs_dim 16,
L = 5, B = 32 and 1024: loss plus gradients (loss.StochasticFusedLossGrad against stochastic_loss_fn + backward) and the
whole update() (MuZero(stochastic_fused_update=True) under backend="hip" against backend="torch", Adam), the two routes
alternating in one process after warm_runtime().  Host wall time around a synchronised call, in microseconds: the
torch route is launch-bound, so its figure is mostly host time and moves with the load of the machine; median, min
and max over `--repeats` (at least 15).

--act: the whole MuZero.act() of the default family on device observations at 2048's shape (4 actions + 32 outcomes,
E = 16, support 10, obs_dim 16, `--sims` simulations, root noise drawn from the key, device outputs) at 64, 1024 and
4096 roots, on the one-launch route with the root inference on the torch modules (stochastic_root_in_kernel=False),
inside the launch (True), and with the root noise drawn inside the launch as well (stochastic_noise_in_kernel=True): three
models of the same weights alternating in one process after warm_runtime() and five warm-up acts each; --graph: all three
with capture_graph=True.  A sample is the host wall time around ten consecutive acts and one synchronisation, per act, in
microseconds (the torch root is launch-bound: its cost is host time); median, min and max over `--repeats` (at least 15).
`dirichlet_launch` is the separate draw the third setting removes (model._dirichlet: mzs_dirichlet's launch and its
output allocation), timed the same way.

--unroll: the value priorities of the default family at (A, C, E, support) = (4, 32, 16, 10), obs_dim 16, for 32 and 4096
windows of 10 steps: MuZero(stochastic_unroll_values=True).unroll_values on the kernel route (backend="hip", one launch)
and on the torch modules (backend="torch"), and beside them vector.value_priorities, the ONE priority per window that
fit_vector writes back with priority_steps=None -- the three alternating in one process after warm_runtime() and ten
warm-up calls each.  A sample is the host wall time around ten consecutive calls and one synchronisation, per call, in
microseconds; median, min and max over `--repeats` (at least 15).
"""
import argparse
import json
import os
import statistics
import sys

os.environ["MZS_STEP_WALK"] = "1"  # (read when a handle first allocates its tree)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from muax_amd import MuZeroSearch, SearchConfig  # noqa: E402

A, C, E = 4, 32, 32


def make(batch, sims):
    g = torch.Generator().manual_seed(batch)
    r = lambda *s: torch.randn(*s, generator=g).cuda()  # noqa: E731
    st = MuZeroSearch(batch, SearchConfig(A, sims, E, policy="stochastic", num_chance_outcomes=C))
    de = MuZeroSearch(batch, SearchConfig(A + C, sims, E, policy="muzero"))
    disc = torch.full((batch,), 0.99).cuda()
    s_root, d_root = (r(batch, A), r(batch), r(batch, E)), (r(batch, A + C), r(batch), r(batch, E))
    s_out = ((r(batch, C), r(batch)), r(batch, E), (r(batch, A), r(batch), r(batch), disc), r(batch, E))
    d_out = (r(batch), disc, r(batch, A + C), r(batch), r(batch, E))

    def stochastic():
        st.root_stochastic(*s_root, key=1)
        for sim in range(sims):
            st.select_stochastic(sim)
            st.expand_backup_stochastic(sim, *s_out)
        st.finish_stochastic()

    def deterministic():
        de.root(*d_root, key=1)
        for sim in range(sims):
            de.select(sim)
            de.expand_backup(sim, *d_out)
        de.finish()

    return stochastic, deterministic, (st, de)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # us


def make_mlp(batch, sims, graph):
    """(callable route, library route, one-launch route, handles) for one act of the default family at 2048's shape."""
    import numpy as np

    import muax_amd as mx
    e = 16
    net = mx.create_stochastic_muzero_network(e, A, C, 21, generator=torch.Generator().manual_seed(1))
    m = mx.MuZero(net, policy="stochastic")
    m.init(0, np.zeros((1, 16), np.float32))
    g = torch.Generator().manual_seed(batch)
    root = m._root_inference_eager(torch.rand(batch, 16, generator=g).cuda())
    cfg = SearchConfig(A, sims, e, policy="stochastic", num_chance_outcomes=C)
    hc, hl, ho = MuZeroSearch(batch, cfg), MuZeroSearch(batch, cfg), MuZeroSearch(batch, cfg)
    for h in (hl, ho):
        h.set_stochastic_mlp_weights({k: v.detach() for k, v in mx.nn.stochastic_mlp_weights(net).items()}, 10, 0.99)
    dec = lambda a, s: m._decision_inference(None, None, a, s)  # noqa: E731
    cha = lambda c, s: m._chance_inference(None, None, c, s)  # noqa: E731
    return (lambda: hc.search_stochastic(root, dec, cha, key=1, dirichlet_fraction=0.0, graph=graph),
            lambda: hl.search_stochastic_mlp(root, key=1, dirichlet_fraction=0.0, graph=graph),
            lambda: ho.search_stochastic_mlp(root, key=1, dirichlet_fraction=0.0, graph=graph, one_launch=True), (hc, hl, ho))


def main_mlp(args):
    rows = []
    for batch in (64, 1024, 4096):
        for graph in (False, True):
            call, lib, one, handles = make_mlp(batch, args.sims, graph)
            for _ in range(3):
                call(), lib(), one()
            torch.cuda.synchronize()
            same = torch.equal(handles[1].action_weights, handles[2].action_weights) and torch.equal(handles[1].action, handles[2].action)
            t = {"callables": [], "library": [], "one_launch": []}
            for _ in range(args.repeats):  # alternating
                t["callables"].append(timed(call))
                t["library"].append(timed(lib))
                t["one_launch"].append(timed(one))
            row = {"roots": batch, "sims": args.sims, "graph": graph}
            for k, v in t.items():
                row[k] = {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1),
                          "per_sim_us": round(statistics.median(v) / args.sims, 2)}
            row["speedup_median"] = round(row["callables"]["median_us"] / row["library"]["median_us"], 2)
            row["one_launch_speedup_median"] = round(row["library"]["median_us"] / row["one_launch"]["median_us"], 2)
            row["one_launch_same_bits"] = same
            rows.append(row)
            print(json.dumps(row), flush=True)
            for h in handles:
                h.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


def wall(fn):
    import time
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6  # us


def main_train(args):
    import time

    import numpy as np

    import muax_amd as mx
    from muax_amd.utils import warm_runtime
    warm_runtime()
    repeats = max(15, args.repeats)
    rows = []
    L = 5
    # (A, C, E, support, obs_dim): 2048's two listed shapes, or --shape (an unlisted one gets an instance built on demand)
    shapes = [tuple(args.shape)] if args.shape else [(4, 32, 16, 10, 16), (4, 32, 32, 31, 16)]
    for A, C, e, support, od in shapes:  # (A, C: the module's 2048 constants, shadowed by the row's)
        for batch in (32, 1024):
            rng = np.random.default_rng(batch)
            b = mx.Transition(obs=torch.from_numpy(rng.uniform(0, 1, (batch, L, od)).astype(np.float32)).cuda(),
                              a=torch.from_numpy(rng.integers(0, A, (batch, L)).astype(np.int32)).cuda(),
                              r=torch.from_numpy(rng.uniform(-1, 2, (batch, L)).astype(np.float32)).cuda(),
                              Rn=torch.from_numpy(rng.uniform(-5, 9, (batch, L)).astype(np.float32)).cuda(),
                              pi=torch.from_numpy(rng.dirichlet(np.ones(A), (batch, L)).astype(np.float32)).cuda())
            models = {}
            for route in ("fused", "torch"):
                net = mx.create_stochastic_muzero_network(e, A, C, 2 * support + 1, generator=torch.Generator().manual_seed(1))
                m = models[route] = mx.MuZero(net, policy="stochastic", support_size=support, stochastic_fused_update=True,
                                              stochastic_train_on_demand=bool(args.shape),
                                              optimizer=mx.optimizers.create_optimizer("adam", 1e-3))
                m.init(0, np.zeros((1, od), np.float32))
            fused = mx.loss.StochasticFusedLossGrad(models["fused"])
            if args.shape:
                from muax_amd import _jit
                t0 = time.perf_counter()
                built = _jit.ensure_stochastic_train_instance(A, C, e, 2 * support + 1, od)
                print(json.dumps({"ensure_s": round(time.perf_counter() - t0, 2), "registered": built,
                                  "info": _jit.stochastic_train_instance_info(A, C, e, 2 * support + 1, od)}), flush=True)

            def grad_torch(m=models["torch"]):
                for mod in m.network:
                    mod.zero_grad(set_to_none=True)
                mx.loss.stochastic_loss_fn(m, b).backward()
            calls = {"loss_grad": {"fused": lambda: fused(b), "torch": grad_torch},
                     "update": {"fused": lambda: models["fused"].update(b, backend="hip"),
                                "torch": lambda: models["torch"].update(b, backend="torch")}}
            row = {"A": A, "C": C, "E": e, "F": 2 * support + 1, "obs_dim": od, "L": L, "B": batch, "repeats": repeats}
            for what, pair in calls.items():
                for _ in range(5):  # warm-up: workspace, optimiser state, torch's autograd caches
                    pair["fused"](), pair["torch"]()
                t = {"fused": [], "torch": []}
                for _ in range(repeats):  # alternating
                    for k in ("fused", "torch"):
                        t[k].append(wall(pair[k]))
                row[what] = {k: {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1),
                                 "max_us": round(max(v), 1)} for k, v in t.items()}
                row[what]["torch_over_fused_median"] = round(row[what]["torch"]["median_us"] / row[what]["fused"]["median_us"], 2)
            assert models["fused"]._last_update_route == "hip_stochastic_fused" and models["torch"]._last_update_route == "torch"
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


def main_act(args):
    import numpy as np

    import muax_amd as mx
    from muax_amd.utils import warm_runtime
    warm_runtime()
    repeats, inner, od, e = max(15, args.repeats), 10, 16, 16
    # setting -> (the model's flags, the route its acts must take)
    settings = {"torch_root": ({}, "hip_stochastic_one_launch"),
                "root_in_kernel": (dict(stochastic_root_in_kernel=True), "hip_stochastic_one_launch_root"),
                "noise_in_kernel": (dict(stochastic_root_in_kernel=True, stochastic_noise_in_kernel=True),
                                    "hip_stochastic_one_launch_root_noise")}
    rows = []
    for batch in (64, 1024, 4096):
        obs = torch.rand(batch, od, generator=torch.Generator().manual_seed(batch)).cuda()
        models = {}
        for name, (flags, _) in settings.items():
            net = mx.create_stochastic_muzero_network(e, A, C, 21, generator=torch.Generator().manual_seed(1))
            m = models[name] = mx.MuZero(net, policy="stochastic", stochastic_one_launch=True, capture_graph=args.graph, **flags)
            m.init(0, np.zeros((1, od), np.float32))

        def acts(m, n):
            for i in range(n):
                m.act([7, i], obs, with_pi=True, with_value=True, obs_from_batch=True, num_simulations=args.sims,
                      device_outputs=True)

        def draws(n):
            for i in range(n):
                mx.model._dirichlet((7, i), 0.3, (batch, A), "cuda")
        for name, m in models.items():
            acts(m, 5)
            assert m._last_route == settings[name][1], m._last_route
        draws(5)
        t = {name: [] for name in list(settings) + ["dirichlet_launch"]}
        for _ in range(repeats):  # alternating
            for name, m in models.items():
                t[name].append(wall(lambda: acts(m, inner)) / inner)
            t["dirichlet_launch"].append(wall(lambda: draws(inner)) / inner)
        a = {name: [x.clone() for x in m.act([7, 0], obs, with_pi=True, obs_from_batch=True, num_simulations=args.sims,
                                             device_outputs=True)] for name, m in models.items()}
        row = {"roots": batch, "sims": args.sims, "graph": bool(args.graph), "repeats": repeats, "acts_per_sample": inner,
               "same_actions": round(float((a["torch_root"][0] == a["root_in_kernel"][0]).float().mean()), 4),
               "noise_in_kernel_same_bits": all(torch.equal(x.view(torch.int32), y.view(torch.int32))
                                                for x, y in zip(a["root_in_kernel"], a["noise_in_kernel"]))}
        for name, v in t.items():
            row[name] = {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}
        row["torch_root_over_in_kernel_median"] = round(row["torch_root"]["median_us"] / row["root_in_kernel"]["median_us"], 2)
        row["root_in_kernel_over_noise_in_kernel_median"] = round(row["root_in_kernel"]["median_us"]
                                                                  / row["noise_in_kernel"]["median_us"], 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


def main_unroll(args):
    import numpy as np

    import muax_amd as mx
    from muax_amd.utils import warm_runtime
    from muax_amd.vector import value_priorities
    warm_runtime()
    repeats, inner, od, e, support, L = max(15, args.repeats), 10, 16, 16, 10, 10
    rows = []
    for batch in (32, 4096):
        rng = np.random.default_rng(batch)
        b = mx.Transition(obs=torch.from_numpy(rng.uniform(0, 1, (batch, L, od)).astype(np.float32)).cuda(),
                          a=torch.from_numpy(rng.integers(0, A, (batch, L)).astype(np.int32)).cuda(),
                          r=torch.from_numpy(rng.uniform(-1, 2, (batch, L)).astype(np.float32)).cuda(),
                          Rn=torch.from_numpy(rng.uniform(-5, 9, (batch, L)).astype(np.float32)).cuda(),
                          pi=torch.from_numpy(rng.dirichlet(np.ones(A), (batch, L)).astype(np.float32)).cuda())
        net = mx.create_stochastic_muzero_network(e, A, C, 2 * support + 1, generator=torch.Generator().manual_seed(1))
        m = mx.MuZero(net, policy="stochastic", support_size=support, stochastic_unroll_values=True)
        m.init(0, np.zeros((1, od), np.float32))
        calls = {"kernel": lambda: m.unroll_values(b, backend="hip"), "torch": lambda: m.unroll_values(b, backend="torch"),
                 "one_priority_torch": lambda: value_priorities(m, b)}  # (fit_vector's step with priority_steps=None)

        def many(fn):
            for _ in range(inner):
                fn()
        for fn in calls.values():
            many(fn)
        t = {k: [] for k in calls}
        for _ in range(repeats):  # alternating
            for k, fn in calls.items():
                t[k].append(wall(lambda: many(fn)) / inner)
        pk, pt = calls["kernel"]()[1], calls["torch"]()[1]
        row = {"A": A, "C": C, "E": e, "F": 2 * support + 1, "obs_dim": od, "windows": batch, "k_prio": L, "repeats": repeats,
               "calls_per_sample": inner, "kernel_against_torch_of_largest": float((pk - pt).abs().max() / pt.max())}
        for k, v in t.items():
            row[k] = {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}
        row["torch_over_kernel_median"] = round(row["torch"]["median_us"] / row["kernel"]["median_us"], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out")
    ap.add_argument("--mlp", action="store_true")
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--shape", type=int, nargs=5, metavar=("A", "C", "E", "SUPPORT", "OBS"),
                    help="--train: time this shape instead of 2048's two (built on demand where the library lists none)")
    ap.add_argument("--act", action="store_true")
    ap.add_argument("--graph", action="store_true", help="--act: the models run with capture_graph=True")
    ap.add_argument("--unroll", action="store_true")
    args = ap.parse_args()
    if args.unroll:
        return main_unroll(args)
    if args.act:
        return main_act(args)
    if args.train:
        return main_train(args)
    if args.mlp:
        return main_mlp(args)
    rows = []
    for batch in (64, 1024):
        sto, det, handles = make(batch, args.sims)
        for _ in range(3):
            sto(), det()
        torch.cuda.synchronize()
        t = {"stochastic": [], "deterministic": []}
        for _ in range(args.repeats):  # alternating
            t["stochastic"].append(timed(sto))
            t["deterministic"].append(timed(det))
        row = {"roots": batch, "sims": args.sims}
        for k, v in t.items():
            row[k] = {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1),
                      "per_sim_us": round(statistics.median(v) / args.sims, 2)}
        row["depth_mean"] = {k: round(float(h.depth_sum.float().mean()) / args.sims, 2)
                             for k, h in zip(("stochastic", "deterministic"), handles)}
        rows.append(row)
        print(json.dumps(row))
        for h in handles:
            h.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
