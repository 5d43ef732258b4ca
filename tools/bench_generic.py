"""Per-act time of the three routes a default-trio act() can take, on one shape: the tuned fused instance, the generic
one-launch search (MZS_FORCE_GENERIC=1 on a handle with allow_generic), and -- for shapes without an instance -- the
generic route alone.   python tools/bench_generic.py
--wide: 17..64 actions at 4096 roots x 50 simulations under the MuZero and the Gumbel policy, the wide-action kernel (its
opt-in ONLY) beside the generic route (allow_generic ONLY) and the metric's listed instance, alternated, medians and spread
of the alternations; --wide-one POLICY: one run of the A = 18 wide launch (25 acts), the target of a rocprofv3 trace."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import haiku_style_weights  # noqa: E402
from muax_amd import MuZeroSearch, SearchConfig  # noqa: E402
from muax_amd.utils import warm_runtime  # noqa: E402

warm_runtime()  # (the runtime's signal pool grown before anything is timed: tools/diag_stall.py)


def run(B, obs_dim, E, A, S, force_generic, wide=False, gumbel=False):
    """wide: the wide-action kernel's opt-in of the policy and NOT the generic route (a decline raises, nothing is timed on
    another route by accident); gumbel: the Gumbel policy with mctx's defaults (completed_by_mix_value, 16 considered)."""
    w = haiku_style_weights(0, obs_dim, E, A, 21)
    cfg = SearchConfig(A, S, E, tiebreak=False, policy="gumbel", qtransform="qtransform_completed_by_mix_value",
                       max_num_considered_actions=16) if gumbel else SearchConfig(A, S, E, tiebreak=True)
    s = MuZeroSearch(B, cfg)
    s.set_mlp_weights(w, obs_dim, 10, 0.99)
    if wide:
        s.allow_wide(gumbel=gumbel)
    else:
        s.allow_generic()
    if force_generic:
        os.environ["MZS_FORCE_GENERIC"] = "1"
    else:
        os.environ.pop("MZS_FORCE_GENERIC", None)
    obs = (torch.rand(B, obs_dim) * 2 - 1).cuda()
    noise = None if gumbel else torch.distributions.Dirichlet(torch.full((A,), 0.3)).sample((B,)).cuda()
    for i in range(5):
        s.act_mlp(obs, (0, i), dirichlet_noise=noise)
    torch.cuda.synchronize()
    n = 20
    ts = []
    for i in range(n):  # the MEDIAN of per-act times: one host stall of the runtime (tens of ms, tools/diag_stall.py) in 20
        t0 = time.perf_counter()  # acts is otherwise the whole figure
        s.act_mlp(obs, (0, 100 + i), dirichlet_noise=noise)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    dt = sorted(ts)[n // 2]
    depth = float(s.depth_sum.float().mean()) / S
    s.close()
    os.environ.pop("MZS_FORCE_GENERIC", None)
    return dt, depth


def run_jit(B, obs_dim, E, A, S, gumbel=True):
    """The same shape through an instance built on demand (muax_amd/_jit.py), or None when no instance can exist.
    gumbel=False: an instance planned for the MuZero policy's record alone (round 6)."""
    from muax_amd import _jit
    if _jit.plan(A, E, 21, S, gumbel) is None or not _jit.ensure_instance(A, E, 21, S, gumbel=gumbel):
        return None
    return run(B, obs_dim, E, A, S, False) + (_jit.plan(A, E, 21, S, gumbel),)


def guarded(label, fn):
    """A shape that fails is a ROW of the table (profiles/r05_generic_route.txt committed a raw traceback instead)."""
    try:
        return fn()
    except Exception as e:  # noqa: BLE001
        print(f"{label}: FAILED -- {type(e).__name__}: {str(e)[:200]}")
        return None


def wide_table(rounds=5):
    """Wide-action kernel | generic route | the metric's listed instance, under both policies, one after the other `rounds`
    times on one box (each run: 5 settling acts, the median of 20 timed ones); the table gives the medians over the rounds
    and their spread (min .. max)."""
    from muax_amd.search import wide_plan
    shapes = tuple(sh + (pol,) for pol in ("muzero", "gumbel")
                   for sh in ((4096, 4, 8, 18, 50), (4096, 4, 8, 32, 50), (4096, 4, 8, 64, 50), (4096, 8, 32, 18, 50)))
    t = {k: [] for k in [("ref",)] + [(sh, r) for sh in shapes for r in ("wide", "generic")]}
    depth = {}
    for _ in range(rounds):
        t[("ref",)].append(run(4096, 4, 8, 2, 50, False)[0])
        for sh in shapes:
            for route in ("wide", "generic"):
                r = guarded(f"{sh} {route}", lambda: run(*sh[:5], False, wide=route == "wide", gumbel=sh[5] == "gumbel"))
                if r:
                    t[(sh, route)].append(r[0])
                    depth[sh] = r[1]
    med = lambda v: sorted(v)[len(v) // 2] if v else float("nan")  # noqa: E731
    rng = lambda v: f"{min(v) * 1e3:.3f} .. {max(v) * 1e3:.3f}" if v else "-"  # noqa: E731
    t_ref = med(t[("ref",)])
    print(f"reference: 4096 roots, A=2, E=8, S=50, listed instance {t_ref * 1e3:.3f} ms = {t_ref / 50 * 1e6:.2f} us/sim "
          f"(median of {rounds} alternations; min {min(t[('ref',)]) * 1e3:.3f}, max {max(t[('ref',)]) * 1e3:.3f})")
    for sh in shapes:
        B, od, E, A, S, pol = sh
        pl = wide_plan(A, E, 10, S, policy=pol)
        tw, tg = med(t[(sh, "wide")]), med(t[(sh, "generic")])
        per = lambda x: (x / S) / (t_ref / 50) * 4096 / B  # noqa: E731
        plan = (f"{pl['waves']} roots/workgroup, {pl['lds_bytes']} B LDS, {pl['roots_per_cu']} roots/CU, embeddings in "
                f"{'LDS' if pl['emb_lds'] else 'HBM'}") if pl else "declined"
        print(f"{pol:6s} {B} roots, A={A}, E={E}, S={S} (mean depth {depth.get(sh, float('nan')):.1f}): wide {tw * 1e3:8.3f} ms "
              f"({rng(t[(sh, 'wide')])}) = {tw / S * 1e6:6.2f} us/sim = x{per(tw):.1f} | generic route {tg * 1e3:8.3f} ms "
              f"({rng(t[(sh, 'generic')])}) = {tg / S * 1e6:6.2f} us/sim = x{per(tg):.1f} | wide is x{tg / tw:.2f} faster | "
              f"plan: {plan}", flush=True)


if __name__ == "__main__":
    if "--wide-one" in sys.argv:  # one wide-route run of 4096 x (A = 18, E = 8) x 50, for a profiler: --wide-one muzero|gumbel
        pol = sys.argv[sys.argv.index("--wide-one") + 1]
        dt, d = run(4096, 4, 8, 18, 50, False, wide=True, gumbel=pol == "gumbel")
        print(f"{pol} 4096 roots, A=18, E=8, S=50 (mean depth {d:.1f}): wide {dt * 1e3:.3f} ms per act")
        sys.exit(0)
    if "--wide" in sys.argv:
        wide_table(int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5)
        sys.exit(0)
    if "--round6" in sys.argv:
        # round 6: (a) instances planned per policy (the MuZero policy's four-word children: more roots per workgroup),
        # per simulation against the metric's listed instance; (b) the generic route where B (S + 1)^2 path words used to
        # exceed the 1 GiB slab (4096 roots x 300 simulations), undivided (8 GiB budget) and in chunks (forced)
        t_ref, _ = run(4096, 4, 8, 2, 50, False)
        print(f"reference: 4096 roots, A=2, E=8, S=50, listed instance {t_ref * 1e3:.3f} ms = {t_ref / 50 * 1e6:.2f} us/sim")
        for (B, od, E, A, S) in ((4096, 4, 8, 2, 160), (4096, 4, 8, 9, 50), (4096, 4, 8, 12, 50), (4096, 4, 8, 16, 50),
                                 (4096, 4, 8, 18, 50)):
            label = f"{B} roots, A={A}, E={E}, S={S}"
            os.environ["MUAX_AMD_JIT"] = "1"
            for gumbel in (True, False):
                r = guarded(label, lambda: run_jit(B, od, E, A, S, gumbel))
                if r is None:
                    print(f"{label}: no {'all-modes' if gumbel else 'MuZero-only'} instance")
                    continue
                t_j, d, pl = r
                print(f"{label} (mean depth {d:.1f}): {'all-modes  ' if gumbel else 'MuZero-only'} instance (NMAX {pl[1]}, "
                      f"{4 * pl[2]} roots/workgroup, paths in {'HBM' if pl[3] else 'LDS'}) {t_j * 1e3:8.3f} ms = "
                      f"{t_j / S * 1e6:6.2f} us/sim = x{(t_j / S) / (t_ref / 50) * 4096 / B:.1f} the listed instance's")
            os.environ["MUAX_AMD_JIT"] = "0"
            r = guarded(label, lambda: run(B, od, E, A, S, True))
            os.environ["MUAX_AMD_JIT"] = "1"
            if r:
                print(f"{label}: generic route {r[0] * 1e3:8.3f} ms = {r[0] / S * 1e6:6.2f} us/sim = "
                      f"x{(r[0] / S) / (t_ref / 50) * 4096 / B:.1f}")
        for budget in (None, "256"):
            if budget:
                os.environ["MZS_JUMP_BUDGET_MB"] = budget
            r = guarded("4096 roots, A=2, E=8, S=300", lambda: run(4096, 4, 8, 2, 300, False))
            if r:
                print(f"4096 roots, A=2, E=8, S=300 (mean depth {r[1]:.1f}): generic only, "
                      f"{'slab budget ' + budget + ' MB (chunks of roots)' if budget else 'undivided (8 GiB slab budget)'} "
                      f"{r[0] * 1e3:8.3f} ms = {r[0] / 300 * 1e6:6.2f} us/sim")
        os.environ.pop("MZS_JUMP_BUDGET_MB", None)
        sys.exit(0)
    if "--round5" in sys.argv:
        # round 5: shapes beyond round 4's instance limits (A <= 8, S <= 127) -- generic one-launch search against the
        # instance now built on demand (A <= 16; 128..255 simulations with the root paths in HBM), per simulation, next
        # to the metric's own instance (4096 x (2, 8) x 50: the reference for "a listed instance's per-simulation cost")
        t_ref, _ = run(4096, 4, 8, 2, 50, False)
        print(f"reference: 4096 roots, A=2, E=8, S=50, listed instance {t_ref * 1e3:.3f} ms = {t_ref / 50 * 1e6:.2f} us/sim")
        for (B, od, E, A, S) in ((4096, 4, 8, 2, 160), (4096, 4, 8, 2, 255), (4096, 4, 8, 9, 50), (4096, 4, 8, 12, 50),
                                 (4096, 4, 8, 16, 50), (4096, 8, 32, 4, 200), (4096, 4, 8, 6, 100), (1024, 4, 8, 16, 50),
                                 (1024, 4, 8, 2, 255)):
            os.environ["MUAX_AMD_JIT"] = "0"
            t_g, d = run(B, od, E, A, S, True)
            os.environ["MUAX_AMD_JIT"] = "1"
            r = run_jit(B, od, E, A, S)
            if r is None:
                print(f"{B} roots, A={A}, E={E}, S={S}: generic {t_g * 1e3:8.3f} ms = {t_g / S * 1e6:6.2f} us/sim | no instance possible")
                continue
            t_j, _, pl = r
            print(f"{B} roots, A={A}, E={E}, S={S} (mean depth {d:.1f}): generic {t_g * 1e3:8.3f} ms = {t_g / S * 1e6:6.2f} us/sim | "
                  f"on-demand instance (NMAX {pl[1]}, {4 * pl[2]} roots/workgroup, paths in {'HBM' if pl[3] else 'LDS'}) "
                  f"{t_j * 1e3:8.3f} ms = {t_j / S * 1e6:6.2f} us/sim = x{(t_j / S) / (t_ref / 50) * 4096 / B:.1f} the listed instance's per-root-simulation cost "
                  f"(generic: x{(t_g / S) / (t_ref / 50) * 4096 / B:.1f})")
        sys.exit(0)
    for (B, od, E, A, S) in ((4096, 4, 8, 2, 50), (8192, 8, 32, 4, 50)):
        t_f, d = run(B, od, E, A, S, False)
        t_g, _ = run(B, od, E, A, S, True)
        print(f"{B} roots, A={A}, E={E}, S={S} (mean depth {d:.1f}): fused instance {t_f * 1e3:8.3f} ms = {t_f / S * 1e6:6.2f} us/sim | "
              f"generic {t_g * 1e3:8.3f} ms = {t_g / S * 1e6:6.2f} us/sim | x{t_g / t_f:.1f}")
    for (B, od, E, A, S) in ((4096, 4, 8, 2, 300), (4096, 4, 8, 18, 50), (1024, 8, 100, 4, 50)):  # (no instance can serve these)
        r = guarded(f"{B} roots, A={A}, E={E}, S={S}", lambda: run(B, od, E, A, S, False))
        if r is None:
            continue
        t_g, d = r
        print(f"{B} roots, A={A}, E={E}, S={S} (mean depth {d:.1f}): generic only {t_g * 1e3:8.3f} ms = {t_g / S * 1e6:6.2f} us/sim")
