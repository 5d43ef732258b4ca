"""Every output of the two one-launch search kernels with one root per wavefront (mz_wide.cuh through act_mlp with
allow_wide only, mz_stoch_wide.cuh through search_stochastic_mlp(one_launch=True)) over a fixed list of seeded cases,
written to an .npz -- for A/B runs of two builds that must agree bit for bit.

    python tools/act_bits.py --out a.npz            # the build of the tree this file lies in (or MUAX_AMD_LIB), one process
    python tools/act_bits.py --compare a.npz b.npz  # exact equality of every array (tobytes()); exit status 1 if not

Each case records the action, the action weights, the search value, the depth sum and, with a tree export, every tree
array.  Cases, the smallest that reach every shared piece (mz_wave_tree.cuh).  Wide kernel: its four modes (MuZero policy
with and without tie-break noise, Gumbel policy with either qtransform) x A in 17, 33, 64 x E in 8, 64 at 12 simulations
x {plain, mask + Dirichlet noise, max_depth 3} x with / without export; per mode one chain of 110 simulations (one
action dominates the prior: backup over two chunks of 64 levels) and the longest search at 64 x 64 whose plan keeps the embeddings in HBM.
Stochastic kernel: SEARCH_CASES of tests/test_gpu_stochastic_one_launch.py (both tie-break settings are among them) x
eager / captured (the captured launch reads key, temperature and Dirichlet fraction from the device block) x with /
without export.

    python tools/act_bits.py --set mlp --out a.npz  # the kernels on the run-time-shape MLP blocks (mz_mlp_blocks.cuh)

Generic route (allow_generic only, MZS_FORCE_GENERIC=1; 5 roots, 12 simulations): A in 1, 16, 17, 33, 64 x E in 1, 5, 64
with obs_dim in 1, 9, 128 and support 8 / 31 rotating over them, x both policies x pred_on_parent x with / without
export; mask + Dirichlet noise; 2049 roots (the 128-register build, 32-bit weight offsets); the shortest search whose
LDS plan has no room for the pUCT table.  Stochastic step-wise recurrent step: the same SEARCH_CASES through
search_stochastic_mlp(one_launch=False), eager, with export, and stochastic_mlp_recurrent itself on three shapes with
both parent kinds mixed and the slots at both clamps.  Unroll (mzs_mlp_unroll_values): three shapes x k_prio 1 / 5 of
L = 5 with an action outside 0..A-1 and a NaN return, both outputs, values only, priorities only."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
# (tiebreak, policy, qtransform) of the wide kernel's modes 0..3
WIDE_MODES = [(False, "muzero", "qtransform_by_parent_and_siblings"), (True, "muzero", "qtransform_by_parent_and_siblings"),
              (False, "gumbel", "qtransform_by_parent_and_siblings"), (False, "gumbel", "qtransform_completed_by_mix_value")]


def tree_arrays(out):
    return {} if out.search_tree is None else {"tree." + f: getattr(out.search_tree, f) for f in out.search_tree._fields}


def record(res, key, s, out):
    torch.cuda.synchronize()
    arrays = dict(action=out.action, weights=out.action_weights, value=s.search_value, depth_sum=s.depth_sum, **tree_arrays(out))
    for n, t in arrays.items():
        res[f"{key}/{n}"] = t.cpu().numpy().copy()


def wide_cases(res):
    from muax_amd import MuZeroSearch, SearchConfig
    from muax_amd.search import wide_plan
    from oracle import pyoracle as po
    B, obs_dim, support = 9, 6, 10

    def run(mode, A, E, S, variant, chain=False):
        tiebreak, policy, qt = WIDE_MODES[mode]
        seed = 1000 * mode + 10 * A + E + S
        w = po.random_mlp_weights(seed, obs_dim, E, A, 2 * support + 1, bias_scale=0.1)
        if chain:
            w["pp_b2"] = np.array([7.0] + [-7.0] * (A - 1), F32)
        rng = np.random.default_rng(seed + 1)
        obs = torch.from_numpy(rng.uniform(-1, 1, (B, obs_dim)).astype(F32))
        noise = torch.from_numpy(rng.dirichlet([0.3] * A, B).astype(F32))
        invalid = (rng.uniform(size=(B, A)) < 0.2).astype(np.uint8)
        invalid[np.arange(B), rng.integers(0, A, B)] = 0
        masked = variant == "mask+noise"
        s = MuZeroSearch(B, SearchConfig(A, S, E, tiebreak=tiebreak, policy=policy, qtransform=qt, max_num_considered_actions=8,
                                         max_depth=3 if variant == "max_depth" else None))
        s.set_mlp_weights({k: torch.from_numpy(v) for k, v in w.items()}, obs_dim, support, 0.99, "child")
        s.allow_wide(gumbel=policy == "gumbel")
        for with_tree in (True, False):
            args = dict(invalid_actions=torch.from_numpy(invalid) if masked else None, with_tree=with_tree)
            if masked and policy == "muzero":
                args["dirichlet_noise"] = noise
            record(res, f"wide{mode}/A{A}/E{E}/S{S}/{variant}/tree{int(with_tree)}", s, s.act_mlp(obs, [3, seed], **args))
        s.close()

    for mode in range(4):
        for A in (17, 33, 64):
            for E in (8, 64):
                for variant in ("plain", "mask+noise", "max_depth"):
                    run(mode, A, E, 12, variant)
        run(mode, 18, 8, 110, "chain", chain=True)
        plans = ((S, wide_plan(64, 64, support, S, WIDE_MODES[mode][1])) for S in range(110, 1, -1))
        run(mode, 64, 64, next(S for S, pl in plans if pl is not None and not pl["emb_lds"]), "emb_hbm")


def stochastic_cases(res):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import stochastic_mlp_reference as smr
    import test_gpu_stochastic_one_launch as t
    from muax_amd import MuZeroSearch, SearchConfig
    for ci, case in enumerate(t.SEARCH_CASES):
        if case == "emb_hbm":
            E, S = t._emb_hbm_shape()
            case = (3, 5, E, 10, 2, S, False, False, None)
        A, Cn, E, support, B, S, tiebreak, masked, max_depth = case
        w = smr.random_weights(11, A, Cn, E, support)
        rng = np.random.default_rng([7, A, Cn, E, B, S])
        root = tuple(torch.from_numpy(x).cuda() for x in (rng.standard_normal((B, A)).astype(F32), rng.uniform(-3, 3, B).astype(F32),
                                                          rng.uniform(0, 1, (B, E)).astype(F32)))
        invalid = (rng.uniform(size=(B, A)) < 0.3).astype(np.uint8)
        invalid[:, 0] = 0
        noise = torch.from_numpy(rng.dirichlet([0.3] * A, B).astype(F32)).cuda()
        s = MuZeroSearch(B, SearchConfig(A, S, E, policy="stochastic", num_chance_outcomes=Cn, tiebreak=tiebreak, max_depth=max_depth))
        s.set_stochastic_mlp_weights({k: torch.from_numpy(v).cuda() for k, v in w.items()}, support, 0.97)
        for graph in (False, True):
            for with_tree in (True, False):
                out = s.search_stochastic_mlp(root, key=[4, 5 + ci], invalid_actions=torch.from_numpy(invalid).cuda() if masked else None,
                                              dirichlet_noise=noise, temperature=0.5, with_tree=with_tree, graph=graph, one_launch=True)
                record(res, f"stoch{ci}{case[:6]}/block{int(graph)}/tree{int(with_tree)}", s, out)
        s.close()


def generic_cases(res):
    from muax_amd import MuZeroSearch, SearchConfig
    from oracle import pyoracle as po

    def run(name, A, E, obs_dim, support, policy, pred_on, B=5, S=12, masked=False, trees=(True, False)):
        seed = 100 * A + E + obs_dim + support
        w = po.random_mlp_weights(seed, obs_dim, E, A, 2 * support + 1, bias_scale=0.1)
        rng = np.random.default_rng(seed + 1)
        obs = torch.from_numpy(rng.uniform(-1, 1, (B, obs_dim)).astype(F32))
        noise = torch.from_numpy(rng.dirichlet([0.3] * A, B).astype(F32))
        invalid = (rng.uniform(size=(B, A)) < 0.2).astype(np.uint8)
        invalid[np.arange(B), rng.integers(0, A, B)] = 0
        s = MuZeroSearch(B, SearchConfig(A, S, E, tiebreak=False, policy=policy, qtransform=(
            "qtransform_completed_by_mix_value" if policy == "gumbel" else "qtransform_by_parent_and_siblings")))
        s.set_mlp_weights({k: torch.from_numpy(v) for k, v in w.items()}, obs_dim, support, 0.99, pred_on)
        s.allow_generic()
        for with_tree in trees:
            args = dict(invalid_actions=torch.from_numpy(invalid) if masked else None, with_tree=with_tree)
            if masked and policy == "muzero":
                args["dirichlet_noise"] = noise
            out = s.act_mlp(obs, [9, seed], **args)
            key = f"generic/{name}/A{A}/E{E}/obs{obs_dim}/sup{support}/{policy}/{pred_on}/B{B}/S{S}/tree{int(with_tree)}"
            record(res, key, s, out)
            res[key + "/root_value"] = s.root_value.cpu().numpy().copy()
        s.close()

    for ia, A in enumerate((1, 16, 17, 33, 64)):
        for ie, E in enumerate((1, 5, 64)):
            obs_dim, support = (1, 9, 128)[(ia + ie) % 3], (8, 31)[(ia + ie) % 2]
            for policy in ("muzero", "gumbel"):
                for pred_on in ("child", "parent"):
                    run("grid", A, E, obs_dim, support, policy, pred_on)
    run("tail", 17, 5, 128, 8, "muzero", "child")  # E + A = 22: gen_linear's tail loop; obs_dim > E + A
    run("tail", 17, 5, 9, 31, "gumbel", "child")
    run("mask+noise", 17, 5, 9, 8, "muzero", "child", masked=True)
    run("occ4", 4, 8, 9, 8, "muzero", "child", B=2049, S=4)
    # launch_mlp_search: lds_tbl = 4 * 15 * (S + 2) + 4 * gen_scratch_words(E, A) + 4 * 2 * (S + 2) > 64 KiB
    scratch_words = (8 + 4 + 3) // 4 * 4 + 32 + 3 * 64 + (8 + 3) // 4 * 4 + 4  # gen_scratch_words(8, 4), mz_mlp_blocks.cuh
    S = next(S for S in range(1, 1024) if 68 * (S + 2) + 4 * scratch_words > 64 * 1024)
    run("no_table", 4, 8, 9, 8, "muzero", "child", B=2, S=S, trees=(True,))


def stochastic_stepwise_cases(res):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import stochastic_mlp_reference as smr
    import test_gpu_stochastic_one_launch as t
    from muax_amd import MuZeroSearch, SearchConfig

    def handle(A, Cn, E, support, B, S, **cfg):
        s = MuZeroSearch(B, SearchConfig(A, S, E, policy="stochastic", num_chance_outcomes=Cn, **cfg))
        s.set_stochastic_mlp_weights({k: torch.from_numpy(v).cuda() for k, v in smr.random_weights(11, A, Cn, E, support).items()},
                                     support, 0.97)
        return s

    for ci, case in enumerate(t.SEARCH_CASES):
        if case == "emb_hbm":
            E, S = t._emb_hbm_shape()
            case = (3, 5, E, 10, 2, S, False, False, None)
        A, Cn, E, support, B, S, tiebreak, masked, max_depth = case
        rng = np.random.default_rng([7, A, Cn, E, B, S])
        root = tuple(torch.from_numpy(x).cuda() for x in (rng.standard_normal((B, A)).astype(F32), rng.uniform(-3, 3, B).astype(F32),
                                                          rng.uniform(0, 1, (B, E)).astype(F32)))
        invalid = (rng.uniform(size=(B, A)) < 0.3).astype(np.uint8)
        invalid[:, 0] = 0
        noise = torch.from_numpy(rng.dirichlet([0.3] * A, B).astype(F32)).cuda()
        s = handle(A, Cn, E, support, B, S, tiebreak=tiebreak, max_depth=max_depth)
        out = s.search_stochastic_mlp(root, key=[4, 5 + ci], invalid_actions=torch.from_numpy(invalid).cuda() if masked else None,
                                      dirichlet_noise=noise, temperature=0.5, with_tree=True, one_launch=False)
        record(res, f"stepwise{ci}{case[:6]}", s, out)
        s.close()
    names = ("chance_logits", "afterstate_value", "afterstate_embedding", "action_logits", "value", "reward", "discount",
             "state_embedding")
    for A, Cn, E in ((1, 1, 1), (3, 5, 8), (40, 24, 64)):
        B = 5
        s = handle(A, Cn, E, 10, B, 2)
        rng = np.random.default_rng([A, Cn, E])
        emb = torch.from_numpy(rng.uniform(0, 1, (B, E)).astype(F32)).cuda()
        for swap in (0, 1):  # both kinds in one launch; row 0 at the clamp of its kind, the others anywhere in 0..A+C-1
            kind = ((np.arange(B) + swap) % 2).astype(np.int32)
            slot = rng.integers(0, A + Cn, B).astype(np.int32)
            slot[0] = A + Cn - 1 if kind[0] else 0
            s.stochastic_mlp_recurrent(torch.from_numpy(slot).cuda(), torch.from_numpy(kind).cuda(), emb)
            torch.cuda.synchronize()
            for n, buf in zip(names, s._stochastic_out[1]):
                res[f"recurrent/A{A}/C{Cn}/E{E}/swap{swap}/{n}"] = buf.cpu().numpy().copy()
        s.close()


def unroll_cases(res):
    import ctypes as C
    from muax_amd import _lib
    from oracle import pyoracle as po
    L_, B, L, support = _lib.load(), 5, 5, 10
    for obs_dim, E, A in ((1, 1, 1), (9, 5, 17), (128, 64, 64)):
        w = po.random_mlp_weights(40 + A, obs_dim, E, A, 2 * support + 1, bias_scale=0.1)
        dev = {n: torch.from_numpy(np.ascontiguousarray(w[n], F32)).cuda() for n in _lib.MLP_WEIGHT_NAMES}
        rng = np.random.default_rng([obs_dim, E, A])
        act = rng.integers(0, A, (B, L)).astype(np.int32)
        act[1, 0], act[2, 1] = A, -1  # outside 0..A-1: an all-zero one-hot
        Rn = rng.uniform(-3, 3, (B, L)).astype(F32)
        Rn[3, 0] = np.nan
        obs, act, Rn = (torch.from_numpy(x).cuda() for x in (rng.uniform(-1, 1, (B, obs_dim)).astype(F32), act, Rn))
        ws = _lib.args(_lib.MzsMlpWeights, obs_dim=obs_dim, support_size=support, discount=0.99,
                       **{n: t.data_ptr() for n, t in dev.items()})
        for kp in (1, 5):
            for which in ("both", "values", "prio"):
                out = torch.full((2, B, kp), -7.0, dtype=torch.float32, device="cuda")
                u = _lib.args(_lib.MzsUnrollArgs, device=torch.cuda.current_device(), batch=B, row_steps=L, k_prio=kp, num_actions=A,
                              embed_dim=E, obs=obs.data_ptr(), actions=act.data_ptr(), returns=Rn.data_ptr(),
                              values=out[0].data_ptr() if which != "prio" else None,
                              prio=out[1].data_ptr() if which != "values" else None)
                _lib.check(L_.mzs_mlp_unroll_values(C.byref(ws), C.byref(u), None))
                torch.cuda.synchronize()
                res[f"unroll/obs{obs_dim}/E{E}/A{A}/kp{kp}/{which}/out"] = out.cpu().numpy().copy()


def run(out, case_set):
    sys.path.insert(0, ROOT)
    from muax_amd import _lib
    res = {}
    if case_set == "mlp":
        os.environ["MZS_FORCE_GENERIC"] = "1"  # (read at every act: shapes with a fused instance take the generic route too)
        generic_cases(res)
        stochastic_stepwise_cases(res)
        unroll_cases(res)
        n_cases = len({k.rsplit("/", 1)[0] for k in res})
    else:
        wide_cases(res)
        stochastic_cases(res)
        n_cases = sum(k.endswith('/action') for k in res)
    np.savez(out, **res)
    print(f"{n_cases} cases, {len(res)} arrays -> {out} ({_lib.load()._name})")


def compare(a, b):
    x, y = np.load(a), np.load(b)
    if sorted(x.files) != sorted(y.files):
        print("the two files hold different cases")
        return 1
    for k in x.files:  # (in the order the cases ran)
        if x[k].dtype != y[k].dtype or x[k].shape != y[k].shape or x[k].tobytes() != y[k].tobytes():
            print(f"first difference: {k}")
            return 1
    print(f"{len(x.files)} arrays: all equal")
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar="NPZ")
    ap.add_argument("--set", choices=("wide", "mlp"), default="wide", help="the case set (default: the two one-launch kernels)")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    run(args.out or "act_bits.npz", args.set)
