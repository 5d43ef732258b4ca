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
without export."""
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


def run(out):
    sys.path.insert(0, ROOT)
    from muax_amd import _lib
    res = {}
    wide_cases(res)
    stochastic_cases(res)
    np.savez(out, **res)
    print(f"{sum(k.endswith('/action') for k in res)} cases, {len(res)} arrays -> {out} ({_lib.load()._name})")


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
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    run(args.out or "act_bits.npz")
