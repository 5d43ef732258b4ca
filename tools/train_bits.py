"""Loss and flat gradient of both fused training steps (loss.FusedLossGrad, loss.StochasticFusedLossGrad) over a fixed
list of seeded cases, written to an .npz -- for A/B runs of two builds that must agree bit for bit.

    python tools/train_bits.py --out a.npz            # the build of the tree this file lies in (or MUAX_AMD_LIB), one process
    python tools/train_bits.py --compare a.npz b.npz  # exact equality of every array (tobytes()); exit status 1 if not

Cases, the smallest that reach every path.  Deterministic trio: the listed instances (2, 8, 21) at obs_dim 4,
(4, 32, 21), (2, 8, 41) at obs_dim 17 and 128, a narrow on-demand instance (5, 12, 21) and the wide one (18, 8, 63);
batch 1, 17, 40 (a dead-row tail, two workgroups, more than eight wavefronts: each of the reduction's eight groups sums
more than one row); unroll 1, 2, 5; with and without sample_weight; divide_by_length both ways.  Stochastic family: the
four listed instances at obs_dim 1, 17, 32, the same batches, unroll 1, 2 and -- for (4, 32, 32, 63) -- the instance's
longest, with and without sample_weight."""
import argparse
import os
import re
import sys

import numpy as np
import torch

BATCHES, UNROLLS = (1, 17, 40), (1, 2, 5)
# (A, E, support, obs_dim)
TRIO = [(2, 8, 10, 4), (4, 32, 10, 6), (2, 8, 20, 17), (2, 8, 20, 128), (5, 12, 10, 4), (18, 8, 31, 9)]
# (A, C, E, support)
STOCH, STOCH_OBS = [(3, 2, 4, 8), (4, 32, 16, 10), (4, 17, 8, 8), (4, 32, 32, 31)], (1, 17, 32)


def noisy_biases(m, g):
    with torch.no_grad():
        for p in [p for mod in m.network for p in mod.parameters()]:
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=g).to(p.device))


def batch(mx, B, L, A, obs_dim, seed):
    rng = np.random.default_rng(seed)
    f = np.float32
    return mx.Transition(obs=rng.uniform(-1, 1, (B, L, obs_dim)).astype(f), a=rng.integers(0, A, (B, L)),
                         r=rng.uniform(-2, 3, (B, L)).astype(f), Rn=rng.uniform(-30, 60, (B, L)).astype(f),
                         pi=rng.dirichlet(np.ones(A), (B, L)).astype(f)), rng.uniform(0.2, 3.0, B).astype(f)


def run(out):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import muax_amd as mx
    from muax_amd import _jit, _lib
    res = {}

    def put(key, f, b, **kw):
        loss, grads = f(b, **kw)
        res[key + "/loss"], res[key + "/grads"] = loss.cpu().numpy().copy(), grads.cpu().numpy().copy()

    for si, (A, E, S, od) in enumerate(TRIO):
        g = torch.Generator().manual_seed(100 + si)
        F = 2 * S + 1
        net = mx.nn.MZNetwork(mx.nn.Representation(E, generator=g), mx.nn.Prediction(A, F, generator=g),
                              mx.nn.Dynamic(E, A, F, generator=g))
        m = mx.MuZero(net, support_size=S)
        m.init(0, np.zeros((1, od)))
        noisy_biases(m, g)
        f = mx.loss.FusedLossGrad(m)
        if (A, E, F) == (5, 12, 21):
            assert _jit.ensure_train_instance(A, E, F), _jit.build_log_tail()
        if A > 16:
            assert _jit.ensure_wide_train_instance(A, E, F), _jit.build_log_tail()
        for B in BATCHES:
            for L in UNROLLS:
                b, w = batch(mx, B, L, A, od, 1000 * si + 10 * B + L)
                for sw in (None, torch.from_numpy(w).cuda()):
                    for dbl in (False, True):
                        put(f"trio{(A, E, F)}/obs{od}/B{B}/L{L}/sw{int(sw is not None)}/dbl{int(dbl)}", f, b,
                            divide_by_length=dbl, sample_weight=sw)
    for si, (A, Cn, E, S) in enumerate(STOCH):
        for od in STOCH_OBS:
            g = torch.Generator().manual_seed(200 + 10 * si + od)
            net = mx.create_stochastic_muzero_network(E, A, Cn, 2 * S + 1, generator=g)
            m = mx.MuZero(net, support_size=S)
            m.init(0, np.zeros((1, od)))
            noisy_biases(m, g)
            m.weights_changed()
            f = mx.loss.StochasticFusedLossGrad(m)
            unrolls = [1, 2]
            if (A, Cn, E, S) == (4, 32, 32, 31):  # the instance's longest unroll, read off its own refusal (no launch)
                try:
                    f(batch(mx, 1, 1000, A, od, 0)[0])
                    raise SystemExit("an unroll of 1000 was not refused")
                except _lib.TooLargeForLds as e:
                    unrolls.append(int(re.search(r"at most (\d+)", str(e)).group(1)))
            for B in BATCHES:
                for L in unrolls:
                    b, w = batch(mx, B, L, A, od, 5000 + 1000 * si + 10 * B + L + od)
                    for sw in (None, torch.from_numpy(w).cuda()):
                        put(f"stoch{(A, Cn, E, 2 * S + 1)}/obs{od}/B{B}/L{L}/sw{int(sw is not None)}", f, b, sample_weight=sw)
    torch.cuda.synchronize()
    np.savez(out, **res)
    print(f"{len(res) // 2} cases -> {out} ({_lib.load()._name})")


def compare(a, b):
    x, y = np.load(a), np.load(b)
    if sorted(x.files) != sorted(y.files):
        print("the two files hold different cases")
        return 1
    for k in x.files:  # (in the order the cases ran)
        if x[k].dtype != y[k].dtype or x[k].shape != y[k].shape or x[k].tobytes() != y[k].tobytes():
            print(f"first difference: {k}")
            return 1
        if not np.isfinite(x[k]).all():
            print(f"not finite: {k}")
            return 1
    print(f"{len(x.files) // 2} cases, {len(x.files)} arrays: all equal")
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar="NPZ")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    run(args.out or "train_bits.npz")
