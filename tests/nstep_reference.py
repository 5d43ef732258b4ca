"""Plain-loop float64 reference of the n-step fields the device replay computes ("Adding" and
"Reanalysis"), for test_nstep_reference_cpu.py and test_gpu_replay_kernels.py.  One transition at a time, Python floats
(IEEE double) and explicit loops: no array arithmetic, nothing from muax_amd but prng, and in particular not
`vector.nstep_returns`, which the older tests share with the product.

The arithmetic is the one DESIGN 4.7 spells out, in its order:

    Rn = 0;  for i = 0 .. n-1:  Rn = Rn + gamma**i * (r[t+i], or 0 past the end)
    Rn = Rn + v[t+n] * gamma**n   when step t+n exists (the bootstrap);  done = there was none
    w  = |v[t] - Rn| ** alpha     (1 without alpha)
    cw = the running sum of w, one addition per transition;  episode weight = cw[last] / T ("mean") or cw[last] ("sum")

with gamma**i taken as `float(gamma) ** i`, the way replay_device.py fills the table it uploads.  No imports at all."""


def transition(r, v, t, n, gamma, alpha=None):
    """(Rn, done, w) of transition t of the episode with rewards r[0..T) and values v[0..T)."""
    T, g = len(r), float(gamma)
    Rn = 0.0
    for i in range(n):
        Rn += g ** i * (float(r[t + i]) if t + i < T else 0.0)
    boot = t + n < T
    if boot:
        Rn += float(v[t + n]) * g ** n
    w = 1.0 if alpha is None else abs(float(v[t]) - Rn) ** float(alpha)
    return Rn, not boot, w


def episode(r, v, n, gamma, alpha=None, weight="mean"):
    """(Rn [T], done [T], w [T], cw [T], episode weight) as Python lists of floats / bools."""
    assert weight in ("mean", "sum")
    T = len(r)
    Rn, done, w, cw = [], [], [], []
    carry = 0.0
    for t in range(T):
        x, d, y = transition(r, v, t, n, gamma, alpha)
        carry += y
        Rn.append(x), done.append(d), w.append(y), cw.append(carry)
    return Rn, done, w, cw, (cw[-1] / T if weight == "mean" else cw[-1])


def terms(r, v, t, n, gamma):
    """The addends of Rn[t] (those past the end left out), for a rounding bound on a sum taken in another order."""
    T, g = len(r), float(gamma)
    out = [g ** i * float(r[t + i]) for i in range(n) if t + i < T]
    if t + n < T:
        out.append(float(v[t + n]) * g ** n)
    return out
