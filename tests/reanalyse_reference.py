"""NumPy restatement of what `DeviceReplayBuffer.reanalyse` must leave in the arenas ("Reanalysis"), for
test_reanalyse_cpu.py and test_gpu_reanalyse.py.  Built on vector.nstep_returns, np.abs(...) ** alpha and np.cumsum; it
shares nothing with the kernels."""
import numpy as np

from muax_amd import vector


def targets(r, pi, v, n, gamma, alpha=None, weight="mean"):
    """The stored rewards `r` (float32) of one episode with the new search results `pi` [T, A], `v` [T] (float32) ->
    (Rn float32 [T], done bool [T], w float64 [T], cw float64 [T], the episode's buffer weight).  `pi` passes through
    unchanged: it is an argument so that a caller states the whole of what was searched."""
    r, v = np.asarray(r), np.asarray(v)
    assert r.dtype == np.float32 and v.dtype == np.float32 and np.asarray(pi).dtype == np.float32
    v64 = v.astype(np.float64)
    Rn, done = vector.nstep_returns(r.astype(np.float64), v64, n, gamma)
    w = np.ones_like(Rn) if alpha is None else np.abs(v64 - Rn) ** alpha
    cw = np.cumsum(w)
    return Rn.astype(np.float32), done, w, cw, float(w.mean() if weight == "mean" else w.sum())
