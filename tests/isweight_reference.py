"""Plain-loop float64 restatement of the importance-sampling weights of the device replay, for
test_isweight_cpu.py and test_gpu_isweight.py.  Built on tests/replay_reference.py (the draws, the prefix sums, the
searches); it shares nothing with the kernels.  Episodes are replay_reference's dicts, oldest first."""
import numpy as np

import replay_reference as rr

F32 = np.float32


def eligible_windows(lengths, k):
    """N: the windows of k transitions a sample can draw -- len - k of every episode LONGER than k."""
    n = 0
    for T in lengths:
        if T > k:
            n += int(T) - k
    return n


def episode_probability(episodes, e, k):
    """p_e: the share of episode e in the buffer weights of the episodes longer than k (1 when they are all zero)."""
    CW = rr.episode_cw([ep["weight"] for ep in episodes], [len(ep["w"]) for ep in episodes], k)
    total = CW[-1]
    if total == 0.0:
        return 1.0
    return float((CW[e] - (CW[e - 1] if e > 0 else 0.0)) / total)


def start_probability(w, s, k):
    """p_s: the share of transition s in the weights of the m = len(w) - k possible starts (1 / m when all are zero)."""
    m = len(w) - k
    cw = np.cumsum(np.asarray(w, np.float64))[:m]
    tot = cw[-1]
    if tot == 0.0:
        return 1.0 / float(m)
    return float((cw[s] - (cw[s - 1] if s > 0 else 0.0)) / tot)


def window_probability(episodes, e, s, k):
    """q: the probability that one batch row is window (e, s)."""
    return episode_probability(episodes, e, k) * start_probability(episodes[e]["w"], s, k)


def raw_weight(N, q, beta):
    x = float(N) * q
    if beta == 1:
        return 1.0 / x
    return float(np.power(np.float64(x), np.float64(-beta)))


def sample_rows(key, episodes, B, k, sample_per_trajectory=1):
    """(episode [B], start [B]) as the kernel draws them; start -1 marks a zero-filled row (every buffer weight zero
    and the newest episode no longer than k)."""
    lengths = [len(ep["w"]) for ep in episodes]
    CW = rr.episode_cw([ep["weight"] for ep in episodes], lengths, k)
    if CW[-1] != 0.0:
        return rr.sample_indices(key, episodes, B, k, sample_per_trajectory)
    last = len(episodes) - 1
    _, u1 = rr.draws(key, B, sample_per_trajectory)
    start = [rr.pick_start(u1[j], episodes[last]["w"], k) if lengths[last] > k else -1 for j in range(B)]
    return np.full(B, last), np.array(start)


def weights(key, episodes, B, k, sample_per_trajectory=1, beta=1.0, normalize=True):
    """dict(e, start, q [B] f64, raw [B] f64, isw [B] f32, N) of one batch."""
    e, start = sample_rows(key, episodes, B, k, sample_per_trajectory)
    N = eligible_windows([len(ep["w"]) for ep in episodes], k)
    q, raw = np.zeros(B), np.zeros(B)
    for j in range(B):
        if start[j] < 0:
            continue  # a zero-filled row: raw 0
        q[j] = window_probability(episodes, int(e[j]), int(start[j]), k)
        raw[j] = raw_weight(N, q[j], beta)
    isw = np.zeros(B, F32)
    top = 0.0
    for j in range(B):
        top = raw[j] if raw[j] > top else top
    for j in range(B):
        if normalize:
            isw[j] = F32(raw[j] / top) if top > 0.0 else F32(0.0)
        else:
            isw[j] = F32(raw[j])
    return dict(e=e, start=start, q=q, raw=raw, isw=isw, N=N)
