"""NumPy float64 restatement of the device replay's sampling rules, for test_replay_cpu.py and
test_gpu_replay.py.  Built on prng.threefry2x32, np.cumsum and np.searchsorted(side="right"); it shares nothing with
the kernels.  An episode here is a dict of host arrays: obs [T, obs_dim] f32, a [T] i32, r / Rn / v [T] f32,
done [T] bool, pi [T, A] f32, w [T] f64, plus `weight` (the buffer weight, a float)."""
import numpy as np

from muax_amd import prng

F32 = np.float32


def uniform53(key, x0, x1):
    """((y0 << 32 | y1) >> 11) * 2^-53 of threefry2x32(key, x0, x1), float64 in [0, 1); arrays broadcast."""
    y0, y1 = prng.threefry2x32(key, x0, x1)
    bits = ((y0.astype(np.uint64) << np.uint64(32)) | y1.astype(np.uint64)) >> np.uint64(11)
    return bits.astype(np.float64) * 2.0 ** -53


def draws(key, B, sample_per_trajectory=1):
    rows = np.arange(B)
    return uniform53(key, rows // sample_per_trajectory, 0), uniform53(key, rows, 1)


def episode_cw(weights, lengths, k):
    """Inclusive prefix sums of the buffer weights, episodes no longer than k carrying none."""
    return np.cumsum(np.where(np.asarray(lengths) > k, np.asarray(weights, np.float64), 0.0))


def pick_episodes(u0, weights, lengths, k):
    CW = episode_cw(weights, lengths, k)
    return np.searchsorted(CW, u0 * CW[-1], side="right")


def pick_start(u1, w, k):
    """Start of one row inside an episode with transition weights w."""
    m = len(w) - k
    cw = np.cumsum(np.asarray(w, np.float64))[:m]
    if cw[-1] == 0:
        return int(np.floor(u1 * m))
    return int(np.searchsorted(cw, u1 * cw[-1], side="right"))


def sample_indices(key, episodes, B, k, sample_per_trajectory=1):
    """(episode index [B], start [B]) of a batch over `episodes` (oldest first)."""
    u0, u1 = draws(key, B, sample_per_trajectory)
    e = pick_episodes(u0, [ep["weight"] for ep in episodes], [len(ep["w"]) for ep in episodes], k)
    return e, np.array([pick_start(u1[j], episodes[e[j]]["w"], k) for j in range(B)])


def window(ep, start, k):
    """The fields of one batch row by direct slicing: what sample() must return for it."""
    s = slice(start, start + k)
    return dict(obs=ep["obs"][start][None], a=ep["a"][s], r=ep["r"][s], Rn=ep["Rn"][s], v=ep["v"][s], done=ep["done"][s],
                pi=ep["pi"][s], w=ep["w"][s].astype(F32))


def batch_fields(episodes, e, start, k):
    rows = [window(episodes[i], int(s), k) for i, s in zip(e, start)]
    return {n: np.stack([r[n] for r in rows]) for n in rows[0]}


def dyadic_weights(rng, n, zero_frac=0.0):
    """Multiples of 2^-10 below 2^10: every partial sum of a few thousand of them is exact in float64."""
    w = rng.integers(0, 1 << 20, n).astype(np.float64) / 1024.0
    if zero_frac:
        w[rng.uniform(size=n) < zero_frac] = 0.0
    return w


def make_episode(rng, T, A, obs_dim, w=None, weight=None):
    w = dyadic_weights(rng, T) if w is None else np.asarray(w, np.float64)
    return dict(obs=rng.uniform(-1, 1, (T, obs_dim)).astype(F32), a=rng.integers(0, A, T).astype(np.int32),
                r=rng.uniform(-2, 3, T).astype(F32), Rn=rng.uniform(-30, 60, T).astype(F32),
                v=rng.uniform(-30, 60, T).astype(F32), done=rng.uniform(size=T) < 0.2,
                pi=rng.dirichlet(np.ones(A), T).astype(F32), w=w,
                weight=float(dyadic_weights(rng, 1)[0] + 1.0) if weight is None else float(weight))


class ArenaModel:
    """Host model of the eviction rule: episodes are contiguous in an arena of max_steps rows and never split across
    its end; a new one evicts the oldest while the count would exceed `capacity` or no contiguous room is left.  With the
    live episodes in one stretch [lo, tail) the new one goes at `tail` when it fits before the end, else at row 0 when
    it fits below `lo`; with them wrapped ([lo, end) and [0, tail)) it goes at `tail` when it fits below `lo`."""

    def __init__(self, capacity, max_steps):
        self.capacity, self.max_steps = capacity, max_steps
        self.live, self.tail, self.next_serial = [], 0, 0  # live: [(serial, start, length)] oldest first

    def _room(self, T):
        if not self.live:
            return 0
        lo = self.live[0][1]
        if lo < self.tail:
            if self.tail + T <= self.max_steps:
                return self.tail
            return 0 if T <= lo else None
        return self.tail if self.tail + T <= lo else None

    def add(self, T):
        assert T <= self.max_steps
        while len(self.live) >= self.capacity:
            self.live.pop(0)
        while (dst := self._room(T)) is None:
            self.live.pop(0)
        self.live.append((self.next_serial, dst, T))
        self.next_serial += 1
        self.tail = dst + T
        spans = sorted((s, s + n) for _, s, n in self.live)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= self.max_steps

    @property
    def serials(self):
        return [s for s, _, _ in self.live]

    @property
    def steps(self):
        return sum(n for _, _, n in self.live)
