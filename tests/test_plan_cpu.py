"""The device plan's arithmetic on the host (no GPU): the plain-loop reference tests/plan_reference.py, which the GPU
tests hold the kernels against, must itself be `vector.ring_plan` and collect()'s `np.sum` returns, and the public
switches must refuse what they cannot serve."""

import numpy as np
import pytest

import muax_amd as mx
import plan_reference as plan
from muax_amd import _lib, vector


def _call(rng, T, N, p):
    return rng.random((T, N)) < p


def _ring_of(S, N, row0, D, R=None):
    """[S][N] ring planes holding the call's rows from ring row `row0` on; other rows are poison."""
    done = np.full((S, N), 7, np.int64)  # non-zero: a row read outside the call would end episodes
    r = np.full((S, N), 1e300)
    for t in range(D.shape[0]):
        done[(row0 + t) % S] = D[t]
        if R is not None:
            r[(row0 + t) % S] = R[t]
    return done.tolist(), r.tolist()


@pytest.mark.parametrize("min_length", [1, 3, 6, 100])
@pytest.mark.parametrize("T,N,S,p", [(1, 1, 4, 0.5), (7, 5, 20, 0.3), (13, 9, 30, 0.15), (8, 3, 30, 0.0), (5, 4, 12, 1.0)])
def test_reference_equals_ring_plan_over_two_calls(T, N, S, p, min_length):
    rng = np.random.default_rng(1000 * T + 10 * N + min_length)
    carried = rng.integers(0, S - 2 * T + 1, N)  # steps of the open episodes before the first call: both calls fit the ring
    step0 = int(carried.max()) + int(rng.integers(0, 3 * S))
    open_start = step0 - carried
    open_len, open_ret = carried.tolist(), [0.0] * N
    for _ in range(2):
        D = _call(rng, T, N, p)
        assert (np.asarray(open_len) + T).max() <= S  # (a call the collector accepts)
        finished, dropped, new_open = vector.ring_plan(D, open_start, step0, min_length)
        done, r = _ring_of(S, N, step0 % S, D, np.zeros((T, N)))
        ep, _, counts, open_len, open_ret = plan.plan_steps(done, r, step0 % S, T, S, open_len, open_ret, min_length)
        assert [(e, f, L) for e, f, L, s in ep if s] == [(e, f % S, L) for e, f, L in finished]
        assert [(e, f, L) for e, f, L, s in ep if not s] == [(e, f % S, L) for e, f, L in dropped]
        every = sorted(finished + dropped, key=lambda x: (x[0], x[1]))
        assert [(e, f, L) for e, f, L, _ in ep] == [(e, f % S, L) for e, f, L in every]  # the merged order
        assert counts == [len(every), len(finished), int((step0 + T - new_open).max()), 0]
        assert open_len == (step0 + T - new_open).tolist()
        open_start, step0 = new_open, step0 + T


def test_reference_returns_equal_np_sum_for_integer_rewards():
    """collect()'s return of an episode is np.sum over the carried reward pieces and the call's segment; for small
    integer rewards the reference's sequential sum is the same double."""
    rng = np.random.default_rng(5)
    T, N, S, calls = 9, 6, 40, 3
    R = rng.integers(-3, 4, (calls * T, N)).astype(np.float64)
    D = rng.random((calls * T, N)) < 0.2
    open_len, open_ret, got = [0] * N, [0.0] * N, []
    for c in range(calls):
        rows = slice(c * T, (c + 1) * T)
        done, r = _ring_of(S, N, (c * T) % S, D[rows], R[rows])
        ep, ret, _, open_len, open_ret = plan.plan_steps(done, r, (c * T) % S, T, S, open_len, open_ret, 1)
        got += [(e, L, g) for (e, _, L, _), g in zip(ep, ret)]
    want = []
    for c in range(calls):  # every episode that ends in call c, environment-major then time, summed by np.sum
        for e in range(N):
            for t in np.flatnonzero(D[c * T:(c + 1) * T, e]) + c * T:
                before = np.flatnonzero(D[:t, e])
                first = int(before[-1]) + 1 if len(before) else 0
                want.append((e, int(t) - first + 1, float(np.sum(R[first:t + 1, e]))))
    assert len(want) > 10 and any(L > T for _, L, _ in want)  # episodes that span calls are among them
    assert [(e, L) for e, L, _ in got] == [(e, L) for e, L, _ in want]
    assert np.array_equal(np.array([g for _, _, g in got]).view(np.uint64), np.array([g for _, _, g in want]).view(np.uint64))


class _Store:
    def add_steps(self, *a, **k):
        raise AssertionError("not reached")


class _HostEnv:
    n = 2

    def reset(self):
        return np.zeros((2, 4))

    def step(self, a):
        return np.zeros((2, 4)), np.ones(2), np.zeros(2, bool)


def test_device_plan_needs_a_device_environment():
    with pytest.raises(ValueError, match="step_device"):
        mx.DeviceVectorCollector(_HostEnv(), _Store(), 5, 0.99, device_plan=True)
    c = mx.DeviceVectorCollector(_HostEnv(), _Store(), 5, 0.99)
    assert c.device_plan is False


def test_fit_vector_device_plan_needs_device_collect():
    class DeviceEnv(_HostEnv):
        def step_device(self, *a):
            raise AssertionError("not reached")

    with pytest.raises(ValueError, match="device_plan"):
        mx.fit_vector(None, DeviceEnv(), None, buffer=_Store(), device_plan=True)
    with pytest.raises(ValueError, match="device_plan"):
        mx.fit_vector(None, _HostEnv(), None, buffer=_Store(), device_collect=True, device_plan=True)


def test_abi_declares_the_plan_entry():
    """(The entry and its block against the header: tests/test_abi_cpu.py, for the whole ABI.)"""
    assert "mzs_replay_plan_steps" in _lib.EXPORTED_SYMBOLS and _lib.STRUCTS["mzs_replay_plan_args"] is _lib.MzsReplayPlanArgs
    assert _lib.replay_plan_scratch(1) == 2 and _lib.replay_plan_scratch(256) == 257 and _lib.replay_plan_scratch(257) == 259
