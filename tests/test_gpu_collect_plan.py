"""`DeviceVectorCollector(device_plan=True)` against the default route on `DeviceCartPole`, end to end: two collectors
on two equal environments, two equal-weight models and two fresh `DeviceReplayBuffer`s, the same keys.  The plan on the
device (mzs_replay_plan_steps) must hand out the `finished` lists the host's `ring_plan` and `np.sum` hand out, and
leave the same episodes in the buffer, bit for bit.

8 environments, max_episode_steps 12 (so episodes are truncated; a pole may also fall from step 8 on), a ring of 20
rows, three calls of 7 steps: the third wraps (rows 14..19, 0), episodes span calls, and with min_length 3 the staggered
starts (step counters set after the first reset, as tests/test_gpu_collect_env.py does) give dropped episodes of 1 and
2 steps beside stored ones.  A fourth call of 14 steps would outgrow the ring."""
import functools

import numpy as np
import pytest
import torch

import muax_amd as mx
from helpers import train_model

pytestmark = pytest.mark.gpu
N, MAX_STEPS, RING, STEPS, CALLS, SIMS, MIN_LENGTH, N_STEP, GAMMA, ALPHA = 8, 12, 20, 7, 3, 4, 3, 5, 0.997, 0.5
T0 = (0, 11, 10, 5, 0, 9, 3, 11)
SEED = 23


class StaggeredCartPole(mx.DeviceCartPole):
    """DeviceCartPole whose environments are T0 steps into their first episode."""

    def reset_device(self):
        obs = super().reset_device()
        self._t.copy_(torch.tensor(T0, dtype=torch.int32))
        return obs


class Downloads:
    """Counts the elements `Tensor.cpu()` brings down while it is active."""

    def __enter__(self):
        self.elements, self._cpu = [], torch.Tensor.cpu
        outer = self

        def cpu(t, *a, **k):
            if t.is_cuda:
                outer.elements.append(t.numel())
            return outer._cpu(t, *a, **k)
        torch.Tensor.cpu = cpu
        return self

    def __exit__(self, *exc):
        torch.Tensor.cpu = self._cpu


@functools.lru_cache(maxsize=None)
def _routes():
    out = {}
    for plan in (False, True):
        model = train_model(2, 8, 4, seed=3, support=10)
        buf = mx.DeviceReplayBuffer(32, 512, random_seed=0)
        env = StaggeredCartPole(N, max_episode_steps=MAX_STEPS, seed=SEED)
        col = mx.DeviceVectorCollector(env, buf, N_STEP, GAMMA, ALPHA, min_length=MIN_LENGTH, ring_steps=RING,
                                       device_plan=plan)
        key, fins, keys, down = mx.prng.PRNGKey(7), [], [], []
        for _ in range(CALLS):
            with Downloads() as d:
                fin, key, count = col.collect(model, key, STEPS, num_simulations=SIMS)
            assert count == STEPS * N
            fins.append(fin), keys.append(np.array(key)), down.append(d.elements)
        torch.cuda.synchronize()
        out[plan] = dict(model=model, buf=buf, col=col, fins=fins, keys=keys, key=key, down=down)
    return out


def _bits(x):
    return x.contiguous().view({4: torch.int32, 8: torch.int64, 1: torch.uint8}[x.element_size()])


def test_finished_lists_and_buffers_are_equal():
    R = _routes()
    a, b = R[False], R[True]
    every = [x for fin in a["fins"] for x in fin]
    stored = [x for x in every if x[2] is not None]
    assert len(stored) >= 8 and len(every) - len(stored) >= 2  # something stored, something dropped
    assert any(T > STEPS for T, _, _ in every)                 # episodes that span calls
    assert all(s is None for T, _, s in every if T < MIN_LENGTH) and [T for T, _, _ in every if T < MIN_LENGTH]
    assert a["fins"] == b["fins"]  # lengths, returns (== on floats: exact), serials, None for the dropped
    for fa, fb in zip(a["fins"], b["fins"]):
        assert [type(x) for row in fa for x in row] == [type(x) for row in fb for x in row]
    assert all(np.array_equal(x, y) for x, y in zip(a["keys"], b["keys"]))
    assert a["buf"].serials == b["buf"].serials == [s for _, _, s in stored]
    assert a["buf"].steps == b["buf"].steps
    for serial in a["buf"].serials:
        ea, eb = a["buf"].episode(serial), b["buf"].episode(serial)
        for name in ("obs", "a", "r", "done", "Rn", "v", "pi", "w"):
            assert torch.equal(_bits(getattr(ea, name)), _bits(getattr(eb, name))), (serial, name)
    for name in a["buf"]._t:  # and every arena and table as a whole
        assert torch.equal(_bits(a["buf"]._t[name]), _bits(b["buf"]._t[name])), name


def test_the_plan_route_downloads_only_the_counts_and_the_episode_rows():
    R = _routes()
    for fin, elements in zip(R[True]["fins"], R[True]["down"]):
        assert elements == [4] + ([4 * len(fin), len(fin)] if fin else [])
    assert all(sum(e) == 2 * STEPS * N for e in R[False]["down"])  # (the default route: the [T, N] rewards and flags)
    col = R[True]["col"]
    assert col._open_start is None and col._open_r is None  # no per-environment state on the host
    assert col._plan["ep"].shape == (N * STEPS, 4) and col._plan["ret"].shape == (N * STEPS,)


def test_a_call_that_would_outgrow_the_ring_is_refused_alike():
    R = _routes()
    msgs = []
    for plan in (False, True):
        col, before = R[plan]["col"], R[plan]["buf"].serials
        with pytest.raises(ValueError, match="does not fit the ring") as err:
            col.collect(R[plan]["model"], R[plan]["key"], RING - 6, num_simulations=SIMS)
        msgs.append(str(err.value))
        assert R[plan]["buf"].serials == before
    assert msgs[0] == msgs[1]
    held = int(msgs[0].split("open episode of ")[1].split(" steps")[0])
    assert held >= 7 and held + RING - 6 > RING


def _fit(plan):
    g = torch.Generator().manual_seed(0)
    net = mx.nn.MZNetwork(mx.nn.Representation(8, generator=g), mx.nn.Prediction(2, 21, generator=g),
                          mx.nn.Dynamic(8, 2, 21, generator=g))
    model = mx.MuZero(net, optimizer=mx.optimizers.create_optimizer("adam", 5e-3))
    buf, rows = mx.DeviceReplayBuffer(64, 4096, random_seed=13), []
    mx.fit_vector(model, mx.DeviceCartPole(8, max_episode_steps=6, seed=1), mx.DeviceCartPole(2, max_episode_steps=5, seed=2),
                  n_step=3, alpha=None, buffer=buf, iterations=2, steps_per_iteration=8, num_simulations=4, k_steps=3,
                  num_trajectory=8, sample_per_trajectory=2, num_update_per_iteration=3, test_interval=10, random_seed=3,
                  metrics=rows, device_collect=True, device_plan=plan)
    return rows, buf


def test_fit_vector_with_the_device_plan_equals_the_default():
    (rows_a, buf_a), (rows_b, buf_b) = _fit(False), _fit(True)
    assert len(rows_a) == len(rows_b) == 2 and [r["episodes"] for r in rows_b] == [8, 8]
    for ra, rb in zip(rows_a, rows_b):
        for k in ("episodes", "G", "loss", "training_step"):
            assert ra[k] == rb[k], k
    assert buf_a.serials == buf_b.serials and len(buf_b) == 16
