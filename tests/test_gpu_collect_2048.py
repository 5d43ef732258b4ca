"""Collection, greedy evaluation, reanalysis and one `fit_vector` iteration on `Device2048`, the device environment
with legal-move masks (muax_amd/envs.py).

Setup: 8 environments, max_episode_steps 16, 48 steps in calls of 20, 17 and 11, 5 simulations, into a
`DeviceReplayBuffer`.  `DeviceVectorCollector` -- with the plan on the host and on the device (`device_plan`) -- hands the
environment's own mask tensor to every act().  The yardstick is a hand loop on the plain-Python game
(tests/game2048_reference.py): `model.act(..., invalid_actions=<the reference's mask>)` on the reference's observations,
the reference stepped with the actions, its episodes cut by hand and flattened into `add_raw`.  The `finished` lists,
the serials and every stored field must be the same bits.  tests/test_env_2048_reference_cpu.py verifies without a GPU
that this seed meets states with an illegal move under a random legal policy; here the stored states are counted
again, so "no stored action is illegal" cannot pass vacuously."""
import functools

import numpy as np
import pytest
import torch

import game2048_reference as g
import muax_amd as mx
from helpers import train_model

pytestmark = pytest.mark.gpu
N, MAX_STEPS, CALLS, SIMS, N_STEP, GAMMA, ALPHA, MIN_LENGTH = 8, 16, (20, 17, 11), 5, 3, 0.997, 0.5, 1
SEED, SHIFT = 23, 2


def _model():
    return train_model(g.NUM_ACTIONS, 8, g.OBS_DIM, seed=3, support=10)


def _bits(x):
    return x.view({4: torch.int32, 8: torch.int64, 1: torch.uint8}[x.element_size()])


def _hand_loop():
    """The reference stepped by hand with act(invalid_actions=its mask).  Per call: the finished episodes as (T, G) in
    the collector's order (environment-major, then time) and their flat add_raw stream; the keys after every call."""
    model, buf = _model(), mx.DeviceReplayBuffer(64, 1024, random_seed=0)
    env = g.Vector2048(N, MAX_STEPS, seed=SEED, reward_shift=SHIFT)
    key, obs = mx.prng.PRNGKey(7), env.reset()
    open_eps = [[] for _ in range(N)]  # per environment: the steps (obs, a, r, v, pi) of its open episode
    fins, keys, masks = [], [], []
    for steps in CALLS:
        ended = [[] for _ in range(N)]
        for _ in range(steps):
            key, subkey = mx.prng.split(key)
            mask = env.invalid_actions()
            a, pi, v = model.act(subkey, obs, with_pi=True, with_value=True, obs_from_batch=True, num_simulations=SIMS,
                                 temperature=1.0, invalid_actions=mask)
            nxt, r, done = env.step(a)
            masks.append(mask)
            for e in range(N):
                open_eps[e].append((obs[e], int(a[e]), float(r[e]), float(v[e]), np.asarray(pi[e]).reshape(-1)))
                if done[e]:
                    ended[e].append(open_eps[e])
                    open_eps[e] = []
            obs = nxt
        episodes = [ep for e in range(N) for ep in ended[e]]
        if episodes:
            flat = [x for ep in episodes for x in ep]
            buf.add_raw(np.array([x[0] for x in flat], np.float32), np.array([x[1] for x in flat]),
                        np.array([x[2] for x in flat]), np.array([x[3] for x in flat]),
                        np.array([x[4] for x in flat], np.float32), [len(ep) for ep in episodes], N_STEP, GAMMA, ALPHA,
                        weight="mean")
        fins.append([(len(ep), float(np.sum([x[2] for x in ep]))) for ep in episodes])
        keys.append(np.array(key))
    return dict(buf=buf, fins=fins, keys=keys, masks=np.stack(masks), env=env)


@functools.lru_cache(maxsize=None)
def _routes():
    out = {}
    for route in ("host_plan", "device_plan"):
        model, buf = _model(), mx.DeviceReplayBuffer(64, 1024, random_seed=0)
        venv = mx.Device2048(N, max_episode_steps=MAX_STEPS, seed=SEED, reward_shift=SHIFT)
        col = mx.DeviceVectorCollector(venv, buf, N_STEP, GAMMA, ALPHA, min_length=MIN_LENGTH,
                                       device_plan=route == "device_plan")
        key, fins, keys = mx.prng.PRNGKey(7), [], []
        for steps in CALLS:
            fin, key, count = col.collect(model, key, steps, num_simulations=SIMS)
            assert count == steps * N
            fins.append(fin), keys.append(np.array(key))
        out[route] = dict(buf=buf, fins=fins, keys=keys, col=col, model=model)
    out["hand"] = _hand_loop()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("route", ["host_plan", "device_plan"])
def test_collection_equals_the_hand_loop_on_the_reference(route):
    R = _routes()
    dev, hand = R[route], R["hand"]
    assert all(np.array_equal(x, y) for x, y in zip(dev["keys"], hand["keys"]))
    for fin, want in zip(dev["fins"], hand["fins"]):  # the same episodes in the same order, call by call
        assert [(T, G) for T, G, _ in fin] == want
    every = [x for fin in dev["fins"] for x in fin]
    assert len(every) == N * (sum(CALLS) // MAX_STEPS) and any(G > 0 for _, G, _ in every)
    bd, bh = dev["buf"], hand["buf"]
    assert bd.serials == bh.serials == [s for _, _, s in every] and bd.steps == bh.steps == sum(T for T, _, _ in every)
    for s in bd.serials:  # the stored bits, episode by episode
        ed, eh = bd.episode(s), bh.episode(s)
        assert tuple(ed.obs.shape[1:]) == (g.OBS_DIM,) and ed.pi.shape[-1] == g.NUM_ACTIONS
        for k in ("obs", "a", "r", "Rn", "v", "done", "pi", "w"):
            gx, gy = getattr(ed, k), getattr(eh, k)
            assert gx.dtype == gy.dtype and gx.shape == gy.shape and torch.equal(_bits(gx), _bits(gy)), (route, s, k)
    # the environment ended where the reference did
    venv, ref = dev["col"].venv, hand["env"]
    assert np.array_equal(venv._board.cpu().numpy().view(np.uint64), ref.boards())
    assert venv._draws.cpu().tolist() == ref.draws and venv._t.cpu().tolist() == ref.t
    assert np.array_equal(venv.invalid_actions(), ref.invalid_actions())


def test_device_plan_off_and_on_leave_the_same_bits():
    R = _routes()
    a, b = R["host_plan"], R["device_plan"]
    assert a["fins"] == b["fins"]
    ba, bb = a["buf"], b["buf"]
    assert set(ba._t) == set(bb._t)
    for n in ba._t:
        assert torch.equal(_bits(ba._t[n]), _bits(bb._t[n])), n
    for k in ("obs", "a", "r", "v", "pi"):
        assert torch.equal(_bits(a["col"]._fields[k]), _bits(b["col"]._fields[k])), k


def _illegal_of(obs):
    """[T, 4] bool: the reference's mask of every stored observation."""
    return np.array([g.mask(g.grid_of_obs(row)) for row in obs.cpu().numpy()], bool)


@pytest.mark.parametrize("route", ["host_plan", "device_plan"])
def test_no_stored_action_is_illegal_in_its_stored_observation(route):
    R = _routes()
    buf = R[route]["buf"]
    with_illegal = rows = 0
    for s in buf.serials:
        ep = buf.episode(s)
        illegal = _illegal_of(ep.obs)
        a = ep.a.cpu().numpy().reshape(-1).astype(int)
        assert ((a >= 0) & (a < 4)).all() and not illegal[np.arange(len(a)), a].any(), s
        pi = ep.pi.cpu().numpy().reshape(len(a), -1)
        assert (pi[illegal] == 0).all(), s  # nor does a search policy put weight there
        with_illegal, rows = with_illegal + int(illegal.any(1).sum()), rows + len(a)
    assert rows == sum(CALLS) * N and with_illegal >= N  # the check is not vacuous
    assert R["hand"]["masks"].any(2).sum() >= with_illegal  # (the hand loop saw the open episodes' states as well)


@pytest.mark.parametrize("max_episode_steps,max_steps", [(9, None), (20, None), (20, 5)])
def test_vector_device_equals_test_vector(max_episode_steps, max_steps):
    model = train_model(g.NUM_ACTIONS, 8, g.OBS_DIM, seed=5, support=10)
    key = mx.prng.PRNGKey(11)
    make = lambda: mx.Device2048(6, max_episode_steps=max_episode_steps, seed=4, reward_shift=SHIFT)  # noqa: E731
    want = mx.test_vector(model, make(), key, SIMS, max_steps=max_steps)
    got = mx.test_vector_device(model, make(), key, SIMS, max_steps=max_steps)
    assert got == want and np.isfinite(want) and want >= 0.0
    # and the greedy actions were legal: the same loop by hand on the reference gives the same return only if no move
    # was a no-op the reference would also have taken -- so count them
    ref = g.Vector2048(6, max_episode_steps, seed=4, reward_shift=SHIFT)
    obs, G, live, k = ref.reset(), np.zeros(6), np.ones(6, bool), key
    for _ in range(max_steps or max_episode_steps):
        k, sub = mx.prng.split(k)
        mask = ref.invalid_actions()
        a = model.act(sub, obs, obs_from_batch=True, num_simulations=SIMS, temperature=0., invalid_actions=mask)
        assert not mask[np.arange(6), np.asarray(a)].any()
        obs, r, done = ref.step(a)
        G += np.where(live, r, 0.0)
        live &= ~done
        if not live.any():
            break
    assert float(G.mean()) == want


def test_reanalyse_with_mask_fn_leaves_no_weight_on_illegal_moves():
    """chunk_rows 80: five chunks, the last one zero-padded (all-zero rows: mask 0, they must not stop the search)."""
    R = _routes()
    src = R["hand"]["buf"]
    model = R["host_plan"]["model"]
    venv = mx.Device2048(1, seed=0)
    masked, plain = (mx.DeviceReplayBuffer(64, 1024, random_seed=0) for _ in range(2))
    for buf in (masked, plain):  # two copies of the collected episodes
        eps = [src.episode(s) for s in src.serials]
        cat = lambda k: torch.cat([getattr(e, k) for e in eps])  # noqa: E731
        buf.add_raw(cat("obs"), cat("a"), cat("r").double(), cat("v").double(), cat("pi").reshape(-1, 4),
                    [int(e.a.shape[0]) for e in eps], N_STEP, GAMMA, ALPHA)
    calls = []

    def mask_fn(chunk):
        calls.append(tuple(chunk.shape))
        return venv.invalid_actions_of(chunk)

    key = mx.prng.PRNGKey(5)
    rows = masked.reanalyse(model, key, N_STEP, GAMMA, ALPHA, chunk_rows=80, mask_fn=mask_fn, num_simulations=SIMS)
    assert rows == plain.reanalyse(model, key, N_STEP, GAMMA, ALPHA, chunk_rows=80, num_simulations=SIMS) == src.steps
    assert calls == [(80, 16)] * -(-rows // 80) and rows % 80 != 0
    on_illegal = [0.0, 0.0]
    changed = False
    for s in masked.serials:
        illegal = _illegal_of(masked.episode(s).obs)
        for i, buf in enumerate((masked, plain)):
            pi = buf.episode(s).pi.cpu().numpy().reshape(illegal.shape[0], -1)
            assert np.isfinite(pi).all() and np.allclose(pi.sum(1), 1.0, atol=1e-5)
            on_illegal[i] += float(pi[illegal].sum())
        changed |= not torch.equal(masked.episode(s).pi, src.episode(s).pi)
    assert on_illegal[0] == 0.0 and changed
    assert on_illegal[1] > 0.0  # without mask_fn the search does put weight on illegal moves: what mask_fn is for


def test_reanalyse_without_mask_fn_on_cartpole_is_unchanged():
    """`mask_fn` None takes the path it always took: the same call twice with the same key leaves the same bits, and
    the collector asked a CartPole for no mask."""
    model = train_model(2, 8, 4, seed=3, support=10)
    buf = mx.DeviceReplayBuffer(32, 512, random_seed=0)
    venv = mx.DeviceCartPole(5, max_episode_steps=7, seed=2)
    assert not hasattr(venv, "invalid_actions_device") and not hasattr(venv, "invalid_actions_of")
    col = mx.DeviceVectorCollector(venv, buf, N_STEP, GAMMA, ALPHA)
    col.collect(model, mx.prng.PRNGKey(1), 20, num_simulations=SIMS)
    assert len(buf) >= 5
    key, snaps = mx.prng.PRNGKey(9), []
    for _ in range(2):
        assert buf.reanalyse(model, key, N_STEP, GAMMA, ALPHA, chunk_rows=64, num_simulations=SIMS) == buf.steps
        snaps.append({n: _bits(t).clone() for n, t in buf._t.items()})
    assert all(torch.equal(snaps[0][n], snaps[1][n]) for n in snaps[0])


def test_one_fit_vector_iteration_end_to_end():
    torch_g = torch.Generator().manual_seed(0)
    net = mx.nn.MZNetwork(mx.nn.Representation(8, generator=torch_g), mx.nn.Prediction(4, 21, generator=torch_g),
                          mx.nn.Dynamic(8, 4, 21, generator=torch_g))
    model = mx.MuZero(net, optimizer=mx.optimizers.create_optimizer("adam", 5e-3))
    buf, rows = mx.DeviceReplayBuffer(64, 4096, random_seed=13), []

    class Counting(mx.Device2048):
        host_steps = mask_calls = 0

        def step(self, actions):
            Counting.host_steps += 1
            return super().step(actions)

        def invalid_actions_of(self, obs):
            Counting.mask_calls += 1
            return super().invalid_actions_of(obs)

    mx.fit_vector(model, Counting(8, max_episode_steps=6, seed=1, reward_shift=SHIFT),
                  Counting(2, max_episode_steps=5, seed=2, reward_shift=SHIFT),
                  n_step=3, alpha=None, buffer=buf, iterations=1, steps_per_iteration=6, num_simulations=4, k_steps=3,
                  num_trajectory=8, sample_per_trajectory=2, num_update_per_iteration=2, test_interval=10,
                  random_seed=3, metrics=rows, device_collect=True, device_plan=True, reanalyse_every=1)
    assert len(rows) == 1 and rows[0]["episodes"] == 8 and np.isfinite(rows[0]["G"]) and rows[0]["G"] >= 0.0
    assert np.isfinite(rows[0]["test_G"]) and np.isfinite(rows[0]["loss"])
    assert Counting.host_steps == 0 and Counting.mask_calls == 1
    for s in buf.serials:  # the reanalysed policies respect the masks
        ep = buf.episode(s)
        illegal = _illegal_of(ep.obs)
        assert (ep.pi.cpu().numpy().reshape(illegal.shape[0], -1)[illegal] == 0).all()
