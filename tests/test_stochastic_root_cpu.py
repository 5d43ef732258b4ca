"""CPU side of the library's own root inference for the default stochastic MLP family (MuZero(stochastic_root_in_kernel=
True), nn.stochastic_root_weights, MuZeroSearch.search_stochastic_mlp(None, obs=...)): without a GPU the flag changes
nothing -- the torch root, the callables route, the same arrays --, the weight accessor returns the representation's two
arrays, and the argument errors that need no device are raised.  The policy's search itself needs a device: its
`__call__` is replaced by a function of the root it is handed, so that a different root would show in the outputs."""
import numpy as np
import pytest
import torch

import muax_amd as mx
from muax_amd.search import MuZeroSearch, PolicyOutput

F32 = np.float32
A, CN, E, OBS = 3, 4, 8, 5


def _model(**kw):
    g = torch.Generator().manual_seed(0)
    m = mx.MuZero(mx.nn.create_stochastic_muzero_network(E, A, CN, 21, generator=g), device="cpu", **kw)
    m.init(0, np.zeros((1, OBS)))
    return m


@pytest.fixture
def roots(monkeypatch):
    """StochasticMuZeroPolicy.__call__ as a function of the RootFnOutput it receives; the roots it saw."""
    seen = []

    def call(self, params, rng_key, root, **kwargs):
        logits, value, emb = root
        seen.append((logits.clone(), value.clone(), emb.clone()))
        return PolicyOutput(logits.argmax(dim=1).to(torch.int32), torch.softmax(logits + value[:, None], dim=1), None)

    monkeypatch.setattr(mx.StochasticMuZeroPolicy, "__call__", call)
    return seen


def test_flag_changes_nothing_on_the_cpu(roots):
    on, off = _model(stochastic_root_in_kernel=True, stochastic_one_launch=True), _model()
    assert on.stochastic_root_in_kernel and not off.stochastic_root_in_kernel
    obs = np.random.default_rng(1).uniform(-1, 1, (6, OBS)).astype(F32)
    kw = dict(with_pi=True, with_value=True, obs_from_batch=True, dirichlet_fraction=0.0)  # (the noise is drawn on a GPU)
    got = on.act(7, obs, **kw)
    assert on._last_route == "callables"
    ref = off.act(7, obs, **kw)
    assert off._last_route == "callables"
    for g, r in zip(got, ref):
        assert g.dtype == r.dtype and np.array_equal(g.view(np.uint32), r.view(np.uint32))
    # both searched the torch root of the observations
    assert len(roots) == 2
    for a, b in zip(*roots):
        assert torch.equal(a, b)
    with torch.no_grad():
        s = off.repr_func(torch.from_numpy(obs))
    assert torch.equal(roots[0][2], s)


def test_stochastic_root_weights():
    m = _model()
    w, b = mx.nn.stochastic_root_weights(m.network)
    assert tuple(w.shape) == (OBS, E) and tuple(b.shape) == (E,)
    assert w is m.repr_func.repr_func.w and b is m.repr_func.repr_func.b
    # the arrays are the ones the training step's accessor lists first
    tw = mx.nn.stochastic_train_weights(m.network)
    assert tw["repr_w"] is w and tw["repr_b"] is b
    g = torch.Generator().manual_seed(0)
    with pytest.raises(ValueError, match="no weights yet"):
        mx.nn.stochastic_root_weights(mx.nn.create_stochastic_muzero_network(E, A, CN, 21, generator=g))


def test_search_stochastic_mlp_takes_a_root_or_observations():
    """Both or neither: refused before the handle is looked at (no device needed)."""
    s = object.__new__(MuZeroSearch)
    z = torch.zeros
    with pytest.raises(ValueError, match="either root_fn_output or obs"):
        MuZeroSearch.search_stochastic_mlp(s)
    with pytest.raises(ValueError, match="either root_fn_output or obs"):
        MuZeroSearch.search_stochastic_mlp(s, (z(2, A), z(2), z(2, E)), obs=z(2, OBS))
    with pytest.raises(ValueError, match="either root_fn_output or obs"):
        MuZeroSearch.search_stochastic_mlp(s, None, one_launch=True)
    # the handle's own state is asked next: weights, then the representation
    s._stochastic_weights = s._stochastic_repr = None
    with pytest.raises(ValueError, match="set_stochastic_mlp_weights"):
        MuZeroSearch.search_stochastic_mlp(s, None, obs=z(2, OBS))
    s._stochastic_weights = {}
    for one_launch in (False, True):
        with pytest.raises(ValueError, match="set_stochastic_representation"):
            MuZeroSearch.search_stochastic_mlp(s, None, obs=z(2, OBS), one_launch=one_launch)
