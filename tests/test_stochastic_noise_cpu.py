"""CPU side of the root noise drawn inside the one-launch stochastic search (mzs_mlp_stochastic_search_draw,
MuZeroSearch.search_stochastic_mlp(draw_dirichlet=...), MuZero(stochastic_noise_in_kernel=True)): the device block's
host arithmetic against the existing block and muax_amd.prng, the binding's table, and the refusals that are decided
before a device is needed.  tests/test_gpu_stochastic_noise.py holds everything that launches."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

import muax_amd as mx
from muax_amd import _lib, prng
from muax_amd.search import MuZeroSearch

A, CN, E, OBS = 3, 4, 8, 5


def _words(entry, key, S, *floats, n):
    out = np.full(n + 5, 0xA5A5A5A5, np.uint32)  # (five guard words behind the block)
    kw = (C.c_uint32 * 2)(*key)
    assert entry(C.byref(kw), S, *floats, out.ctypes.data_as(C.c_void_p)) == 0
    assert (out[n:] == 0xA5A5A5A5).all()
    return out[:n]


def test_entries_are_declared():
    for name in ("mzs_mlp_stochastic_search_draw", "mzs_stochastic_search_block_draw"):
        assert name in _lib.ENTRIES and name in _lib.EXPORTED_SYMBOLS
        assert hasattr(_lib.load(), name)


@pytest.mark.parametrize("S", [1, 7, 255])
@pytest.mark.parametrize("key,temperature,fraction,alpha", [((4, 5), 1.0, 0.25, 0.3), ((0xFFFFFFFF, 0), 0.0, 1.0, 0.03),
                                                            ((0, 0), 0.5, 0.0, 2.5)])
def test_block_draw_is_the_block_plus_key_and_alpha(S, key, temperature, fraction, alpha):
    L = _lib.load()
    head = _words(L.mzs_stochastic_search_block, key, S, temperature, fraction, n=4 + 2 * S)
    got = _words(L.mzs_stochastic_search_block_draw, key, S, temperature, fraction, alpha, n=7 + 2 * S)
    assert np.array_equal(got[:4 + 2 * S], head)
    k_dir = prng.split(key, 3)[1]
    assert (int(got[4 + 2 * S]), int(got[5 + 2 * S])) == (int(k_dir[0]), int(k_dir[1]))
    assert int(got[6 + 2 * S]) == struct.unpack("<I", struct.pack("<f", alpha))[0]


def test_block_draw_refusals_and_null_key():
    L = _lib.load()
    out = np.zeros(9, np.uint32)
    p = out.ctypes.data_as(C.c_void_p)
    kw = (C.c_uint32 * 2)(1, 2)
    assert L.mzs_stochastic_search_block_draw(C.byref(kw), 0, 1.0, 0.25, 0.3, p) == -1
    assert L.mzs_stochastic_search_block_draw(C.byref(kw), 1, 1.0, 0.25, 0.3, None) == -1
    assert L.mzs_stochastic_search_block_draw(None, 1, 1.0, 0.25, 0.3, p) == 0  # a null key is the zero key
    assert np.array_equal(out, _words(L.mzs_stochastic_search_block_draw, (0, 0), 1, 1.0, 0.25, 0.3, n=9))


def test_search_refusals_that_need_no_device():
    """After the root-or-observations check and before the handle is looked at."""
    s = object.__new__(MuZeroSearch)
    z = torch.zeros
    root = (z(2, A), z(2), z(2, E))
    with pytest.raises(ValueError, match="either root_fn_output or obs"):
        MuZeroSearch.search_stochastic_mlp(s, one_launch=True, draw_dirichlet=0.3)
    with pytest.raises(ValueError, match="draw_dirichlet needs one_launch=True"):
        MuZeroSearch.search_stochastic_mlp(s, root, draw_dirichlet=0.3)
    with pytest.raises(ValueError, match="draw_dirichlet needs one_launch=True"):
        MuZeroSearch.search_stochastic_mlp(s, None, obs=z(2, OBS), draw_dirichlet=0.3)
    with pytest.raises(ValueError, match="draw_dirichlet and dirichlet_noise exclude each other"):
        MuZeroSearch.search_stochastic_mlp(s, root, one_launch=True, draw_dirichlet=0.3, dirichlet_noise=z(2, A))
    for alpha in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="alpha must be positive and finite"):
            MuZeroSearch.search_stochastic_mlp(s, root, one_launch=True, draw_dirichlet=alpha)
    with pytest.raises(ValueError, match="noise_out needs draw_dirichlet"):
        MuZeroSearch.search_stochastic_mlp(s, root, one_launch=True, noise_out=True)
    # the handle's own state is asked next, as without the option
    s._stochastic_weights = s._stochastic_repr = None
    with pytest.raises(ValueError, match="set_stochastic_mlp_weights"):
        MuZeroSearch.search_stochastic_mlp(s, root, one_launch=True, draw_dirichlet=0.3)


def test_model_flag_changes_nothing_on_the_cpu(monkeypatch):
    """Off by default; on the CPU the route is the callables and the noise act() draws itself is asked for as before
    (there it needs a GPU: the same error with and without the flag)."""
    def model(**kw):
        g = torch.Generator().manual_seed(0)
        m = mx.MuZero(mx.nn.create_stochastic_muzero_network(E, A, CN, 21, generator=g), device="cpu", **kw)
        m.init(0, np.zeros((1, OBS)))
        return m

    on = model(stochastic_one_launch=True, stochastic_root_in_kernel=True, stochastic_noise_in_kernel=True)
    off = model()
    assert on.stochastic_noise_in_kernel and not off.stochastic_noise_in_kernel
    obs = np.random.default_rng(1).uniform(-1, 1, (6, OBS)).astype(np.float32)
    for m in (on, off):
        with pytest.raises(RuntimeError, match="draws the root noise on the GPU"):
            m.act(7, obs, obs_from_batch=True)

    seen = []

    def call(self, params, rng_key, root, **kwargs):
        seen.append(kwargs["dirichlet_noise"])
        logits = root[0]
        return mx.search.PolicyOutput(logits.argmax(dim=1).to(torch.int32), torch.softmax(logits, dim=1), None)

    monkeypatch.setattr(mx.StochasticMuZeroPolicy, "__call__", call)
    noise = np.full((6, A), 1.0 / A, np.float32)
    for m in (on, off):
        m.act(7, obs, obs_from_batch=True, dirichlet_noise=noise)
        assert m._last_route == "callables" and seen.pop() is not None
        m.act(7, obs, obs_from_batch=True, dirichlet_fraction=0.0)
        assert m._last_route == "callables" and seen.pop() is None
