"""Forward value unroll of a sampled batch: v_i = value(s_i), s_0 = repr(obs[:, 0]), s_{i+1} = dynamics(s_i, a_i), and
the priorities |v_i - Rn_i| that `DeviceReplayBuffer.update_priorities` takes as [B, kp].

`FusedUnrollValues` is the HIP route (mzs_mlp_unroll_values, muax_amd/csrc/mz_unroll.cuh: one launch for the default
MLP trio); `torch_unroll_values` the same unroll on the model's torch modules, for the CPU and for any nets."""
from __future__ import annotations

import ctypes as C

import torch

from . import _call, _lib

# what mzs_mlp_unroll_values states (include/mzsearch.h): outside them backend="auto" takes the torch route
LIMITS = {"obs_dim": (1, 128), "embed_dim": (1, 64), "num_actions": (1, 64), "support_size": (8, 31)}


def batch_window(batch, k_prio):
    """(B, L, kp) of a batch whose `a` is [B, L, ...]; kp defaults to L and must be in 1..L."""
    shape = tuple(batch.a.shape)
    if len(shape) < 2:
        raise ValueError(f"batch.a must be [B, L, ...], got {shape}")
    B, L = int(shape[0]), int(shape[1])
    kp = L if k_prio is None else int(k_prio)
    if kp < 1 or kp > L:
        raise ValueError(f"k_prio must be in 1..{L} (the window length), got {kp}")
    return B, L, kp


def within_limits(model) -> bool:
    r, p, _ = model.network
    got = {"obs_dim": r.obs_dim or 0, "embed_dim": r.embedding_dim, "num_actions": p.num_actions,
           "support_size": model._support_size}
    return all(lo <= int(got[n]) <= hi for n, (lo, hi) in LIMITS.items())


def torch_unroll_values(model, batch, kp):
    """(values, priorities), both [B, kp] float32 on the model's device, from the model's modules under no_grad; the
    scalar value decoded from the support logits as in root inference.  No synchronisation."""
    from . import utils as mx_utils
    dev = model.device
    with torch.no_grad():
        obs = torch.as_tensor(batch.obs, dtype=torch.float32, device=dev)
        a = torch.as_tensor(batch.a, device=dev)
        B, L = a.shape[:2]
        a = a.reshape(B, L)
        Rn = torch.as_tensor(batch.Rn, dtype=torch.float32, device=dev).reshape(B, L)
        s = model.repr_func(obs[:, 0])
        values = []
        for i in range(kp):
            v_logits, _ = model.pred_func(s)
            values.append(mx_utils.support_to_scalar(torch.softmax(v_logits, dim=-1), model._support_size).reshape(B))
            if i + 1 < kp:
                _, s = model.dy_func(s, a[:, i])
        values = torch.stack(values, dim=1).to(torch.float32)
        return values, (values - Rn[:, :kp]).abs()


class FusedUnrollValues:
    """The kernel route for one model: the weight struct is kept and rebuilt only when a parameter tensor moved
    (optimisers update in place): _call.MlpWeights, as in FusedLossGrad."""

    def __init__(self, muzero_instance):
        from . import nn as mz_nn
        if not mz_nn.is_default_mlp_trio(muzero_instance.network):
            raise ValueError("the value-unroll kernel is built for the default MLP trio")
        self.m = muzero_instance
        params = mz_nn.mlp_trio_weights(muzero_instance.network)
        self.params = [params[n] for n in _lib.MLP_WEIGHT_NAMES]
        self.dev = self.params[0].device
        if self.dev.type != "cuda":
            raise RuntimeError("muax_amd needs a ROCm GPU (gfx950); there is no CPU fallback")
        self._L = _lib.load()
        r, p, _ = muzero_instance.network
        self.obs_dim, self.E, self.A = r.obs_dim, r.embedding_dim, p.num_actions
        self._weights, self._w = _call.MlpWeights(self.params), None

    def __call__(self, batch, kp):
        dev = self.dev

        def t(x, dt):  # (tensors that already are what the kernel reads pass through untouched)
            if isinstance(x, torch.Tensor) and x.dtype == dt and x.device == dev and x.is_contiguous():
                return x
            return torch.as_tensor(x, device=dev).to(dt).contiguous()
        a = t(batch.a, torch.int32)
        B, L = a.shape[:2]
        a = a.reshape(B, L)
        obs = t(batch.obs, torch.float32)[:, 0].reshape(B, -1).contiguous()
        Rn = t(batch.Rn, torch.float32).reshape(B, L)
        if obs.shape[1] != self.obs_dim:
            raise ValueError(f"batch.obs has {obs.shape[1]} features, the network takes {self.obs_dim}")
        w, keep = self._weights.get()
        self._w = w  # (read by nobody here: tests/test_gpu_unroll_values.py checks through it that the struct is kept)
        w.obs_dim, w.support_size, w.discount = self.obs_dim, self.m._support_size, self.m._discount
        out = torch.empty((2, B, kp), dtype=torch.float32, device=dev)
        idx = _call.device_index(dev)
        args = _lib.args(_lib.MzsUnrollArgs)
        args.device, args.batch, args.row_steps, args.k_prio = idx, B, L, kp
        args.num_actions, args.embed_dim = self.A, self.E
        args.obs, args.actions, args.returns = obs.data_ptr(), a.data_ptr(), Rn.data_ptr()
        args.values, args.prio = out[0].data_ptr(), out[1].data_ptr()
        _lib.check(self._L.mzs_mlp_unroll_values(C.byref(w), C.byref(args), _call.raw_stream(idx)))
        self._keep = (obs, a, Rn, keep)  # (alive until the next call: the launch is asynchronous)
        return out[0], out[1]
