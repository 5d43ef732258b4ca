"""Forward value unroll of a sampled batch: v_i = value(s_i), s_0 = repr(obs[:, 0]), s_{i+1} = dynamics(s_i, a_i), and
the priorities |v_i - Rn_i| that `DeviceReplayBuffer.update_priorities` takes as [B, kp].

`FusedUnrollValues` is the HIP route (mzs_mlp_unroll_values, muax_amd/csrc/mz_unroll.cuh: one launch for the default
MLP trio); `torch_unroll_values` the same unroll on the model's torch modules, for the CPU and for any nets.
`StochasticFusedUnrollValues` / `torch_stochastic_unroll_values` are their siblings for a model on an `SMZNetwork`, whose
unroll goes through the afterstate dynamics and the chance dynamics on the encoder's code of every next observation."""
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


# ---- the default stochastic MLP family (an SMZNetwork): between two values lie the afterstate dynamics on the action and
# the chance dynamics on the code the encoder gives the NEXT observation, so every step's observation is read ----
# what mzs_stochastic_mlp_unroll_values states (include/mzsearch.h); "actions_and_outcomes" is A + C
STOCHASTIC_LIMITS = {"obs_dim": (1, 128), "embed_dim": (1, 64), "num_actions": (1, 63), "num_chance_outcomes": (1, 63),
                     "actions_and_outcomes": (2, 64), "support_size": (8, 31)}


def _stochastic_shape(model) -> dict:
    r, p, _, ap, _, _ = model.network
    return {"obs_dim": r.obs_dim or 0, "embed_dim": r.embedding_dim, "num_actions": p.num_actions,
            "num_chance_outcomes": ap.num_actions, "actions_and_outcomes": p.num_actions + ap.num_actions,
            "support_size": model._support_size}


def within_stochastic_limits(model) -> bool:
    got = _stochastic_shape(model)
    return all(lo <= int(got[n]) <= hi for n, (lo, hi) in STOCHASTIC_LIMITS.items())


def check_every_observation(shape, B, L):
    """The loss's own refusal (loss.stochastic_loss_fn) for a batch whose obs is not [B, >= L, ...]."""
    if len(shape) < 3 or shape[0] != B or shape[1] < L:
        raise ValueError(f"the stochastic unroll needs every step's observation: batch.obs must be [B, L, ...] with L = {L} "
                         f"rows per window, got {tuple(shape)} (DeviceReplayBuffer.sample hands them out with all_obs=True)")


def _every_observation(obs, B, L):
    check_every_observation(tuple(obs.shape), B, L)
    return obs[:, :L].reshape(B, L, -1)


def torch_stochastic_unroll_values(model, batch, kp, with_codes: bool = False):
    """`torch_unroll_values` for a model on an SMZNetwork: (values, priorities), both [B, kp], from the six modules under
    no_grad -- s_0 = repr(obs[:, 0]); after_i = afterstate_dynamic(s_i, a[:, i]); the code of obs[:, i + 1] is the
    encoder's argmax one-hot (`ChanceEncoder.code`; exact, not the loss's straight-through sum); s_{i+1} = the next state
    of chance_dynamic(after_i, code).  Evaluated in the modules' dtype and returned as float32 (float64 modules: float64).
    `with_codes`: also codes [B, kp] int32, -1 at step 0 and the code of transition i behind it.  No synchronisation."""
    from . import loss as mz_loss
    from . import utils as mx_utils
    dev = model.device
    rep, pred, after_dy, _, chance_dy, enc = model.network
    fdt = next((p.dtype for n in model.network if isinstance(n, torch.nn.Module) for p in n.parameters()), torch.float32)
    with torch.no_grad():
        a = torch.as_tensor(batch.a, device=dev)
        B, L = a.shape[:2]
        a = a.reshape(B, L)
        obs = _every_observation(torch.as_tensor(batch.obs, device=dev).to(fdt), B, L)
        out_dt = torch.promote_types(fdt, torch.float32)
        Rn = torch.as_tensor(batch.Rn, device=dev).to(out_dt).reshape(B, L)
        s = rep(obs[:, 0])
        values, codes = [], [torch.full((B,), -1, dtype=torch.int32, device=dev)]
        for i in range(kp):
            v_logits, _ = pred(s)
            values.append(mx_utils.support_to_scalar(torch.softmax(v_logits, dim=-1), model._support_size).reshape(B))
            if i + 1 < kp:
                after = after_dy(s, a[:, i])
                nxt = obs[:, i + 1]
                _, onehot, _ = enc.code(nxt) if hasattr(enc, "code") else mz_loss._straight_through(enc(nxt))
                codes.append(onehot.argmax(dim=-1).to(torch.int32))
                _, s = chance_dy(after, onehot)
        values = torch.stack(values, dim=1).to(out_dt)
        out = values, (values - Rn[:, :kp]).abs()
        return out + (torch.stack(codes, dim=1),) if with_codes else out


class StochasticFusedUnrollValues:
    """`FusedUnrollValues` for the default stochastic MLP family (mzs_stochastic_mlp_unroll_values, mz_stoch_unroll_kernel in
    muax_amd/csrc/mz_unroll.cuh: one launch): the 34-array weight struct is kept and rebuilt only when a parameter tensor
    moved.  `codes=True` also returns the chance codes [B, kp] int32 (-1 at step 0)."""

    def __init__(self, muzero_instance):
        from . import nn as mz_nn
        if not mz_nn.is_default_stochastic_mlp(muzero_instance.network):
            raise ValueError("the stochastic value-unroll kernel is built for the default stochastic MLP family")
        self.m = muzero_instance
        params = mz_nn.stochastic_train_weights(muzero_instance.network)
        self.params = [params[n] for n in _lib.STOCHASTIC_TRAIN_WEIGHT_NAMES]
        self.dev = self.params[0].device
        if self.dev.type != "cuda":
            raise RuntimeError("muax_amd needs a ROCm GPU (gfx950); there is no CPU fallback")
        self._L = _lib.load()
        shape = _stochastic_shape(muzero_instance)
        self.obs_dim, self.E, self.A, self.C = (shape[n] for n in ("obs_dim", "embed_dim", "num_actions", "num_chance_outcomes"))
        self._weights = _call.MlpWeights(self.params, _lib.MzsStochasticTrainWeights, _lib.STOCHASTIC_TRAIN_WEIGHT_NAMES)
        self._w = None

    def __call__(self, batch, kp, codes: bool = False):
        dev = self.dev

        def t(x, dt):  # (tensors that already are what the kernel reads pass through untouched)
            if isinstance(x, torch.Tensor) and x.dtype == dt and x.device == dev and x.is_contiguous():
                return x
            return torch.as_tensor(x, device=dev).to(dt).contiguous()
        a = t(batch.a, torch.int32)
        B, L = a.shape[:2]
        a = a.reshape(B, L)
        obs = _every_observation(t(batch.obs, torch.float32), B, L).contiguous()
        Rn = t(batch.Rn, torch.float32).reshape(B, L)
        if obs.shape[2] != self.obs_dim:
            raise ValueError(f"batch.obs has {obs.shape[2]} features, the network takes {self.obs_dim}")
        w, keep = self._weights.get()
        self._w = w  # (read by nobody here: the tests check through it that the struct is kept)
        w.obs_dim, w.support_size = self.obs_dim, self.m._support_size
        out = torch.empty((2, B, kp), dtype=torch.float32, device=dev)
        code = torch.empty((B, kp), dtype=torch.int32, device=dev) if codes else None
        idx = _call.device_index(dev)
        args = _lib.args(_lib.MzsStochasticUnrollArgs, device=idx, batch=B, row_steps=L, k_prio=kp, num_actions=self.A,
                         num_chance_outcomes=self.C, embed_dim=self.E, obs=obs.data_ptr(), actions=a.data_ptr(),
                         returns=Rn.data_ptr(), values=out[0].data_ptr(), prio=out[1].data_ptr(),
                         codes=None if code is None else code.data_ptr())
        _lib.check(self._L.mzs_stochastic_mlp_unroll_values(C.byref(w), C.byref(args), _call.raw_stream(idx)))
        self._keep = (obs, a, Rn, keep)  # (alive until the next call: the launch is asynchronous)
        return (out[0], out[1], code) if codes else (out[0], out[1])
