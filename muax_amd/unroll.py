"""Forward value unroll of a sampled batch: v_i = value(s_i), s_0 = repr(obs[:, 0]), s_{i+1} = dynamics(s_i, a_i), and
the priorities |v_i - Rn_i| that `DeviceReplayBuffer.update_priorities` takes as [B, kp].

Two families, each described by one `Family` record that `MuZero.unroll_values` runs its route ladder over: `TRIO`, the
default MLP trio, and `STOCHASTIC`, the default stochastic MLP family of an `SMZNetwork`, whose unroll goes through the
afterstate dynamics and the chance dynamics on the encoder's code of every next observation.  Per family the HIP route,
one launch (muax_amd/csrc/mz_unroll.cuh) -- `FusedUnrollValues` / `StochasticFusedUnrollValues`, both on `_FusedUnroll`
-- and the same unroll on the model's torch modules, for the CPU and for any nets: `torch_unroll_values` /
`torch_stochastic_unroll_values`, both on `_torch_unroll`."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from functools import partial

import torch

from . import _call, _lib
from . import loss as mz_loss
from . import nn as mz_nn
from . import utils as mx_utils


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


def _every_observation(obs, B, L):
    mz_loss.check_every_observation(obs.shape, B, L, "unroll")
    return obs[:, :L].reshape(B, L, -1)


# ---- the torch route: the model's modules under no_grad.  Input preparation is per family (the trio casts to float32,
# the stochastic family evaluates in its modules' dtype); decoding the value and advancing the state is one loop ----
def _torch_unroll(pred, support_size, s, kp, advance, Rn, dtype):
    """(values, priorities), both [B, kp] of `dtype`: v_i decoded from the support logits of prediction(s_i) as in root
    inference, s_{i+1} = advance(s_i, i)."""
    values = []
    for i in range(kp):
        v_logits, _ = pred(s)
        values.append(mx_utils.support_to_scalar(torch.softmax(v_logits, dim=-1), support_size).reshape(len(s)))
        if i + 1 < kp:
            s = advance(s, i)
    values = torch.stack(values, dim=1).to(dtype)
    return values, (values - Rn[:, :kp]).abs()


def torch_unroll_values(model, batch, kp):
    """(values, priorities), both [B, kp] float32 on the model's device, from the model's modules under no_grad; the
    scalar value decoded from the support logits as in root inference.  No synchronisation."""
    dev = model.device
    with torch.no_grad():
        obs = torch.as_tensor(batch.obs, dtype=torch.float32, device=dev)
        a = torch.as_tensor(batch.a, device=dev)
        B, L = a.shape[:2]
        a = a.reshape(B, L)
        Rn = torch.as_tensor(batch.Rn, dtype=torch.float32, device=dev).reshape(B, L)
        return _torch_unroll(model.pred_func, model._support_size, model.repr_func(obs[:, 0]), kp,
                             lambda s, i: model.dy_func(s, a[:, i])[1], Rn, torch.float32)


def torch_stochastic_unroll_values(model, batch, kp, with_codes: bool = False):
    """`torch_unroll_values` for a model on an SMZNetwork: (values, priorities), both [B, kp], from the six modules under
    no_grad -- s_0 = repr(obs[:, 0]); after_i = afterstate_dynamic(s_i, a[:, i]); the code of obs[:, i + 1] is the
    encoder's argmax one-hot (`ChanceEncoder.code`; exact, not the loss's straight-through sum); s_{i+1} = the next state
    of chance_dynamic(after_i, code).  Evaluated in the modules' dtype and returned as float32 (float64 modules: float64).
    `with_codes`: also codes [B, kp] int32, -1 at step 0 and the code of transition i behind it.  No synchronisation."""
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
        codes = [torch.full((B,), -1, dtype=torch.int32, device=dev)]

        def advance(s, i):
            nxt = obs[:, i + 1]
            _, onehot, _ = enc.code(nxt) if hasattr(enc, "code") else mz_loss._straight_through(enc(nxt))
            codes.append(onehot.argmax(dim=-1).to(torch.int32))
            return chance_dy(after_dy(s, a[:, i]), onehot)[1]
        out = _torch_unroll(pred, model._support_size, rep(obs[:, 0]), kp, advance, Rn, out_dt)
        return out + (torch.stack(codes, dim=1),) if with_codes else out


# ---- the HIP route ----
class _FusedUnroll(_call.FusedCall):
    """The kernel route for one model, what its two families share: the weight struct is kept and rebuilt only when a
    parameter tensor moved (optimisers update in place: _call.MlpWeights, as in loss._FusedStep), the batch plumbing, the
    output and the keep-alive of what the launch reads.  A subclass states `_kernel`, `_weights_of`, `_names`,
    `_struct`, `_obs`, `__call__` and `_launch`; `family` is set below, where the records are."""

    def __init__(self, muzero_instance):
        if not self.family.is_family(muzero_instance.network):
            raise ValueError(f"the {self._kernel} kernel is built for {self.family.name}")
        super().__init__(muzero_instance, self._weights_of(muzero_instance.network), self._names, self._struct)
        shape = self.family.shape(muzero_instance)
        self.obs_dim, self.E, self.A = shape["obs_dim"], shape["embed_dim"], shape["num_actions"]
        self.C = shape.get("num_chance_outcomes")
        self._w = None

    def _unroll(self, batch, kp, codes):
        dev, t = self.dev, _call.as_device
        a = t(batch.a, torch.int32, dev)
        B, L = a.shape[:2]
        a = a.reshape(B, L)
        obs = self._obs(t(batch.obs, torch.float32, dev), B, L)
        Rn = t(batch.Rn, torch.float32, dev).reshape(B, L)
        if obs.shape[-1] != self.obs_dim:
            raise ValueError(f"batch.obs has {obs.shape[-1]} features, the network takes {self.obs_dim}")
        w, keep = self._weights.get()
        self._w = w  # (read by nobody here: the GPU tests check through it that the struct is kept)
        out = torch.empty((2, B, kp), dtype=torch.float32, device=dev)
        code = torch.empty((B, kp), dtype=torch.int32, device=dev) if codes else None
        self._launch(w, _call.device_index(dev), B, L, kp, obs, a, Rn, out, code)
        self._keep = (obs, a, Rn, keep)  # (alive until the next call: the launch is asynchronous)
        return (out[0], out[1], code) if codes else (out[0], out[1])


class FusedUnrollValues(_FusedUnroll):
    """The default MLP trio's unroll in one launch (mzs_mlp_unroll_values, mz_mlp_unroll_kernel in
    muax_amd/csrc/mz_unroll.cuh); the values have the bits of act()'s root value."""
    _kernel, _weights_of = "value-unroll", staticmethod(mz_nn.mlp_trio_weights)
    _names, _struct = _lib.MLP_WEIGHT_NAMES, _lib.MzsMlpWeights

    def _obs(self, obs, B, L):  # the first row of every window
        return obs[:, 0].reshape(B, -1).contiguous()

    def __call__(self, batch, kp):
        return self._unroll(batch, kp, False)

    def _launch(self, w, idx, B, L, kp, obs, a, Rn, out, code):
        w.obs_dim, w.support_size, w.discount = self.obs_dim, self.m._support_size, self.m._discount
        args = _lib.args(_lib.MzsUnrollArgs)  # (per call: fields by attribute, cheaper than keywords -- FusedLossGrad._launch)
        args.device, args.batch, args.row_steps, args.k_prio = idx, B, L, kp
        args.num_actions, args.embed_dim = self.A, self.E
        args.obs, args.actions, args.returns = obs.data_ptr(), a.data_ptr(), Rn.data_ptr()
        args.values, args.prio = out[0].data_ptr(), out[1].data_ptr()
        _lib.check(self._L.mzs_mlp_unroll_values(C.byref(w), C.byref(args), _call.raw_stream(idx)))


class StochasticFusedUnrollValues(_FusedUnroll):
    """`FusedUnrollValues` for the default stochastic MLP family (mzs_stochastic_mlp_unroll_values, mz_stoch_unroll_kernel in
    muax_amd/csrc/mz_unroll.cuh: one launch) on the 34-array weight struct.  Between two values lie the afterstate
    dynamics on the action and the chance dynamics on the code the encoder gives the NEXT observation, so every step's
    observation is read.  `codes=True` also returns the chance codes [B, kp] int32 (-1 at step 0)."""
    _kernel, _weights_of = "stochastic value-unroll", staticmethod(mz_nn.stochastic_train_weights)
    _names, _struct = _lib.STOCHASTIC_TRAIN_WEIGHT_NAMES, _lib.MzsStochasticTrainWeights

    def _obs(self, obs, B, L):  # a row for every step
        return _every_observation(obs, B, L).contiguous()

    def __call__(self, batch, kp, codes: bool = False):
        return self._unroll(batch, kp, codes)

    def _launch(self, w, idx, B, L, kp, obs, a, Rn, out, code):
        w.obs_dim, w.support_size = self.obs_dim, self.m._support_size
        args = _lib.args(_lib.MzsStochasticUnrollArgs, device=idx, batch=B, row_steps=L, k_prio=kp, num_actions=self.A,
                         num_chance_outcomes=self.C, embed_dim=self.E, obs=obs.data_ptr(), actions=a.data_ptr(),
                         returns=Rn.data_ptr(), values=out[0].data_ptr(), prio=out[1].data_ptr(),
                         codes=None if code is None else code.data_ptr())
        _lib.check(self._L.mzs_stochastic_mlp_unroll_values(C.byref(w), C.byref(args), _call.raw_stream(idx)))


# ---- each family, once, for MuZero.unroll_values' route ladder and the kernel wrappers above: its name in messages, the
# nn predicate, shape(model) -> what `limits` names, the limits the C entry states (include/mzsearch.h; outside them
# backend="auto" takes the torch route; "actions_and_outcomes" is A + C), the torch unroll and the kernel wrapper ----
Family = namedtuple("Family", "name is_family shape limits torch_unroll fused")


def _trio_shape(model) -> dict:
    r, p, _ = model.network
    return {"obs_dim": r.obs_dim or 0, "embed_dim": r.embedding_dim, "num_actions": p.num_actions,
            "support_size": model._support_size}


def _stochastic_shape(model) -> dict:
    r, p, _, ap, _, _ = model.network
    return {"obs_dim": r.obs_dim or 0, "embed_dim": r.embedding_dim, "num_actions": p.num_actions,
            "num_chance_outcomes": ap.num_actions, "actions_and_outcomes": p.num_actions + ap.num_actions,
            "support_size": model._support_size}


def within(family, model) -> bool:
    got = family.shape(model)
    return all(lo <= int(got[n]) <= hi for n, (lo, hi) in family.limits.items())


LIMITS = {"obs_dim": (1, 128), "embed_dim": (1, 64), "num_actions": (1, 64), "support_size": (8, 31)}
STOCHASTIC_LIMITS = {"obs_dim": (1, 128), "embed_dim": (1, 64), "num_actions": (1, 63), "num_chance_outcomes": (1, 63),
                     "actions_and_outcomes": (2, 64), "support_size": (8, 31)}
TRIO = Family("the default MLP trio", mz_nn.is_default_mlp_trio, _trio_shape, LIMITS, torch_unroll_values,
              FusedUnrollValues)
STOCHASTIC = Family("the default stochastic MLP family", mz_nn.is_default_stochastic_mlp, _stochastic_shape,
                    STOCHASTIC_LIMITS, torch_stochastic_unroll_values, StochasticFusedUnrollValues)
FusedUnrollValues.family, StochasticFusedUnrollValues.family = TRIO, STOCHASTIC
within_limits, within_stochastic_limits = partial(within, TRIO), partial(within, STOCHASTIC)
