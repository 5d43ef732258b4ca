"""k-step unrolled MuZero loss of the reference (muax/loss.py:10-88): SURVEY.md 8(f) n1.

Two routes to the same number.  `default_loss_fn` is the formula in plain PyTorch ops (autograd does the backward
pass): it serves plugin nets and custom losses, and it is the reference the fused kernel is tested against.
`FusedLossGrad` (below) is the product path for the default MLP trio: loss and every gradient from ONE hand-written
forward+backward HIP kernel (muax_amd/csrc/mz_train.cuh through mzs_mlp_loss_grad; its blocks, shared with the
stochastic family's kernel, in mz_train_blocks.cuh).  The reference's formula:

    loss = sum_{i<L} [ mean_B CE(r_logits_i, support(r_i)) + mean_B CE(v_logits_i, support(Rn_i))
                       + mean_B CE(pi_logits_i, pi_i) ]  +  1e-4 * 0.5 * sum ||param||^2

with the hidden state's gradient halved at the start of every dynamics step (Appendix G,
muax/loss.py:60-61).  Reference quirks handled explicitly:
  * muax/loss.py:83 reads `loss` before assignment; the only consistent reading is an initial 0;
  * the coax variant divides by L (muax/frameworks/coax/loss.py:70-71): `divide_by_length=True`;
  * muax stores pi per step as [1, A] (muax/model.py:176), so batch.pi[:, i] is [B, 1, A] against logits
    [B, A] and optax broadcasts to an all-pairs [B, B] cross entropy.  Here pi is squeezed to [B, L, A]
    (the intended per-sample target); `pi_all_pairs=True` reproduces the broadcast.

Beyond the reference: `sample_weight` [B], the importance-sampling weights of prioritised replay
(`DeviceReplayBuffer.sample(is_beta=)`), turns every mean_B CE(...) into mean_B (sample_weight * CE(...)) on both
routes; the L2 term is not weighted.  Its [B] check (`check_sample_weight`) and the refusal of a batch without an
observation for every step (`check_every_observation`) are stated once here, for update(), both fused steps and unroll.py.

`stochastic_loss_fn` is the Stochastic MuZero loss of the reference's acme agent
(muax/frameworks/acme/jax/stochastic_muzero/learning.py:200-277) in the conventions above -- a sum over steps, support
targets by scalar_to_support, the same L2 term over all six modules, the halved hidden-state gradient before each
afterstate step -- on torch autograd; `StochasticFusedLossGrad` (below) is the same loss and its gradients from one HIP
kernel for the default stochastic MLP family.  Its reference quirks:
  * learning.py:262 measures the VQ commitment against the straight-through code, whose value is the one-hot but whose
    gradient is the encoder output's own: the term's gradient is identically zero.  Here the encoder output commits to
    the DETACHED one-hot, which is what a commitment term is for;
  * learning.py:230-231 hands the chance network argmax(code), an integer: the straight-through estimator it has just
    built never carries a gradient.  Here the chance dynamics take the straight-through code itself as their one-hot
    input, so the encoder learns from the losses downstream of the outcome;
  * learning.py:273 divides by the unroll length; here that is `divide_by_length=True`, as in default_loss_fn.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _call, _lib
from . import utils as mx_utils
from .episode_tracer import Transition  # noqa: F401  (muax.episode_tracer.Transition)


def softmax_cross_entropy(logits, labels):
    """optax.softmax_cross_entropy: -sum(labels * log_softmax(logits), -1)."""
    return -(labels * torch.log_softmax(logits, dim=-1)).sum(dim=-1)


def check_every_observation(shape, B, L, what="loss"):
    """The refusal of a batch whose obs (`shape`) is not [B, >= L, ...], by whoever reads an observation for every step
    of a window: the stochastic `what` -- "loss" (both routes) or "unroll" (unroll.py)."""
    if len(shape) < 3 or shape[0] != B or shape[1] < L:
        raise ValueError(f"the stochastic {what} needs every step's observation: batch.obs must be [B, L, ...] with L = {L} "
                         f"rows per window, got {tuple(shape)} (DeviceReplayBuffer.sample hands them out with all_obs=True)")


def check_sample_weight(sample_weight, B):
    """`sample_weight` must be [B]: update() and the fused steps ask before any launch, the two loss functions of the tensor
    they converted.  The shape alone: looking at the values would synchronise."""
    if tuple(getattr(sample_weight, "shape", ())) != (B,):
        raise ValueError(f"sample_weight must be [B] with B = {B}, got {tuple(getattr(sample_weight, 'shape', ()))}")


def default_loss_fn(muzero_instance, batch: Transition, divide_by_length: bool = False,
                    pi_all_pairs: bool = False, sample_weight=None):
    """muax/loss.py:10-88.  `batch` fields are tensors/arrays of shape [B, L, ...].  `sample_weight` [B]: row b's three
    cross entropies count sample_weight[b] times at every step (no gradient flows into the weights)."""
    dev = muzero_instance.device
    if sample_weight is not None and pi_all_pairs:
        raise ValueError("sample_weight cannot be combined with pi_all_pairs: a [B, B] cross entropy has no per-row weight")
    # the nets' own floating-point type: float32 in the product, float64 where a test evaluates the formula so
    fdt = next((p.dtype for m in muzero_instance.network if isinstance(m, torch.nn.Module) for p in m.parameters()),
               torch.float32)
    t = lambda x, dt=fdt: torch.as_tensor(x, dtype=dt, device=dev)  # noqa: E731
    a = t(batch.a, torch.long)
    B, L = a.shape[:2]
    a = a.reshape(B, L)
    S = muzero_instance._support_size
    r_t = mx_utils.scalar_to_support(t(batch.r).reshape(B, L), S).detach()
    Rn_t = mx_utils.scalar_to_support(t(batch.Rn).reshape(B, L), S).detach()
    pi = t(batch.pi)
    pi = pi.reshape(B, L, 1, -1) if pi_all_pairs else pi.reshape(B, L, -1)
    obs = t(batch.obs)
    s = muzero_instance.repr_func(obs[:, 0])
    loss = torch.zeros((), dtype=fdt, device=dev)
    sw = None
    if sample_weight is not None:
        sw = torch.as_tensor(sample_weight, device=dev).detach().to(s.dtype)
        check_sample_weight(sw, B)
    for i in range(L):
        v, logits = muzero_instance.pred_func(s)
        s = mx_utils.scale_gradient(s, 0.5)  # Appendix G
        r, ns = muzero_instance.dy_func(s, a[:, i])
        ce_r, ce_v = softmax_cross_entropy(r, r_t[:, i]), softmax_cross_entropy(v, Rn_t[:, i])
        ce_p = softmax_cross_entropy(logits, pi[:, i].detach())
        if sw is None:
            loss = loss + ce_r.mean() + ce_v.mean() + ce_p.mean()
        else:
            loss = loss + (ce_r * sw).mean() + (ce_v * sw).mean() + (ce_p * sw).mean()
        s = ns
    if divide_by_length:
        loss = loss / L
    l2 = 0.5 * sum((p ** 2).sum() for m in muzero_instance.network if isinstance(m, torch.nn.Module)
                   for p in m.parameters())
    return loss + 1e-4 * l2


def stochastic_loss_fn(muzero_instance, batch: Transition, vqvae_beta: float = 0.25, divide_by_length: bool = False,
                       sample_weight=None):
    """The Stochastic MuZero loss for a model built on an `SMZNetwork` (module docstring).  `batch` fields are [B, L, ...]
    with an observation for EVERY step (obs [B, L, obs_dim]): the chance code of transition i is encoded from obs_i.
    Step 0 contributes CE(v_0, Rn_0) + CE(pi_0, pi_0); transition i = 1..L-1, with action a_{i-1} and the code of obs_i:
    CE(r, r_{i-1}) + CE(v_i, Rn_i) + CE(pi_i, pi_i) + CE(chance_logits, sg(code)) + CE(afterstate value, Rn_{i-1})
    + vqvae_beta * mean ||encoded - sg(onehot)||^2, each a mean over the batch (`sample_weight` [B]: of weight * term)."""
    m = muzero_instance
    dev = m.device
    rep, pred, after_dy, after_pred, chance_dy, enc = m.network
    fdt = next((p.dtype for n in m.network if isinstance(n, torch.nn.Module) for p in n.parameters()), torch.float32)
    t = lambda x, dt=fdt: torch.as_tensor(x, dtype=dt, device=dev)  # noqa: E731
    a = t(batch.a, torch.long)
    B, L = a.shape[:2]
    a = a.reshape(B, L)
    obs = t(batch.obs)
    check_every_observation(obs.shape, B, L)
    S = m._support_size
    r_t = mx_utils.scalar_to_support(t(batch.r).reshape(B, L), S).detach()
    Rn_t = mx_utils.scalar_to_support(t(batch.Rn).reshape(B, L), S).detach()
    pi = t(batch.pi).reshape(B, L, -1).detach()
    sw = None
    if sample_weight is not None:
        sw = torch.as_tensor(sample_weight, device=dev).detach().to(fdt)
        check_sample_weight(sw, B)
    mean = (lambda x: x.mean()) if sw is None else (lambda x: (x * sw).mean())
    s = rep(obs[:, 0])
    v, logits = pred(s)
    loss = mean(softmax_cross_entropy(v, Rn_t[:, 0])) + mean(softmax_cross_entropy(logits, pi[:, 0]))
    for i in range(1, L):
        encoded, onehot, code = enc.code(obs[:, i]) if hasattr(enc, "code") else _straight_through(enc(obs[:, i]))
        s = mx_utils.scale_gradient(s, 0.5)  # Appendix G
        after = after_dy(s, a[:, i - 1])
        av, chance_logits = after_pred(after)
        r, s = chance_dy(after, code)
        v, logits = pred(s)
        loss = (loss + mean(softmax_cross_entropy(r, r_t[:, i - 1])) + mean(softmax_cross_entropy(v, Rn_t[:, i]))
                + mean(softmax_cross_entropy(logits, pi[:, i])) + mean(softmax_cross_entropy(chance_logits, code.detach()))
                + mean(softmax_cross_entropy(av, Rn_t[:, i - 1]))
                + vqvae_beta * mean(((encoded - onehot.detach()) ** 2).mean(dim=-1)))
    if divide_by_length:
        loss = loss / L
    l2 = 0.5 * sum((p ** 2).sum() for n in m.network if isinstance(n, torch.nn.Module) for p in n.parameters())
    return loss + 1e-4 * l2


def _straight_through(encoded):
    """(encoded, argmax one-hot, straight-through code) for a plugin encoder that returns the code logits only."""
    onehot = torch.nn.functional.one_hot(encoded.argmax(dim=-1), encoded.shape[-1]).to(encoded.dtype)
    return encoded, onehot, encoded + (onehot - encoded).detach()


# ---------------------------------------------------------------------------------------------------
# HIP path: loss and gradients in one fused forward+backward kernel and its fixed-order reduction, for the default MLP
# trio (muax_amd/csrc/mz_train.cuh through mzs_mlp_loss_grad) and the default stochastic MLP family
# (mz_stoch_train.cuh through mzs_stochastic_mlp_loss_grad).  The two kernels are built from the same blocks
# (mz_train_blocks.cuh) and the two wrappers from `_FusedStep`, which stands on `_call.FusedCall` beside the unrolls.
# ---------------------------------------------------------------------------------------------------
class _FusedStep(_call.FusedCall):
    """What the two fused training steps have on top of `_call.FusedCall`: the flat gradient with its `views`, the loss,
    the workspace, the batch plumbing and the keep-alive of what the launch reads.  A subclass sets obs_dim / E / A
    (/ C), names its weights and states `_num_params`, `_workspace_bytes`, `_obs` and `_launch`."""

    def __init__(self, muzero_instance, params, names, weight_struct):
        super().__init__(muzero_instance, params, names, weight_struct)
        n = int(self._num_params())
        assert n == sum(x.numel() for x in self.params)
        self.grads = torch.zeros(n, dtype=torch.float32, device=self.dev)
        self.loss = torch.zeros(1, dtype=torch.float32, device=self.dev)
        self.views = [g.view_as(x) for g, x in zip(self.grads.split([x.numel() for x in self.params]), self.params)]
        self._ws = None

    def _step(self, batch, divide_by_length, sample_weight, **extra):
        dev, t, f32 = self.dev, _call.as_device, torch.float32
        a = t(batch.a, torch.int32, dev)
        B, L = a.shape[:2]
        a = a.reshape(B, L)
        obs = self._obs(t(batch.obs, f32, dev), B, L)
        if obs.shape[-1] != self.obs_dim:
            raise ValueError(f"batch.obs has {obs.shape[-1]} features, the network takes {self.obs_dim}")
        r, Rn = t(batch.r, f32, dev).reshape(B, L), t(batch.Rn, f32, dev).reshape(B, L)
        pi = t(batch.pi, f32, dev).reshape(B, L, self.A)
        sw = None
        if sample_weight is not None:
            check_sample_weight(sample_weight, B)
            sw = t(sample_weight.detach() if isinstance(sample_weight, torch.Tensor) else sample_weight, f32, dev)
        need = int(self._workspace_bytes(B))
        if self._ws is None or self._ws.numel() * 4 < need:
            self._ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=dev)
        w, keep = self._weights.get()
        self._launch(w, _call.device_index(dev), B, L, obs, a, r, Rn, pi, sw,
                     1.0 / (B * L) if divide_by_length else 1.0 / B, **extra)
        self._keep, self._keep_w = (obs, a, r, Rn, pi, keep), sw  # (alive until the next call: the launch is asynchronous)
        return self.loss, self.grads


class FusedLossGrad(_FusedStep):
    """value_and_grad of the default loss (muax/loss.py:10-88 via muax/model.py:245-249) for the default
    MLP trio.  The gradient comes back as ONE flat fp32 vector in the C-ABI's array order (that is also the
    buffer a data-parallel all-reduce works on); `views` maps it onto the 18 parameters."""

    def __init__(self, muzero_instance):
        from . import nn as mz_nn
        if not mz_nn.is_default_mlp_trio(muzero_instance.network):
            raise ValueError("the fused training step is built for the default MLP trio")
        r, p, _ = muzero_instance.network
        self.obs_dim, self.E, self.A = r.obs_dim, r.embedding_dim, p.num_actions
        super().__init__(muzero_instance, mz_nn.mlp_trio_weights(muzero_instance.network), _lib.MLP_WEIGHT_NAMES,
                         _lib.MzsMlpWeights)

    def _num_params(self):
        return self._L.mzs_mlp_num_params(self.obs_dim, self.E, self.A, self.S)

    def _workspace_bytes(self, B):
        return self._L.mzs_mlp_train_workspace_bytes(B, self.obs_dim, self.E, self.A, self.S)

    def _obs(self, obs, B, L):  # the first row of every window
        return obs[:, 0].reshape(B, -1).contiguous()

    def __call__(self, batch: Transition, divide_by_length: bool = False, sample_weight=None):
        """(loss [1], flat gradient) of the batch.  `sample_weight` [B] (float32 on the device is read in place): the
        weighted entry mzs_mlp_loss_grad_weighted, each row's cross entropies and gradient scaled by its weight."""
        return self._step(batch, divide_by_length, sample_weight)

    def _launch(self, w, idx, B, L, obs, a, r, Rn, pi, sw, loss_scale):
        w.obs_dim, w.support_size, w.discount = self.obs_dim, self.S, self.m._discount
        args = _lib.args(_lib.MzsTrainArgs)  # (per update: fields by attribute, which is 1 us cheaper than keywords)
        args.device, args.batch, args.unroll_steps, args.num_actions, args.embed_dim = idx, B, L, self.A, self.E
        args.obs, args.actions, args.rewards = obs.data_ptr(), a.data_ptr(), r.data_ptr()
        args.returns, args.policy = Rn.data_ptr(), pi.data_ptr()
        args.loss_scale = loss_scale
        args.l2_coeff = 1e-4
        args.loss, args.grads = self.loss.data_ptr(), self.grads.data_ptr()
        args.workspace, args.workspace_bytes = self._ws.data_ptr(), self._ws.numel() * 4
        stream = _call.raw_stream(idx)
        if sw is None:
            _lib.check(self._L.mzs_mlp_loss_grad(C.byref(w), C.byref(args), stream))
        else:
            _lib.check(self._L.mzs_mlp_loss_grad_weighted(C.byref(w), C.byref(args), sw.data_ptr(), stream))


class StochasticFusedLossGrad(_FusedStep):
    """value_and_grad of `stochastic_loss_fn` for the default stochastic MLP family, `FusedLossGrad`'s sibling: loss and
    every gradient from one forward+backward HIP kernel and its fixed-order reduction (muax_amd/csrc/mz_stoch_train.cuh
    through mzs_stochastic_mlp_loss_grad).  The gradient is ONE flat fp32 vector in the C-ABI's order of the 34 arrays
    (`_lib.STOCHASTIC_TRAIN_WEIGHT_NAMES`); `views` maps it onto the parameters.  The kernel hands the chance dynamics the
    exact one-hot of the code where `stochastic_loss_fn` computes e + (onehot - e) in floating point."""

    def __init__(self, muzero_instance):
        from . import nn as mz_nn
        if not mz_nn.is_default_stochastic_mlp(muzero_instance.network):
            raise ValueError("the fused stochastic training step is built for the default stochastic MLP family")
        r, p, _, ap, _, _ = muzero_instance.network
        self.obs_dim, self.E, self.A, self.C = r.obs_dim, r.embedding_dim, p.num_actions, ap.num_actions
        super().__init__(muzero_instance, mz_nn.stochastic_train_weights(muzero_instance.network),
                         _lib.STOCHASTIC_TRAIN_WEIGHT_NAMES, _lib.MzsStochasticTrainWeights)

    def _num_params(self):
        return self._L.mzs_stochastic_mlp_num_params(self.obs_dim, self.E, self.A, self.C, self.S)

    def _workspace_bytes(self, B):
        return self._L.mzs_stochastic_mlp_train_workspace_bytes(B, self.obs_dim, self.E, self.A, self.C, self.S)

    def _obs(self, obs, B, L):  # a row for every step
        check_every_observation(obs.shape, B, L)
        return obs[:, :L].reshape(B, L, -1).contiguous()

    def __call__(self, batch: Transition, vqvae_beta: float = 0.25, divide_by_length: bool = False, sample_weight=None):
        """(loss [1], flat gradient) of the batch; `batch.obs` is [B, L, obs_dim], an observation for every step."""
        return self._step(batch, divide_by_length, sample_weight, vqvae_beta=vqvae_beta)

    def _launch(self, w, idx, B, L, obs, a, r, Rn, pi, sw, loss_scale, vqvae_beta):
        w.obs_dim, w.support_size = self.obs_dim, self.S
        args = _lib.args(_lib.MzsStochasticTrainArgs, device=idx, batch=B, unroll_steps=L, num_actions=self.A,
                         num_chance_outcomes=self.C, embed_dim=self.E, obs=obs.data_ptr(), actions=a.data_ptr(),
                         rewards=r.data_ptr(), returns=Rn.data_ptr(), policy=pi.data_ptr(),
                         sample_weight=None if sw is None else sw.data_ptr(), loss_scale=loss_scale, l2_coeff=1e-4,
                         vqvae_beta=float(vqvae_beta), loss=self.loss.data_ptr(), grads=self.grads.data_ptr(),
                         workspace=self._ws.data_ptr(), workspace_bytes=self._ws.numel() * 4)
        with torch.cuda.device(idx):
            _lib.check(self._L.mzs_stochastic_mlp_loss_grad(C.byref(w), C.byref(args), _call.raw_stream(idx)))
