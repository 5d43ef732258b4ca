"""MuZero model object with the reference's act() contract (muax/model.py:16-283; README-era
constructor muax/frameworks/coax/model.py:101-110), backed by the HIP search.

    model = MuZero(network)                       # muax/model.py:43-50
    model = MuZero(repr_fn, pred_fn, dy_fn)       # muax/frameworks/coax/model.py:101-110
    model.init(rng_key, sample_input)
    a, pi, v = model.act(rng_key, obs, with_pi=True, with_value=True, num_simulations=50)

What runs where: the default MLP trio of muax/nn.py is evaluated inside the fused gfx950 kernel (one
launch per act); any other torch plugin nets run as torch modules between the step-wise kernels, at
the points where mctx calls root_fn / recurrent_fn.  There is no CPU search path.
"""
from __future__ import annotations

import os
from typing import Optional

import numpy as np
import torch

from . import _lib
from . import loss as mz_loss
from . import nn as mz_nn
from . import prng
from . import sharding
from . import unroll as mz_unroll
from . import utils as mx_utils
from ._call import capture, device_index, raw_stream
from .nn import MZNetwork, MZNetworkParams, SMZNetwork, SMZNetworkParams
from .optimizers import optimizer  # noqa: F401  (the README's `muax.model.optimizer(...)`)
from .policy import GumbelMuZeroPolicy, MuZeroPolicy, Policy, StochasticMuZeroPolicy
from .search import (ChanceRecurrentFnOutput, DecisionRecurrentFnOutput, MuZeroSearch, PolicyOutput,  # noqa: F401
                     SearchConfig, stochastic_plan)  # (PolicyOutput: re-exported type)


def _dirichlet(key_words, alpha: float, shape, device, global_batch=None, root_offset=0) -> torch.Tensor:
    """Root exploration noise of mctx.muzero_policy: rows [root_offset, root_offset + B) of
    jax.random.dirichlet(dirichlet_key, full([A], alpha), (global_batch,)) -- jax's sampler (loggamma by
    Marsaglia-Tsang rejection on the threefry key walk, softmax) restated on the device, ONE launch
    (mzs_dirichlet, muax_amd/csrc/mz_dirichlet.cuh).  The key walk is exact; the float bits are spec-to-confirm
    against a real jax (oracle/mz_oracle.c), so `dirichlet_noise=` stays the way to inject an exact array."""
    import ctypes as C
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("muax_amd draws the root noise on the GPU (there is no CPU search path)")
    B, A = shape
    kw = (C.c_uint32 * 2)(int(key_words[0]) & 0xFFFFFFFF, int(key_words[1]) & 0xFFFFFFFF)
    idx = device_index(device)
    device = torch.device("cuda", idx)  # ONE ordinal for the buffer, the stream and the launch
    out = torch.empty(B, A, dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.load().mzs_dirichlet(idx, C.byref(kw), float(alpha), B, A, global_batch or B,
                                             root_offset, out.data_ptr(), raw_stream(idx)))
    return out


def _jit_tail():
    from . import _jit
    return _jit.build_log_tail(3)


_NO_KEYWORDS = {}  # (of update()'s fused call for the trio: one shared object, none built per update)


# What update() calls after an Unsupported from a fused step (`on_demand` of _fused_update's record): True when an
# instance for the step's shape is now registered, False when none can be had, None when the refusal is not about one.
# (The builders are looked up in _jit at call time.)
def _trio_train_on_demand(step, refusal):
    """muax_amd/_jit.py::ensure_train_instance, or ensure_wide_train_instance for 17 to 64 actions."""
    from . import _jit
    if not isinstance(refusal, _lib.NoKernelInstance):
        return None
    shape = (step.A, step.E, 2 * step.S + 1)
    return _jit.ensure_train_instance(*shape) or _jit.ensure_wide_train_instance(*shape)


def _stochastic_train_on_demand(step, refusal):
    """muax_amd/_jit.py::ensure_stochastic_train_instance for the step's (A, C, E, F) and observation width.  Beyond 32
    observations the library's refusal, with nothing registered, is its plain "obs_dim must be 1..32": an instance at a
    wider cap lifts that one too."""
    from . import _jit
    if not (isinstance(refusal, _lib.NoKernelInstance) or (step.obs_dim > 32 and "obs_dim" in str(refusal))):
        return None
    return _jit.ensure_stochastic_train_instance(step.A, step.C, step.E, 2 * step.S + 1, step.obs_dim)


class MuZero:
    r"""MuZero algorithm (muax/model.py:16-50).

    Parameters mirror the reference: `network` (MZNetwork) or the three plugin callables, `policy_class`
    / `policy` ("muzero" or "gumbel"; "stochastic" with an `SMZNetwork` -- nn.create_stochastic_muzero_network or six
    plugin modules: Stochastic MuZero, chance nodes in the search and loss.stochastic_loss_fn in update(); with a plain
    MZNetwork it raises NotImplementedError, the trio has no decision and chance functions), `optimizer`, `loss_fn`,
    `discount`, `support_size`.  `recurrent_pred_on` selects which
    embedding the prediction net sees inside the search: "child" as muax/model.py:272, "parent" as the
    pip-release class muax/frameworks/coax/model.py:447-448.
    """

    def __init__(self, network=None, prediction_fn=None, dynamic_fn=None, policy_class=MuZeroPolicy,
                 policy: Optional[str] = None, optimizer=None, loss_fn=None, discount: float = 0.99,
                 support_size: int = 10, recurrent_pred_on: str = "child", device=None,
                 representation_fn=None, capture_graph: bool = False, root_graph_cache: int = 2,
                 stochastic_one_launch: bool = False, stochastic_fused_update: bool = False,
                 stochastic_root_in_kernel: bool = False, stochastic_unroll_values: bool = False,
                 stochastic_train_on_demand: bool = False, stochastic_noise_in_kernel: bool = False):
        self._stochastic = isinstance(network, SMZNetwork)
        if self._stochastic:
            if policy not in (None, "stochastic"):
                raise ValueError(f"policy={policy!r}: an SMZNetwork runs policy='stochastic'")
            self.network, policy, policy_class = network, None, StochasticMuZeroPolicy
        elif isinstance(network, MZNetwork):
            self.network = network
        else:
            rep = representation_fn if representation_fn is not None else network
            if rep is None or prediction_fn is None or dynamic_fn is None:
                raise ValueError("give either an MZNetwork or representation_fn, prediction_fn and dynamic_fn")
            self.network = MZNetwork(rep, prediction_fn, dynamic_fn)
        if policy is not None:
            if policy not in ("muzero", "gumbel"):
                # (an MZNetwork trio has no decision / chance functions to hand the stochastic search)
                raise NotImplementedError(f"policy={policy!r}: an MZNetwork runs 'muzero' and 'gumbel'; policy='stochastic' "
                                          "needs an SMZNetwork (nn.create_stochastic_muzero_network), or call "
                                          "StochasticMuZeroPolicy directly with decision_recurrent_fn and chance_recurrent_fn")
            policy_class = MuZeroPolicy if policy == "muzero" else GumbelMuZeroPolicy
        if not (isinstance(policy_class, type) and issubclass(policy_class, Policy)):
            raise TypeError("policy_class must be a subclass of muax_amd.policy.Policy")
        if self._stochastic:
            (self.repr_func, self.pred_func, self.after_dy_func, self.after_pred_func, self.chance_dy_func,
             self.enc_func) = self.network
            self.dy_func = None
        else:
            self.repr_func, self.pred_func, self.dy_func = self.network
        # of the last act(): "fused_host", "fused", "stepwise"; "hip_stochastic_mlp", "hip_stochastic_one_launch", their
        # "..._root" twins (stochastic_root_in_kernel), the one-launch names + "_noise" (stochastic_noise_in_kernel), "callables"
        self._last_route = None
        self._policy = policy_class()
        self._optimizer = optimizer
        self.loss_fn = loss_fn
        self._discount = float(discount)
        self._support_size = int(support_size)
        if recurrent_pred_on not in ("child", "parent"):
            raise ValueError("recurrent_pred_on must be 'child' or 'parent'")
        self._recurrent_pred_on = recurrent_pred_on
        self.device = torch.device(device) if device is not None else (
            torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu"))
        # plugin (non-default) nets: run the S x (select, recurrent_fn, expand_backup) loop as one hipGraph
        self.capture_graph = bool(capture_graph)
        # default stochastic MLP family: the whole search in one launch wherever search.stochastic_plan admits the shape
        # (off by default: the two routes give the same bits, the speed is measured on one shape only -- README)
        self.stochastic_one_launch = bool(stochastic_one_launch)
        # default stochastic MLP family on the library route: root inference by the library too (in the one launch, or
        # one launch in front of the three-launch loop) instead of the torch modules (off by default: README)
        self.stochastic_root_in_kernel = bool(stochastic_root_in_kernel)
        # default stochastic MLP family on the one-launch route: act() draws the root's Dirichlet noise inside that launch
        # instead of by a launch of its own (off by default: the same bits, the speed is measured on one shape -- README)
        self.stochastic_noise_in_kernel = bool(stochastic_noise_in_kernel)
        # default stochastic MLP family: update() takes loss and gradients from the fused training kernel
        # (loss.StochasticFusedLossGrad) instead of torch autograd (off by default: timed on two shapes only -- README)
        self.stochastic_fused_update = bool(stochastic_fused_update)
        # ... and a shape without a listed instance of that kernel, or observations 33 to 128 wide, gets an instance built
        # on demand (_jit.ensure_stochastic_train_instance) instead of autograd; only together with the flag above (off
        # by default: README)
        self.stochastic_train_on_demand = bool(stochastic_train_on_demand)
        # an SMZNetwork: unroll_values() unrolls through the afterstate and chance dynamics, the codes from the encoder --
        # one launch for the default stochastic MLP family (unroll.StochasticFusedUnrollValues), else the modules; with it
        # fit_vector takes priority_steps (off by default: unroll_values() then raises NotImplementedError as before -- README)
        self.stochastic_unroll_values = bool(stochastic_unroll_values)
        self._last_update_route = None  # of the last update(): "hip_stochastic_fused", "hip_fused", "torch"
        # captured root-inference graphs kept per weights version (one per observation shape; each pins its static
        # input and a private memory pool: hundreds of MB for Atari-shaped batches -- INTEGRATION.md)
        self.root_graph_cache = max(1, int(root_graph_cache))
        self._params = None
        self._opt_state_saved = None  # what init() / a checkpoint produced before an optimiser was bound
        self._loaded_opt_state = None
        self._fused_train = None
        self._fused_stoch_train = None
        self._fused_unroll = None
        self._disc_const = None
        self._fused = {}
        self._root_graphs = {}
        self._root_graph_lru = []
        self._weights_version = 0

    # ------------------------------------------------------------------ init / params
    def init(self, rng_key, sample_input):
        """muax/model.py:62-80: materialise the three nets for `sample_input` ([B, ...])."""
        seed = int(prng.as_key(rng_key)[0]) << 32 | int(prng.as_key(rng_key)[1])
        torch.manual_seed(seed & 0x7FFFFFFFFFFFFFFF)
        x = torch.as_tensor(np.asarray(sample_input), dtype=torch.float32)
        for m in self.network:  # lazily built layers are created on the host, then everything moves
            if isinstance(m, torch.nn.Module):
                m.to("cpu")
        with torch.no_grad():
            s = self.repr_func(x)
            self.pred_func(s)
            zeros = torch.zeros(s.shape[0], dtype=torch.long)
            if self._stochastic:  # all six modules
                after = self.after_dy_func(s, zeros)
                self.after_pred_func(after)
                self.chance_dy_func(after, zeros)
                self.enc_func(x)
            else:
                self.dy_func(s, zeros)
        for m in self.network:
            if isinstance(m, torch.nn.Module):
                m.to(self.device)
        self._params = (SMZNetworkParams if self._stochastic else MZNetworkParams)(*[dict(m.named_parameters()) if isinstance(m, torch.nn.Module) else None
                                         for m in self.network])
        self._weights_version += 1
        self._fused_train = None
        self._fused_stoch_train = None
        self._fused_unroll = None
        return self._params

    @property
    def params(self):
        return self._params

    @property
    def _opt_state(self):
        # optimiser moments + schedule position, read when asked for (building the dict costs ~10 us: not per update())
        if self._optimizer is not None and self._optimizer.opt is not None:
            return self._optimizer.state_dict()
        return self._opt_state_saved

    @_opt_state.setter
    def _opt_state(self, value):
        self._opt_state_saved = value

    @property
    def optimizer_state(self):
        return self._opt_state

    def weights_changed(self):
        """Call after modifying parameters in place (the fused kernel reads the live tensors, but
        shape/dtype checks are cached per version)."""
        self._weights_version += 1

    # ------------------------------------------------------------------ sub-networks (coax API)
    def representation(self, obs):
        """muax/frameworks/coax/model.py:144-157."""
        with torch.no_grad():
            return self.repr_func(torch.as_tensor(obs, dtype=torch.float32, device=self.device))

    def prediction(self, s):
        """muax/frameworks/coax/model.py:159-173."""
        with torch.no_grad():
            return self.pred_func(torch.as_tensor(s, dtype=torch.float32, device=self.device))

    def dynamic(self, s, a):
        """muax/frameworks/coax/model.py:175-191."""
        with torch.no_grad():
            return self.dy_func(torch.as_tensor(s, dtype=torch.float32, device=self.device),
                                torch.as_tensor(a, device=self.device))

    # ------------------------------------------------------------------ inference glue
    def _root_inference(self, params, rng_key, obs):
        """muax/model.py:251-263 -> (prior_logits [B,A], value [B], embedding [B,...]).  With
        capture_graph=True the plugin nets' root inference (dozens of small torch kernels for a convolutional
        representation net: launch-bound, 8 of config 4's 39 ms per act were gaps between them) is captured once
        per (shape, weights version) into a hipGraph and replayed on a static input buffer; the returned tensors
        are the graph's static outputs (consumed by mzs_root in stream order before the next replay)."""
        if self.capture_graph and obs.is_cuda and not torch.cuda.is_current_stream_capturing():
            key = (tuple(obs.shape), obs.dtype, obs.device, self._weights_version)
            ent = self._root_graphs.get(key)
            if ent is None:
                # drop graphs of stale weights; keep the other shapes of THIS version (a B = 1 test rollout next to
                # a batched act() must not re-capture on every alternation), at most `root_graph_cache` of them;
                # _root_graph_lru lists the keys least recently used first
                for k in [k for k in self._root_graphs if k[3] != self._weights_version]:
                    del self._root_graphs[k]
                self._root_graph_lru = [k for k in self._root_graph_lru if k in self._root_graphs]
                while len(self._root_graphs) >= self.root_graph_cache:
                    del self._root_graphs[self._root_graph_lru.pop(0)]
                static_in = obs.clone()
                cur = torch.cuda.current_stream(obs.device)
                side = torch.cuda.Stream(device=obs.device)
                side.wait_stream(cur)
                with torch.cuda.stream(side):  # lazy layer creation and MIOpen's solver search stay out of the capture
                    for _ in range(2):
                        self._root_inference_eager(static_in)
                cur.wait_stream(side)
                g = torch.cuda.CUDAGraph()
                with capture(g):
                    out = self._root_inference_eager(static_in)
                ent = self._root_graphs[key] = (g, static_in, out)
                self._root_graph_lru.append(key)
            else:
                self._root_graph_lru.remove(key)
                self._root_graph_lru.append(key)  # most recently used last
            ent[1].copy_(obs)
            ent[0].replay()
            return ent[2]
        return self._root_inference_eager(obs)

    def _root_inference_eager(self, obs):
        with torch.no_grad():
            hip_root = getattr(self.repr_func, "hip_root", None)
            if hip_root is not None:  # ResNet nets: last pool + min-max + prediction net + value decode in one launch
                out = hip_root(obs, self.pred_func, self._support_size)
                if out is not None:
                    return out[2], out[1], out[0]
            s = self.repr_func(obs)
            v, logits = self.pred_func(s)
            v = mx_utils.support_to_scalar(torch.softmax(v, dim=-1), self._support_size).flatten()
        return logits, v, s

    def _recurrent_inference(self, params, rng_key, action, embedding):
        """muax/model.py:265-282 -> ((reward, discount, prior_logits, value), next_embedding)."""
        if self._recurrent_pred_on == "child" and hasattr(self.dy_func, "hip_recurrent"):
            out = self.dy_func.hip_recurrent(self.pred_func, embedding, action, self._support_size)
            if out is not None:  # ResNet nets: the whole recurrent_fn is one HIP launch (mz_conv.cuh)
                r, v, logits, next_embedding = out
                if self._disc_const is None or self._disc_const.shape != r.shape or self._disc_const.device != r.device:
                    self._disc_const = torch.full_like(r, self._discount)  # one constant tensor, not a fill per simulation
                return (r, self._disc_const, logits, v), next_embedding
        with torch.no_grad():
            r, next_embedding = self.dy_func(embedding, action)
            v, logits = self.pred_func(embedding if self._recurrent_pred_on == "parent" else next_embedding)
            r = mx_utils.support_to_scalar(torch.softmax(r, dim=-1), self._support_size).flatten()
            v = mx_utils.support_to_scalar(torch.softmax(v, dim=-1), self._support_size).flatten()
            discount = torch.ones_like(r) * self._discount
        return (r, discount, logits, v), next_embedding

    def _native_loop(self, root):
        """The one-launch simulation loop, when the nets are ones the library evaluates itself (the reference's ResNet
        nets with the prediction net on the child's embedding): a callable for MuZeroSearch.search, else None."""
        dy = self.dy_func
        if self._recurrent_pred_on != "child" or not hasattr(dy, "hip_search_ok"):
            return None
        if not dy.hip_search_ok(self.pred_func, tuple(root[2].shape[1:]), self._support_size):
            return None
        return lambda handle, b, e: dy.hip_search(self.pred_func, handle, self._support_size, self._discount, b, e)

    # ------------------------------------------------------------------ act
    def _device_obs(self, obs):
        """Observations as a float32 tensor on the model's device: what the torch modules take."""
        return obs if isinstance(obs, torch.Tensor) and obs.device == self.device \
            else torch.as_tensor(obs, dtype=torch.float32).to(self.device)

    def _root_noise(self, key, noise, fraction, alpha, obs, A, global_batch, root_offset):
        """mctx.muzero_policy's root noise [B, A] for the roots `obs`: `noise` when the caller gave one (or switched the
        noise off), else rows [root_offset, root_offset + B) of the global batch's Dirichlet draw -- a shard draws exactly
        its rows, results do not depend on the split.  A = None: one row through the plugin nets tells the width."""
        if noise is not None or not fraction:
            return noise
        B = obs.shape[0]
        if A is None:
            with torch.no_grad():
                A = self.pred_func(self.repr_func(self._device_obs(obs[:1])))[1].shape[-1]
        k_dir = prng.split(key, 3)[1]  # mctx: rng_key, dirichlet_rng_key, search_rng_key = split(key, 3)
        return _dirichlet(k_dir, alpha, (B, A), self.device, global_batch, root_offset)

    def _handle(self, batch, cfg, bind, *more):
        """The MuZeroSearch handle of an act() configuration, cached under (batch, cfg, *more); `cfg`: SearchConfig's
        arguments in the order of its fields.  Created once (mzs_create + its device buffers); a new weights version
        only re-binds the weight pointers (`bind(handle, *more)`), it does not re-create the handle -- no allocation on the
        update()-then-act() cycle of fit()."""
        key = (batch, cfg) + more
        h = self._fused.get(key)
        if h is None:
            h = self._fused[key] = [MuZeroSearch(batch, SearchConfig(*cfg), self.device), None]
        if h[1] != self._weights_version:
            bind(h[0], *more)
            h[1] = self._weights_version
        return h[0]

    def _bind_trio(self, handle, obs_dim):
        w = {k: v.detach() for k, v in mz_nn.mlp_trio_weights(self.network).items()}
        handle.set_mlp_weights(w, obs_dim, self._support_size, self._discount, self._recurrent_pred_on)

    def _act_fused(self, key, obs, host_io, gumbel, cfg, kw):
        """One act() of the default MLP trio inside the library -> _route's record, or None.  `host_io`: the whole round
        trip in one C call (mzs_act_mlp_host: staging, root-noise draw from the key, search, one download, sync; NumPy
        results), else mzs_act_mlp on device tensors, results in the handle's buffers.  `cfg`: the handle's SearchConfig
        arguments, (A, S, E, ...); `kw`: the call's keyword arguments; `gumbel`: the policy class.  When the library has no instance
        of the fused kernel for the shape, build one on demand (muax_amd/_jit.py: one translation unit, cached on disk,
        planned for the policy class) and call again; a shape outside that kernel's limits (more than 16 actions, more
        than 255 simulations, embeddings wider than 64) switches the handle to the library's wide-action kernel (17..64
        actions: mzs_mlp_allow_wide for the MuZero policy, mzs_mlp_allow_wide_gumbel for the Gumbel policy;
        MUAX_AMD_WIDE=0 skips both) and its generic one-launch search (mzs_mlp_allow_generic; MUAX_AMD_GENERIC=0), which
        takes what the wide kernel declines.  None when none of them takes the shape: the caller then runs the step-wise
        path with the torch modules."""
        A, S, E = cfg[:3]
        B, obs_dim = obs.shape
        h = self._handle(B, cfg, self._bind_trio, obs_dim)
        call = h.act_mlp_host if host_io else h.act_mlp
        try:
            try:
                out = call(obs, key, **kw)
            except _lib.NoKernelInstance:
                from . import _jit
                if not _jit.ensure_instance(A, E, 2 * self._support_size + 1, S, gumbel=gumbel):
                    tail = _jit.build_log_tail()
                    if tail and _jit.last_build_log not in MuZero._warned_stepwise:  # a compiler was there and the build FAILED: say so
                        MuZero._warned_stepwise.add(_jit.last_build_log)
                        import warnings
                        warnings.warn(f"muax_amd: the on-demand build of a fused act() instance for num_actions={A}, embedding_dim="
                                      f"{E}, num_simulations={S} failed; compiler log {_jit.last_build_log}:\n{tail}",
                                      RuntimeWarning, stacklevel=3)
                    wide = os.environ.get("MUAX_AMD_WIDE", "1") != "0"
                    generic = os.environ.get("MUAX_AMD_GENERIC", "1") != "0"
                    if not (wide or generic):
                        raise
                    if wide:
                        h.allow_wide(gumbel=gumbel)
                    if generic:
                        h.allow_generic()
                out = call(obs, key, **kw)
        except _lib.NoKernelInstance as e:
            self._warn_stepwise(A, E, S, e)
            return None
        if host_io:
            return PolicyOutput(out[0], out[1], None), out[2], None, "fused_host"
        return out, h.root_value, h, "fused"

    def _route(self, rng_key, obs, *, num_simulations=5, temperature=1., invalid_actions=None, max_depth=None,
               loop_fn=None, qtransform=None, dirichlet_fraction=0.25, dirichlet_alpha=0.3, pb_c_init=1.25,
               pb_c_base=19652, dirichlet_noise=None, gumbel=None, tiebreak=True, with_tree=False,
               max_num_considered_actions=16, gumbel_scale=1.0, global_batch=None, root_offset=0,
               host_io=False):
        """One search of `obs` [B, ...] by the first route that takes it (the keywords and defaults of
        muax/model.py:222-243) -> the record (PolicyOutput, the root's network value, the fused handle whose buffers
        hold both -- they then come back in one copy -- or None, the route's name).  `host_io`: the caller gave host
        observations and wants host results; the fused path then makes the whole round trip in one C call and the
        PolicyOutput holds NumPy arrays."""
        if self._params is None:
            raise ValueError("call init() first")
        key = prng.as_key(rng_key)
        if self._stochastic:
            return self._plan_stochastic(key, obs, num_simulations, temperature, invalid_actions, max_depth, qtransform,
                                         dirichlet_fraction, dirichlet_alpha, pb_c_init, pb_c_base, dirichlet_noise, gumbel,
                                         tiebreak, with_tree, global_batch, root_offset)
        gumbel_policy = isinstance(self._policy, GumbelMuZeroPolicy)
        if qtransform is None:
            qtransform = "qtransform_by_parent_and_siblings"  # muax/model.py:230-231, for EVERY policy
        qtransform = getattr(qtransform, "__name__", qtransform)
        if qtransform != "qtransform_by_parent_and_siblings" and not (
                gumbel_policy and qtransform == "qtransform_completed_by_mix_value"):
            raise ValueError(f"qtransform {qtransform!r} is not implemented for this policy")
        S, A = num_simulations, getattr(self.pred_func, "num_actions", None)
        # the fused kernels: the default MLP trio under a policy of the library's own -- a user subclass never
        fused = mz_nn.is_default_mlp_trio(self.network) and obs.ndim == 2 \
            and type(self._policy) is (GumbelMuZeroPolicy if gumbel_policy else MuZeroPolicy)
        host_io = (host_io and fused and not with_tree and gumbel is None and not isinstance(obs, torch.Tensor)
                   and not isinstance(dirichlet_noise, torch.Tensor) and not isinstance(invalid_actions, torch.Tensor))
        if not (gumbel_policy or host_io):  # (the host round trip draws its noise inside the C call)
            dirichlet_noise = self._root_noise(key, dirichlet_noise, dirichlet_fraction, dirichlet_alpha, obs, A,
                                               global_batch, root_offset)
        if fused:
            E = self.repr_func.embedding_dim
            if gumbel_policy:  # (no pUCT constants, no tie-break noise, no root noise, no temperature in this policy)
                cfg = (A, S, E, max_depth, False, 1.25, 19652.0, global_batch, root_offset, "gumbel", qtransform,
                       max_num_considered_actions, float(gumbel_scale))
                kw = dict(dirichlet_fraction=0.0, invalid_actions=invalid_actions) if host_io else \
                    dict(invalid_actions=invalid_actions, gumbel=gumbel, with_tree=with_tree)
            else:
                cfg = (A, S, E, max_depth, tiebreak, pb_c_init, float(pb_c_base), global_batch, root_offset)
                kw = dict(dirichlet_noise=dirichlet_noise, dirichlet_fraction=dirichlet_fraction,
                          dirichlet_alpha=dirichlet_alpha, invalid_actions=invalid_actions,
                          temperature=temperature) if host_io else \
                    dict(dirichlet_noise=dirichlet_noise, dirichlet_fraction=dirichlet_fraction,
                         invalid_actions=invalid_actions, temperature=temperature, gumbel=gumbel, with_tree=with_tree)
            served = self._act_fused(key, obs, host_io, gumbel_policy, cfg, kw)
            if served is not None:
                return served
        # the step-wise kernels, the torch modules between them: plugin nets, user policies, shapes the library declined
        if gumbel_policy:
            policy_kw = dict(qtransform=qtransform, max_num_considered_actions=max_num_considered_actions,
                             gumbel_scale=gumbel_scale)
        else:
            policy_kw = dict(temperature=temperature, dirichlet_fraction=dirichlet_fraction, pb_c_init=pb_c_init,
                             pb_c_base=pb_c_base, tiebreak=tiebreak,
                             dirichlet_noise=self._root_noise(key, dirichlet_noise, dirichlet_fraction, dirichlet_alpha,
                                                              obs, A, global_batch, root_offset))
        root = self._root_inference(self._params, key, self._device_obs(obs))
        out = self._checked_search(lambda: self._policy(
            self._params, key, root, self._recurrent_inference, num_simulations=S, invalid_actions=invalid_actions,
            max_depth=max_depth, gumbel=gumbel, with_tree=with_tree, graph=self.capture_graph,
            graph_version=self._weights_version, global_batch=global_batch, root_offset=root_offset,
            native_loop=self._native_loop(root), **policy_kw))
        return out, root[1], None, "stepwise"

    def _plan(self, params, rng_key, obs, **settings):
        """muax/model.py:222-243 -> (PolicyOutput, root value); `settings`: _route's keywords."""
        out, root_value, _, self._last_route = self._route(rng_key, obs, **settings)
        return out, root_value

    # ------------------------------------------------------------------ Stochastic MuZero (SMZNetwork)
    def _decision_inference(self, params, rng_key, action, embedding):
        """mctx decision_recurrent_fn -> (DecisionRecurrentFnOutput(chance_logits, afterstate_value), afterstate)."""
        with torch.no_grad():
            after = self.after_dy_func(embedding, action)
            av, chance_logits = self.after_pred_func(after)
            av = mx_utils.support_to_scalar(torch.softmax(av, dim=-1), self._support_size).flatten()
        return DecisionRecurrentFnOutput(chance_logits, av), after

    def _chance_inference(self, params, rng_key, outcome, afterstate):
        """mctx chance_recurrent_fn -> (ChanceRecurrentFnOutput(action_logits, value, reward, discount), next state)."""
        with torch.no_grad():
            r, s = self.chance_dy_func(afterstate, outcome)
            v, logits = self.pred_func(s)
            r = mx_utils.support_to_scalar(torch.softmax(r, dim=-1), self._support_size).flatten()
            v = mx_utils.support_to_scalar(torch.softmax(v, dim=-1), self._support_size).flatten()
        return ChanceRecurrentFnOutput(logits, v, r, torch.full_like(r, self._discount)), s

    def _bind_stochastic(self, handle):
        w = {k: v.detach() for k, v in mz_nn.stochastic_mlp_weights(self.network).items()}
        handle.set_stochastic_mlp_weights(w, self._support_size, self._discount)
        if self._stochastic_root_served(handle.cfg.embed_dim):
            handle.set_stochastic_representation(*[t.detach() for t in mz_nn.stochastic_root_weights(self.network)])

    def _stochastic_root_served(self, E):
        """Whether the library route runs root inference itself: the flag, and an embedding a wavefront holds."""
        return self.stochastic_root_in_kernel and E <= 64

    def _plan_stochastic(self, key, obs, num_simulations, temperature, invalid_actions, max_depth, qtransform,
                         dirichlet_fraction, dirichlet_alpha, pb_c_init, pb_c_base, dirichlet_noise, gumbel, tiebreak,
                         with_tree, global_batch, root_offset):
        """_route for an SMZNetwork: root inference on the torch modules, once; then the search with the decision and the
        chance function evaluated by the library (the default stochastic MLP family on a GPU, support_size 8..31:
        MuZeroSearch.search_stochastic_mlp, as one launch with `stochastic_one_launch` where search.stochastic_plan admits
        the shape; MUAX_AMD_STOCHASTIC_MLP=0 switches the library route off) or, for plugin modules, by
        StochasticMuZeroPolicy on callables built from them.  With `stochastic_root_in_kernel` the library route (embeddings
        up to 64 wide) runs root inference too and no torch module is called: the widths come from the modules, the
        observations go to search_stochastic_mlp(None, obs=...), the root value is the kernel's.  With
        `stochastic_noise_in_kernel` the one-launch route draws the root noise too (draw_dirichlet=dirichlet_alpha) when the
        caller gave none and dirichlet_fraction is not 0: `_root_noise` is skipped, the route's name ends in "_noise"."""
        qt = getattr(qtransform, "__name__", qtransform)
        if qt not in (None, "qtransform_by_parent_and_siblings"):
            raise ValueError(f"qtransform {qt!r} is not implemented for this policy")
        hip = (mz_nn.is_default_stochastic_mlp(self.network) and self.device.type == "cuda"
               and 8 <= self._support_size <= 31 and os.environ.get("MUAX_AMD_STOCHASTIC_MLP", "1") != "0")
        Cn = getattr(self.after_pred_func, "num_actions", None)
        in_kernel = hip and obs.ndim == 2 and self._stochastic_root_served(self.repr_func.embedding_dim)
        if in_kernel:
            root, B, A, E = None, obs.shape[0], self.pred_func.num_actions, self.repr_func.embedding_dim
        else:
            root = self._root_inference_eager(self._device_obs(obs))
            (B, A), E = root[0].shape, root[2].shape[1]
        one_launch = hip and self.stochastic_one_launch and stochastic_plan(A, Cn, E, self._support_size,
                                                                            num_simulations) is not None
        # the noise act() would draw itself (_root_noise), drawn by the one launch instead: the same rows, the same bits
        draw = one_launch and self.stochastic_noise_in_kernel and dirichlet_noise is None and bool(dirichlet_fraction)
        if not draw:
            dirichlet_noise = self._root_noise(key, dirichlet_noise, dirichlet_fraction, dirichlet_alpha, obs, A, global_batch,
                                               root_offset)
        if hip:
            h = self._handle(B, (A, num_simulations, E, max_depth, tiebreak, pb_c_init, float(pb_c_base),
                                 global_batch, root_offset, "stochastic", "qtransform_by_parent_and_siblings", 16, 1.0, Cn),
                             self._bind_stochastic)
            out = h.search_stochastic_mlp(root, key=key, invalid_actions=invalid_actions, dirichlet_noise=dirichlet_noise,
                                          dirichlet_fraction=dirichlet_fraction, temperature=temperature, gumbel=gumbel,
                                          with_tree=with_tree, graph=self.capture_graph, graph_version=self._weights_version,
                                          one_launch=one_launch, obs=self._device_obs(obs) if in_kernel else None,
                                          draw_dirichlet=dirichlet_alpha if draw else None)
            t = out.search_tree
            if t is not None:  # the decision slice, as StochasticMuZeroPolicy returns it (mctx _mask_tree)
                t = t._replace(**{f: getattr(t, f)[..., :A] for f in t._fields if f.startswith("children_")})
            route = "hip_stochastic_one_launch" if one_launch else "hip_stochastic_mlp"
            suffix = "_noise" if draw else ""
            if in_kernel:  # (action, weights and root value then share the handle's one output allocation)
                return PolicyOutput(out.action, out.action_weights, t), h.root_value, h, route + "_root" + suffix
            return PolicyOutput(out.action, out.action_weights, t), root[1], None, route + suffix
        shapes = {} if Cn is None else dict(num_chance_outcomes=Cn, afterstate_shape=tuple(root[2].shape[1:]))
        out = self._policy(self._params, key, root, decision_recurrent_fn=self._decision_inference,
                           chance_recurrent_fn=self._chance_inference, num_simulations=num_simulations,
                           temperature=temperature, invalid_actions=invalid_actions, max_depth=max_depth,
                           dirichlet_fraction=dirichlet_fraction, dirichlet_noise=dirichlet_noise, pb_c_init=pb_c_init,
                           pb_c_base=pb_c_base, gumbel=gumbel, tiebreak=tiebreak, with_tree=with_tree,
                           graph=self.capture_graph, graph_version=self._weights_version, global_batch=global_batch,
                           root_offset=root_offset, **shapes)
        return out, root[1], None, "callables"

    _warned_stepwise = set()

    def _warn_stepwise(self, A, E, S, err):
        """Loud, once per shape: the default MLP trio normally runs inside the library (a fused instance, one built on
        demand, the wide-action kernel for 17..64 actions, or the generic one-launch search); a shape none of them takes
        (support_size outside 8..31, more than 64 actions, MUAX_AMD_JIT=0 with MUAX_AMD_WIDE=0 and MUAX_AMD_GENERIC=0)
        drops to the step-wise kernels + torch modules."""
        key = (A, E, self._support_size, S)
        if key not in MuZero._warned_stepwise:
            MuZero._warned_stepwise.add(key)
            import warnings
            warnings.warn(f"muax_amd: no in-library act() route for num_actions={A}, embedding_dim={E}, support_size="
                          f"{self._support_size}, num_simulations={S} ({err}); falling back to the step-wise search "
                          f"with torch modules, which is far slower (about 70x a tuned instance at 4096 roots x 50 "
                          f"simulations; the generic one-launch route is about 16x, the wide-action kernel for 17..64 actions, "
                          f"MuZero or Gumbel policy, less)"
                          + (f"; last failed on-demand build: {_jit_tail()}" if _jit_tail() else ""),
                          RuntimeWarning, stacklevel=5)  # (act <- _route <- _act_fused <- here)

    def _checked_search(self, run):
        """Run a step-wise search; if the ResNet recurrent kernel went through pair mode (two workgroups per
        root meeting in L2, mz_conv.cuh) and any rendezvous was lost -- in ANY launch of the search, graph
        replays included -- drop pair mode and repeat the search with one workgroup per root.  Both launch
        shapes produce the same bits, so the repeat is what the undisturbed search would have returned.
        Reading the status words synchronises the device: a pair-mode search (<= 128 roots of the ResNet nets) is
        not sync-free even with device_outputs=True."""
        out = run()
        dy = self.dy_func
        if getattr(dy, "_pair_scratch", None) and dy.pair_lost():
            import warnings
            warnings.warn("muax_amd: the pair-mode recurrent kernel lost a rendezvous between the two workgroups of a "
                          "root; pair mode is disabled for this process and the search was repeated with one "
                          "workgroup per root", RuntimeWarning)
            dy.disable_pair_mode()
            self._weights_version += 1  # captured graphs hold pair-mode launches: re-capture
            out = run()
            if getattr(dy, "_pair_scratch", None):  # the repeat must not have gone through pair mode again
                raise RuntimeError("muax_amd: pair mode is still active after it was disabled")
        return out

    @staticmethod
    def _deliver(out, root_value, h, on_device):
        """(action, action_weights, root_value) of _route's record as the caller wants them: device tensors of its own
        (`on_device`: no sync) or NumPy arrays (one host sync, like the reference's np.asarray)."""
        if isinstance(out.action, np.ndarray):  # the fused path's host round trip: results are already NumPy
            return out.action, out.action_weights, root_value
        if on_device:
            # the search handle's output buffers are reused by the next act(): hand out copies (stream-ordered, no sync)
            if h is not None:
                return h.outputs_clone()  # one copy kernel instead of three
            return out.action.clone(), out.action_weights.clone(), root_value.clone()
        if h is not None:
            # fused path, device inputs: the three outputs share one allocation -> one device-to-host copy, one sync
            return h.outputs_to_host()
        # one device-to-host copy instead of three (each costs a synchronisation): action, weights, value
        B, A = out.action_weights.shape
        host = torch.cat([out.action.to(torch.float32), out.action_weights.reshape(-1),
                          root_value.reshape(-1).to(torch.float32)]).cpu().numpy()
        return host[:B].astype(np.int32), host[B:B + B * A].reshape(B, A).copy(), host[B + B * A:].copy()

    def act(self, rng_key, obs, with_pi: bool = False, with_value: bool = False, obs_from_batch: bool = False,
            num_simulations: int = 5, temperature: float = 1., invalid_actions=None, max_depth: int = None,
            loop_fn=None, qtransform=None, dirichlet_fraction: float = 0.25, dirichlet_alpha: float = 0.3,
            pb_c_init: float = 1.25, pb_c_base: float = 19652, *, dirichlet_noise=None, gumbel=None,
            tiebreak: bool = True, device_outputs: bool = False, max_num_considered_actions: int = 16,
            gumbel_scale: float = 1.0, global_batch: Optional[int] = None, root_offset: int = 0):
        r"""Acts given environment observations (muax/model.py:82-179, same arguments and defaults).

        Returns `action[, action_weights][, root_value]` in the reference's order.  Unbatched: action is a
        python int, action_weights keeps its leading 1 ([1, A], as muax/model.py:176 leaves it), root_value
        a python float.  Batched (`obs_from_batch=True`): arrays of shape [B], [B, A], [B] -- NumPy by
        default (one host sync, like the reference's np.asarray), or device tensors with
        `device_outputs=True` (no sync).  `root_value` is the NETWORK value of the root, as the reference.
        Keyword-only extras: exact `dirichlet_noise` / `gumbel` arrays, `tiebreak=False` to drop mctx's
        1e-7 tie-break noise; for the Gumbel policy `max_num_considered_actions` and `gumbel_scale`, which
        the reference documents (muax/model.py:142-147) but never plumbs through.  Multi-GPU: a rank that holds
        rows [root_offset, root_offset + B) of a `global_batch`-root batch passes both, and gets exactly the rows
        the un-sharded call would have produced (per-root PRNG streams are indexed by the global root).
        """
        if isinstance(obs, torch.Tensor):
            obs = obs.to(torch.float32)
            if not obs_from_batch:
                obs = obs.unsqueeze(0)
        else:  # host observations stay NumPy: the search handle stages them through pinned memory
            obs = np.asarray(obs, dtype=np.float32)
            if not obs_from_batch:
                obs = obs[None]
        out, root_value, handle, self._last_route = self._route(
            rng_key, obs, num_simulations=num_simulations, temperature=temperature,
            invalid_actions=invalid_actions, max_depth=max_depth, loop_fn=loop_fn, qtransform=qtransform,
            dirichlet_fraction=dirichlet_fraction, dirichlet_alpha=dirichlet_alpha, pb_c_init=pb_c_init,
            pb_c_base=pb_c_base, dirichlet_noise=dirichlet_noise, gumbel=gumbel, tiebreak=tiebreak,
            max_num_considered_actions=max_num_considered_actions, gumbel_scale=gumbel_scale,
            global_batch=global_batch, root_offset=root_offset, host_io=not (device_outputs and obs_from_batch))
        action, weights, root_value = self._deliver(out, root_value, handle, device_outputs and obs_from_batch)
        if not obs_from_batch:
            action, root_value = int(action[0]), float(root_value[0])  # weights keep their leading 1 (muax/model.py:176)
        if with_pi and with_value:
            return action, weights, root_value
        elif not with_pi and with_value:
            return action, root_value
        elif with_pi and not with_value:
            return action, weights
        return action

    # ------------------------------------------------------------------ next tier
    def update(self, batch, *args, sample_weight=None, backend: str = "auto", dp_mean: bool = True, **kwargs):
        """muax/model.py:181-201: one gradient step on a batch of k-step trajectories; returns
        {'loss': float}.  With the default MLP trio and the default loss the loss and all gradients come from
        ONE fused forward+backward HIP kernel (mzs_mlp_loss_grad, muax_amd/csrc/mz_train.cuh) into a flat
        vector; the data-parallel gradient mean is then one all-reduce of that vector (RCCL on GPUs) and the
        optimiser (muax/optimizers.py mirror on torch.optim) consumes views of it.  Plugin nets or a custom
        loss_fn take the torch autograd route (backend="torch" forces it; "hip" refuses to fall back).
        An SMZNetwork runs loss.stochastic_loss_fn on autograd; a model made with `stochastic_fused_update=True` takes the
        default stochastic MLP family's step (obs_dim up to 32, no custom loss_fn) from its own fused kernel instead
        (mzs_stochastic_mlp_loss_grad, muax_amd/csrc/mz_stoch_train.cuh; `vqvae_beta`, `divide_by_length` and
        `sample_weight` reach it), "auto" falling to autograd for a shape without a listed instance or an unroll beyond
        the kernel's LDS.  With `stochastic_train_on_demand=True` as well, a shape without a listed instance (obs_dim up
        to 128) gets one built on demand (muax_amd/_jit.py::ensure_stochastic_train_instance, once per shape, cached on
        disk) and the step is called again; where no instance can be built, "auto" falls to autograd and "hip" raises.  `_last_update_route` names the route taken: "hip_stochastic_fused", "hip_fused" or "torch".
        `dp_mean=False` skips the gradient mean over the ranks of an initialised process group (a rank-local step:
        bench.py times update() with and without its collective).
        `sample_weight` [B]: importance-sampling weights (`DeviceReplayBuffer.sample(is_beta=)`); row b's cross
        entropies and gradient count sample_weight[b] times, the L2 term once.  They reach whichever route serves the
        step -- the fused kernel (mzs_mlp_loss_grad_weighted), its on-demand retry, the torch route -- and a custom
        loss_fn as the keyword `sample_weight`, only when given.  A shape other than [B] is a ValueError before any
        launch; the values are not inspected (that would synchronise)."""
        if self._params is None:
            raise ValueError("call init() first")
        if sample_weight is not None:
            mz_loss.check_sample_weight(sample_weight, int(np.shape(batch.a)[0]))  # (np.shape reads a tensor's .shape)
            kwargs["sample_weight"] = sample_weight
        if self._optimizer is None or self._optimizer.opt is None:
            self._bind_optimizer()
        fused = None if backend == "torch" else self._fused_update(args, kwargs)
        if backend == "hip" and fused is None:
            raise ValueError("backend='hip' needs the default MLP trio on a GPU and the default loss"
                             + (" (the stochastic loss of an SMZNetwork runs on torch autograd only, unless the model was made with "
                                "stochastic_fused_update=True: the default stochastic MLP family on a GPU, obs_dim up to 32)"
                                if self._stochastic else ""))
        if fused is not None:
            cache, cls, route, on_demand, extra = fused
            try:
                step = getattr(self, cache)
                if step is None:
                    step = cls(self)
                    setattr(self, cache, step)  # (it stays after a refusal)
                divide = kwargs.get("divide_by_length", False)
                try:
                    loss, flat = step(batch, divide_by_length=divide, sample_weight=sample_weight, **extra)
                except _lib.Unsupported as e:
                    # a shape the library lists no training instance for: build one on demand (`on_demand`, once per
                    # shape, cached on disk) and call again.  `on_demand` answers None for a refusal that no instance
                    # would lift (it propagates as it is), False when no instance can be had
                    built = on_demand(step, e) if on_demand and not isinstance(e, _lib.TooLargeForLds) else None
                    if built is None or (not built and isinstance(e, _lib.NoKernelInstance)):
                        raise
                    if not built:
                        raise _lib.NoKernelInstance(f"{e} (and no kernel instance could be built on demand)") from e
                    loss, flat = step(batch, divide_by_length=divide, sample_weight=sample_weight, **extra)
                if dp_mean:
                    sharding.allreduce_mean_flat([flat])
                for p, g in zip(step.params, step.views):
                    p.grad = g
            except (_lib.NoKernelInstance, _lib.TooLargeForLds):
                # shapes the kernel cannot serve (no instance, or an unroll longer than its LDS keeps) take the
                # torch route under backend="auto"; the kernel refuses them on the host, before any launch
                if backend == "hip":
                    raise
                fused = None
        if fused is None:
            loss_fn = self.loss_fn or (mz_loss.stochastic_loss_fn if self.trains_stochastic else mz_loss.default_loss_fn)
            loss = loss_fn(self, batch, *args, **kwargs)
            loss.backward()
            if dp_mean:
                sharding.allreduce_mean_flat([p.grad for p in self._all_params()])
            route = "torch"
        self._last_update_route = route
        self._optimizer.step()
        self._weights_version += 1
        return {"loss": float(loss.item())}

    def _all_params(self):
        return [p for m in self.network if isinstance(m, torch.nn.Module) for p in m.parameters()]

    def _bind_optimizer(self):
        """The optimiser (the default one when none was given) bound to the parameters, on the first update()."""
        from . import optimizers as mz_opt
        if self._optimizer is None:
            self._optimizer = mz_opt.create_optimizer()
        loaded = self._loaded_opt_state
        self._opt_state = self._optimizer.init(self._all_params())
        if loaded is not None:
            # a checkpoint was loaded before the optimiser was bound to parameters: resume its moments,
            # step counts and schedule position (the reference restores opt_state, muax/model.py:210-212)
            self._optimizer.load_state_dict(loaded)
            self._loaded_opt_state = None

    def _fused_update(self, args, kwargs):
        """The fused training step that may serve this update(), or None: (the attribute that keeps the step object, its
        class, the route's name, what builds a missing instance on demand -- a function of the step object, or None --, its
        keywords beyond divide_by_length and sample_weight).  At most one: is_default_mlp_trio wants an MZNetwork of three modules, is_default_stochastic_mlp
        an SMZNetwork of six, so the two families' conditions never hold together.  The stochastic family is served only
        with `stochastic_fused_update`, under its own loss and that loss's keywords; with `stochastic_train_on_demand`
        on top it builds missing instances and takes observations up to 128 wide instead of 32."""
        if self.loss_fn is not None or self.device.type != "cuda":
            return None
        if mz_nn.is_default_mlp_trio(self.network):
            if (self.repr_func.obs_dim or 999) <= 128 and not kwargs.get("pi_all_pairs", False):
                return "_fused_train", mz_loss.FusedLossGrad, "hip_fused", _trio_train_on_demand, _NO_KEYWORDS
        elif self.stochastic_fused_update and mz_nn.is_default_stochastic_mlp(self.network):
            on_demand = _stochastic_train_on_demand if self.stochastic_train_on_demand else None
            if (self.repr_func.obs_dim or 999) <= (128 if on_demand else 32) and not args \
                    and set(kwargs) <= {"vqvae_beta", "divide_by_length", "sample_weight"}:
                return ("_fused_stoch_train", mz_loss.StochasticFusedLossGrad, "hip_stochastic_fused", on_demand,
                        {"vqvae_beta": kwargs.get("vqvae_beta", 0.25)})
        return None

    @property
    def trains_stochastic(self):
        """Whether update() trains with loss.stochastic_loss_fn (an SMZNetwork): its batches then need an observation
        for every step of a window, `DeviceReplayBuffer.sample(all_obs=True)`."""
        return self._stochastic

    @property
    def unrolls_stochastic(self):
        """Whether unroll_values() unrolls this model's SMZNetwork (made with `stochastic_unroll_values=True`): what
        `fit_vector(priority_update=True, priority_steps=)` asks of a model that trains stochastically."""
        return self._stochastic and self.stochastic_unroll_values

    def unroll_values(self, batch, k_prio=None, backend: str = "auto"):
        """The forward unroll of a sampled batch with the CURRENT network: `(values, priorities)`, both [B, kp] float32
        on the model's device, with v_i = value(s_i), s_0 = repr(obs[:, 0]), s_{i+1} = dynamics(s_i, a[:, i]) and
        priorities = |v_i - Rn[:, i]| -- what `DeviceReplayBuffer.update_priorities` takes for the first `kp` steps of
        every window.  `k_prio` defaults to the window length L and must be in 1..L.  backend "hip": ONE launch
        (mzs_mlp_unroll_values, muax_amd/csrc/mz_unroll.cuh) for the default MLP trio on a GPU, obs_dim 1..128,
        embedding 1..64, 1..64 actions, support_size 8..31; values then have the bits of act()'s root value.  "torch": the
        model's modules under no_grad, any nets, any device.  "auto": the kernel where it applies, else torch.  No
        synchronisation either way.
        An SMZNetwork raises NotImplementedError unless the model was made with `stochastic_unroll_values=True`
        (`unrolls_stochastic`).  Then s_{i+1} = the next state of chance_dynamic(afterstate_dynamic(s_i, a[:, i]), c_{i+1})
        with c_{i+1} the encoder's argmax code of obs[:, i + 1], so `batch.obs` must be [B, L, obs_dim], an observation
        for every step (a ValueError otherwise).  "hip": ONE launch (mzs_stochastic_mlp_unroll_values, mz_unroll.cuh) for
        the default stochastic MLP family on a GPU, obs_dim 1..128, embedding 1..64, actions + chance outcomes up to 64,
        support_size 8..31; "torch" and "auto" as above."""
        if backend not in ("auto", "hip", "torch"):
            raise ValueError(f"backend must be 'auto', 'hip' or 'torch', got {backend!r}")
        if self._params is None:
            raise ValueError("call init() first")
        if self._stochastic and not self.stochastic_unroll_values:
            raise NotImplementedError("unroll_values is not built for an SMZNetwork (its unroll needs every step's chance code)")
        B, L, kp = mz_unroll.batch_window(batch, k_prio)
        if self._stochastic:
            mz_loss.check_every_observation(tuple(np.shape(batch.obs)), B, L, "unroll")  # (before anything runs)
        family = mz_unroll.STOCHASTIC if self._stochastic else mz_unroll.TRIO
        served = self.device.type == "cuda" and family.is_family(self.network)
        if backend == "hip" and not served:
            raise ValueError(f"backend='hip' needs {family.name} on a GPU")
        if backend == "torch" or not served or (backend == "auto" and not mz_unroll.within(family, self)):
            return family.torch_unroll(self, batch, kp)
        if self._fused_unroll is None:
            self._fused_unroll = family.fused(self)
        return self._fused_unroll(batch, kp)  # (backend="hip" beyond the limits: the library's error, the limit named)

    def save_load(self, file, save=True):
        """muax/model.py:203-212, on torch state dicts (the reference pickles haiku params)."""
        if self._stochastic:
            raise NotImplementedError("checkpoints of an SMZNetwork are not built: save its six modules' state_dict()s "
                                      "(model.network) and the optimiser state yourself")
        mods = {n: m for n, m in zip(("representation", "prediction", "dynamic"), self.network)
                if isinstance(m, torch.nn.Module)}
        if save:
            torch.save({"params": {n: m.state_dict() for n, m in mods.items()}, "optimizer_state": self._opt_state},
                       file)
        elif str(file).endswith(".npy") or (not os.path.exists(file) and os.path.exists(f"{file}.npy")):
            # a checkpoint written by the reference (jnp.save of haiku params): best-effort reader, no jax needed
            from .checkpoint import load_reference_params
            load_reference_params(self, str(file))
        else:
            saved = torch.load(file, map_location=self.device)
            for n, m in mods.items():
                m.load_state_dict(saved["params"][n])
            st = saved.get("optimizer_state")
            self._opt_state = st
            if st is not None:
                if self._optimizer is not None and self._optimizer.opt is not None:
                    self._optimizer.load_state_dict(st)
                else:
                    self._loaded_opt_state = st  # applied when update() binds the optimiser
            self._weights_version += 1

    def save(self, file):
        """muax/model.py `save`: parameters + optimiser state to `file`."""
        self.save_load(file, save=True)

    def load(self, file):
        self.save_load(file, save=False)
