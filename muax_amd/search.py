"""Host side of the HIP search: torch tensors in, C-ABI calls out.

Counterpart of what ``muax.MuZero._plan`` hands to ``mctx.muzero_policy``
(reference muax/model.py:222-243, muax/policy.py:13-30).  PyTorch is used for
device memory and streams only; all search arithmetic runs in
``libmzsearch.so`` (hand-written gfx950 kernels).  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._call import capture, device_index, raw_stream
from ._lib import (MLP_WEIGHT_NAMES, TREE_FIELDS, TREE_INT_FIELDS, MzsActArgs, MzsActHostArgs, MzsConfig,
                   MzsMlpWeights, MzsStochasticMlpWeights, MzsStochasticOutputs, MzsStochasticSearchArgs, MzsTreeView,
                   STOCHASTIC_MLP_WEIGHT_NAMES, STOCHASTIC_OUTPUT_FIELDS)


class SearchTree(NamedTuple):
    """mctx.Tree arrays ([B,N], [B,N,A], [B,N,E]) as torch tensors."""
    node_visits: torch.Tensor
    raw_values: torch.Tensor
    node_values: torch.Tensor
    parents: torch.Tensor
    action_from_parent: torch.Tensor
    children_index: torch.Tensor
    children_prior_logits: torch.Tensor
    children_values: torch.Tensor
    children_visits: torch.Tensor
    children_rewards: torch.Tensor
    children_discounts: torch.Tensor
    embeddings: torch.Tensor


class PolicyOutput(NamedTuple):
    """mctx.PolicyOutput (action, action_weights, search_tree)."""
    action: torch.Tensor
    action_weights: torch.Tensor
    search_tree: Optional[SearchTree]


class DecisionRecurrentFnOutput(NamedTuple):
    """mctx.DecisionRecurrentFnOutput: what the decision function says of the afterstate of (state, action)."""
    chance_logits: torch.Tensor      # [B, C]
    afterstate_value: torch.Tensor   # [B]


class ChanceRecurrentFnOutput(NamedTuple):
    """mctx.ChanceRecurrentFnOutput: what the chance function says of the state after (afterstate, chance outcome)."""
    action_logits: torch.Tensor      # [B, A]
    value: torch.Tensor              # [B]
    reward: torch.Tensor             # [B]
    discount: torch.Tensor           # [B]


@dataclass
class SearchConfig:
    """Keyword arguments of MuZero.act that reach mctx.muzero_policy (muax/model.py:86-95)."""
    num_actions: int
    num_simulations: int
    embed_dim: int
    max_depth: Optional[int] = None
    tiebreak: bool = True          # mctx adds 1e-7*uniform tie-break noise at every selection
    pb_c_init: float = 1.25
    pb_c_base: float = 19652.0
    global_batch: Optional[int] = None
    root_offset: int = 0
    policy: str = "muzero"         # "muzero" (muax/policy.py:13-30), "gumbel" (:33-47) or "stochastic" (:50-67)
    qtransform: str = "qtransform_by_parent_and_siblings"   # or "qtransform_completed_by_mix_value" (gumbel)
    max_num_considered_actions: int = 16
    gumbel_scale: float = 1.0
    # policy "stochastic": C chance outcomes (num_actions + C <= 64) and the widths of the state and the afterstate
    # embedding (None: embed_dim); embed_dim is the larger of the two
    num_chance_outcomes: int = 0
    state_embed_dim: Optional[int] = None
    afterstate_embed_dim: Optional[int] = None


_NO_ACT_CACHE = bool(__import__("os").environ.get("MUAX_AMD_NO_ACT_CACHE"))  # A/B switch of act_mlp's argument cache


def key_words(key) -> tuple:
    """Accept an int seed, a uint32[2] array/tensor (JAX PRNGKey data) or a (hi, lo) tuple."""
    if isinstance(key, (int, np.integer)):
        k = int(key)
        return ((k >> 32) & 0xFFFFFFFF, k & 0xFFFFFFFF)  # jax.random.PRNGKey(seed)
    if isinstance(key, torch.Tensor):
        key = key.detach().cpu().numpy()
    a = np.asarray(key).astype(np.uint64).ravel()
    if a.size != 2:
        raise ValueError("rng_key must be an int seed or two uint32 words")
    return (int(a[0]) & 0xFFFFFFFF, int(a[1]) & 0xFFFFFFFF)


def fn_identity(fn):
    """Hashable identity of a callable that survives bound-method re-creation."""
    return (getattr(fn, "__func__", fn), id(getattr(fn, "__self__", None)))


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def wide_plan(num_actions: int, embed_dim: int, support_size: int, num_simulations: int, policy: str = "muzero"):
    """The wide-action kernel's LDS plan for a shape (mzs_mlp_wide_plan_policy; host arithmetic, no device needed): a
    dict of `waves` (roots per workgroup), `lds_bytes` (per workgroup), `roots_per_cu` and `emb_lds` (embeddings in LDS),
    or None when the kernel declines the shape (outside 17..64 actions, support_size outside 8..31, more than 255
    simulations, or one root's tree beyond a CU's 160 KiB).  `policy` "gumbel": the plan of the Gumbel modes, whose
    record holds a fifth field per action (the prior logits)."""
    try:
        pol = {"muzero": 0, "gumbel": 1}[policy]
    except KeyError:
        raise ValueError(f"unknown policy: {policy!r}") from None
    out = (C.c_int32 * 4)()
    if _lib.load().mzs_mlp_wide_plan_policy(num_actions, embed_dim, support_size, num_simulations, pol, C.byref(out)) != 0:
        return None
    return dict(waves=out[0], lds_bytes=out[1], roots_per_cu=out[2], emb_lds=bool(out[3]))


def stochastic_plan(num_actions: int, num_chance_outcomes: int, embed_dim: int, support_size: int, num_simulations: int):
    """The one-launch stochastic search's LDS plan for a shape (mzs_mlp_stochastic_plan; host arithmetic, no device
    needed): the dict of `wide_plan`, or None when the kernel declines the shape (num_actions + num_chance_outcomes > 64,
    embed_dim > 64, support_size outside 8..31, more than 255 simulations, or one root's tree beyond a CU's 160 KiB)."""
    out = (C.c_int32 * 4)()
    if _lib.load().mzs_mlp_stochastic_plan(num_actions, num_chance_outcomes, embed_dim, support_size, num_simulations,
                                           C.byref(out)) != 0:
        return None
    return dict(waves=out[0], lds_bytes=out[1], roots_per_cu=out[2], emb_lds=bool(out[3]))


class MuZeroSearch:
    """One handle = one (device, batch shard, search configuration).

    Output aliasing: `action`, `action_weights`, `root_value`, `search_value`, `depth_sum` (and the tensors of an
    exported tree) are PERSISTENT buffers of the handle -- act_mlp() / finish() return views of them and the next
    call on the same handle overwrites them in stream order (select() also stages its actions in `action`).
    Clone what must outlive the next call (MuZero.act(device_outputs=True) does)."""

    def __init__(self, batch: int, cfg: SearchConfig, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("muax_amd needs a ROCm GPU (gfx950); there is no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None \
            else torch.device(device)
        self._dev_index = device_index(self.device)
        self.batch, self.cfg = int(batch), cfg
        self._L = _lib.load()
        try:
            policy = {"muzero": 0, "gumbel": 1, "stochastic": 2}[cfg.policy]
            qtransform = {"qtransform_by_parent_and_siblings": 0, "qtransform_completed_by_mix_value": 1}[
                getattr(cfg.qtransform, "__name__", cfg.qtransform)]
        except KeyError as e:
            raise ValueError(f"unknown policy / qtransform: {e}") from None
        self._stochastic = cfg.policy == "stochastic"
        self._es, self._ea = cfg.state_embed_dim or cfg.embed_dim, cfg.afterstate_embed_dim or cfg.embed_dim
        chance = {}
        if self._stochastic:
            chance = dict(num_chance_outcomes=cfg.num_chance_outcomes, state_embed_dim=self._es, afterstate_embed_dim=self._ea)
        elif cfg.num_chance_outcomes:
            raise ValueError("num_chance_outcomes is for policy='stochastic'")
        c = _lib.args(MzsConfig, device=self._dev_index, batch=self.batch, num_actions=cfg.num_actions,
                      num_simulations=cfg.num_simulations, embed_dim=cfg.embed_dim, max_depth=cfg.max_depth or 0,
                      policy=policy, qtransform=qtransform, tiebreak=int(bool(cfg.tiebreak)),
                      max_num_considered_actions=cfg.max_num_considered_actions, gumbel_scale=cfg.gumbel_scale,
                      pb_c_init=cfg.pb_c_init, pb_c_base=cfg.pb_c_base, global_batch=cfg.global_batch or self.batch,
                      root_offset=cfg.root_offset, **chance)
        self._slots = cfg.num_actions + (cfg.num_chance_outcomes if self._stochastic else 0)  # children per node
        h = C.c_void_p()
        _lib.check(self._L.mzs_create(C.byref(c), C.byref(h)))
        self._h = h
        self._weights = None
        self._stochastic_weights = self._stochastic_out = None  # set_stochastic_mlp_weights; its recurrent step's outputs
        self._stochastic_repr = self._stochastic_root = None  # set_stochastic_representation; stochastic_mlp_root's outputs
        self._root_noise = self.root_noise = None  # search_stochastic_mlp(draw_dirichlet=): the handle's buffer; the last call's rows
        B, A = self.batch, cfg.num_actions
        with torch.cuda.device(self.device):
            # action | action_weights | root_value in ONE allocation: a NumPy caller gets them with one copy
            self._out = torch.empty(B * (2 + A), dtype=torch.float32, device=self.device)
            self.action = self._out[:B].view(torch.int32)
            self.action_weights = self._out[B:B + B * A].view(B, A)
            self.root_value = self._out[B + B * A:]
            self.search_value = torch.empty(B, dtype=torch.float32, device=self.device)
            self.depth_sum = torch.empty(B, dtype=torch.int32, device=self.device)
            # select_stochastic: 1 where the selected edge leaves a decision node
            self.parent_is_decision = torch.empty(B, dtype=torch.int32, device=self.device)
        self._out_host = None   # pinned mirror of _out (outputs_to_host)
        self._obs_stage = None  # (pinned host [B, obs_dim], its NumPy view, device twin, copy-done event)
        self._tree = None
        self._parent_emb = None
        self._graphs = {}  # (recurrent_fn) -> captured simulation loop
        self._act_cache = None  # act_mlp: (argument signature, filled MzsActArgs, tree, kept tensors, noise given)

    def close(self):
        if getattr(self, "_h", None):
            self._L.mzs_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    def _stream(self):
        return raw_stream(self._dev_index)  # torch's current stream of this device, raw

    def _f32(self, t, shape, name):
        if t is None:
            return None
        t = torch.as_tensor(t, device=self.device)
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t.to(torch.float32).contiguous()

    def _u8(self, t, shape, name):
        if t is None:
            return None
        t = torch.as_tensor(t, device=self.device)
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return (t != 0).to(torch.uint8).contiguous()

    def _alloc_tree(self) -> SearchTree:
        if self._tree is None:
            B, N = self.batch, self.cfg.num_simulations + 1
            A, E = self._slots, self.cfg.embed_dim
            shapes = {"embeddings": (B, N, E)}
            out = {}
            for f in TREE_FIELDS:
                shp = shapes.get(f, (B, N, A) if f.startswith("children_") else (B, N))
                dt = torch.int32 if f in TREE_INT_FIELDS else torch.float32
                out[f] = torch.empty(shp, dtype=dt, device=self.device)
            self._tree = SearchTree(**out)
        return self._tree

    def _tree_view(self, tree: SearchTree) -> MzsTreeView:
        return MzsTreeView(**{f: getattr(tree, f).data_ptr() for f in TREE_FIELDS})

    def _export_tree(self) -> SearchTree:
        """The finished tree of the handle copied into its persistent tree tensors (mzs_tree_export)."""
        tree = self._alloc_tree()
        view = self._tree_view(tree)
        _lib.check(self._L.mzs_tree_export(self._h, C.byref(view), self._stream()), self._h)
        return tree

    def outputs_to_host(self):
        """(action int32 [B], action_weights f32 [B, A], root_value f32 [B]) as fresh NumPy arrays: ONE
        device-to-host copy into pinned memory and one stream synchronisation (the reference's np.asarray /
        .item() sync, muax/model.py:173-174)."""
        B, A = self.batch, self.cfg.num_actions
        if self._out_host is None:
            self._out_host = torch.empty(B * (2 + A), dtype=torch.float32).pin_memory()
            self._out_host_np = self._out_host.numpy()
        self._out_host.copy_(self._out, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        h = self._out_host_np
        return h[:B].view(np.int32).copy(), h[B:B + B * A].reshape(B, A).copy(), h[B + B * A:].copy()

    def outputs_clone(self):
        """(action, action_weights, root_value) of the last fused act() as views of ONE fresh device buffer: a single
        stream-ordered copy (the handle's own buffers are overwritten by the next act())."""
        B, A = self.batch, self.cfg.num_actions
        c = self._out.clone()
        return c[:B].view(torch.int32), c[B:B + B * A].view(B, A), c[B + B * A:]

    def _stage_obs(self, obs, obs_dim):
        """Host observations (NumPy / CPU tensor) -> device through a pinned staging buffer, asynchronously."""
        B = self.batch
        if isinstance(obs, torch.Tensor):
            if obs.is_cuda:
                return self._f32(obs, (B, obs_dim), "obs")
            obs = obs.detach().numpy()
        obs = np.asarray(obs)
        if obs.shape != (B, obs_dim):
            raise ValueError(f"obs: expected shape {(B, obs_dim)}, got {obs.shape}")
        if self._obs_stage is None or self._obs_stage[0].shape[1] != obs_dim:
            host = torch.empty(B, obs_dim, dtype=torch.float32).pin_memory()
            self._obs_stage = (host, host.numpy(), torch.empty(B, obs_dim, dtype=torch.float32, device=self.device),
                               torch.cuda.Event())
        host, host_np, dev, ev = self._obs_stage
        ev.synchronize()  # the previous upload has left the staging buffer (no-op when it has, or never ran)
        np.copyto(host_np, obs, casting="same_kind")
        with torch.cuda.device(self.device):
            dev.copy_(host, non_blocking=True)
            ev.record(torch.cuda.current_stream(self.device))
        return dev

    # ------------------------------------------------------------------ fused path
    def set_mlp_weights(self, weights: dict, obs_dim: int, support_size: int = 10,
                        discount: float = 0.99, recurrent_pred_on: str = "child"):
        """Weights of the default MLP trio (muax/nn.py:59-115), haiku layout w[in][out]."""
        A, E = self.cfg.num_actions, self.cfg.embed_dim
        F, H = 2 * support_size + 1, 16
        shapes = {"repr_w": (obs_dim, E), "repr_b": (E,),
                  "pv_w1": (E, H), "pv_b1": (H,), "pv_w2": (H, F), "pv_b2": (F,),
                  "pp_w1": (E, H), "pp_b1": (H,), "pp_w2": (H, A), "pp_b2": (A,),
                  "dr_w1": (E + A, H), "dr_b1": (H,), "dr_w2": (H, F), "dr_b2": (F,),
                  "dn_w1": (E + A, H), "dn_b1": (H,), "dn_w2": (H, E), "dn_b2": (E,)}
        keep = {n: self._f32(weights[n], shapes[n], n) for n in MLP_WEIGHT_NAMES}
        w = _lib.args(MzsMlpWeights, obs_dim=obs_dim, support_size=support_size, discount=discount,
                      recurrent_pred_on={"child": 0, "parent": 1}[recurrent_pred_on],
                      **{n: keep[n].data_ptr() for n in MLP_WEIGHT_NAMES})
        _lib.check(self._L.mzs_mlp_set_weights(self._h, C.byref(w)), self._h)
        self._weights = (keep, obs_dim)  # keep the device buffers alive

    def allow_generic(self, allow: bool = True):
        """Let act_mlp / act_mlp_host serve default-trio shapes without a fused-kernel instance through the library's
        generic one-launch search (mzs_mlp_allow_generic) instead of raising "no fused kernel instance"."""
        _lib.check(self._L.mzs_mlp_allow_generic(self._h, int(bool(allow))), self._h)

    def allow_wide(self, allow: bool = True, gumbel: bool = False):
        """Let act_mlp / act_mlp_host serve 17..64 actions under the MuZero policy through the wide-action one-launch
        kernel (mzs_mlp_allow_wide: one root per wavefront, one lane per action, tree in LDS).  Tried after the fused
        instances and before the generic route; a shape it declines (Gumbel policy, a root that does not fit the LDS:
        `wide_plan`) goes on to the generic route if that is allowed, else raises "no fused kernel instance".
        `gumbel=True` sets the switch of the Gumbel policy instead (mzs_mlp_allow_wide_gumbel; the two are separate: a
        Gumbel handle is served by the wide kernel only after allow_wide(gumbel=True), plan `wide_plan(..., policy="gumbel")`)."""
        fn = self._L.mzs_mlp_allow_wide_gumbel if gumbel else self._L.mzs_mlp_allow_wide
        _lib.check(fn(self._h, int(bool(allow))), self._h)

    def act_mlp(self, obs, key, dirichlet_noise=None, dirichlet_fraction: float = 0.25,
                invalid_actions=None, temperature: float = 1.0, gumbel=None,
                with_tree: bool = False) -> PolicyOutput:
        """Whole act(): root inference, S simulations, summary and sampling -- ONE kernel launch.
        Outputs live in self.action / action_weights / root_value / search_value / depth_sum."""
        if self._weights is None:
            raise ValueError("set_mlp_weights() first")
        B, A = self.batch, self.cfg.num_actions
        # An RL loop calls act() with the same device buffers step after step: when every tensor argument is the very
        # object (and storage) of the previous call, the checked / converted inputs and the filled argument block are
        # reused and only the key and the scalars are written (~8 us of host time per act otherwise, on the critical
        # path of a synchronised act: the GPU idles while the host prepares the launch).
        sig = (id(obs), id(dirichlet_noise), id(invalid_actions), id(gumbel), bool(with_tree),
               tuple(t.data_ptr() if isinstance(t, torch.Tensor) else None for t in (obs, dirichlet_noise, invalid_actions, gumbel)))
        fast = self._act_cache if (self._act_cache is not None and self._act_cache[0] == sig and not _NO_ACT_CACHE
                                   and isinstance(obs, torch.Tensor) and obs.is_cuda) else None
        if fast is not None:
            _, a, tree, keep, has_noise = fast
        else:
            obs_t = self._stage_obs(obs, self._weights[1])
            noise = self._f32(dirichlet_noise, (B, A), "dirichlet_noise")
            inv = self._u8(invalid_actions, (B, A), "invalid_actions")
            gum = self._f32(gumbel, (B, A), "gumbel")
            a = _lib.args(MzsActArgs, obs=obs_t.data_ptr(), dirichlet_noise=_ptr(noise), invalid_actions=_ptr(inv),
                          gumbel=_ptr(gum), action=self.action.data_ptr(), action_weights=self.action_weights.data_ptr(),
                          root_value=self.root_value.data_ptr(), search_value=self.search_value.data_ptr(),
                          depth_sum=self.depth_sum.data_ptr())
            tree = None
            if with_tree:
                tree = self._alloc_tree()
                view = self._tree_view(tree)
                a.tree = C.pointer(view)
            keep = (obs_t, noise, inv, gum, obs, dirichlet_noise, invalid_actions, gumbel, view if with_tree else None)  # (ids stay unique while held)
            has_noise = noise is not None
            # cached only when the kernel reads the caller's own storage (a converted copy would go stale under an
            # in-place update of the original)
            same = all(x is None or (isinstance(y, torch.Tensor) and x.data_ptr() == y.data_ptr())
                       for x, y in ((obs_t, obs), (noise, dirichlet_noise), (inv, invalid_actions), (gum, gumbel)))
            self._act_cache = (sig, a, tree, keep, has_noise) if same else None
        k = key_words(key)
        a.key[0], a.key[1] = k
        a.dirichlet_fraction = dirichlet_fraction if has_noise else 0.0
        a.temperature = temperature
        _lib.check(self._L.mzs_act_mlp(self._h, C.byref(a), self._stream()), self._h)
        self._keep = keep  # alive until the stream has consumed them
        return PolicyOutput(self.action, self.action_weights, tree)

    def act_mlp_host(self, obs: np.ndarray, key, dirichlet_noise=None, dirichlet_fraction: float = 0.25,
                     dirichlet_alpha: float = 0.3, invalid_actions=None, temperature: float = 1.0):
        """The reference's act() round trip in ONE C call (mzs_act_mlp_host): NumPy observations in, (action int32
        [B], action_weights f32 [B, A], root_value f32 [B]) NumPy out, synchronised.  Root noise: `dirichlet_noise`
        if given, else drawn on the device from split(key, 3)[1] (muzero policy, dirichlet_fraction != 0)."""
        if self._weights is None:
            raise ValueError("set_mlp_weights() first")
        B, A, od = self.batch, self.cfg.num_actions, self._weights[1]
        obs = np.ascontiguousarray(obs, np.float32)
        if obs.shape != (B, od):
            raise ValueError(f"obs: expected shape {(B, od)}, got {obs.shape}")
        nz = iv = None  # (the converted arrays stay alive until the call has returned)
        if dirichlet_noise is not None:
            nz = np.ascontiguousarray(dirichlet_noise, np.float32)
            if nz.shape != (B, A):
                raise ValueError(f"dirichlet_noise: expected shape {(B, A)}, got {nz.shape}")
        if invalid_actions is not None:
            iv = np.ascontiguousarray(np.asarray(invalid_actions) != 0, np.uint8)
            if iv.shape != (B, A):
                raise ValueError(f"invalid_actions: expected shape {(B, A)}, got {iv.shape}")
        action = np.empty(B, np.int32)
        weights = np.empty((B, A), np.float32)
        value = np.empty(B, np.float32)
        a = _lib.args(MzsActHostArgs, draw_dirichlet=1, obs=obs.ctypes.data,
                      dirichlet_noise=None if nz is None else nz.ctypes.data,
                      invalid_actions=None if iv is None else iv.ctypes.data, key=key_words(key),
                      dirichlet_fraction=dirichlet_fraction, dirichlet_alpha=dirichlet_alpha, temperature=temperature,
                      action=action.ctypes.data, action_weights=weights.ctypes.data, root_value=value.ctypes.data)
        _lib.check(self._L.mzs_act_mlp_host(self._h, C.byref(a), self._stream()), self._h)
        return action, weights, value

    # ------------------------------------------------------------------ step-wise path
    def _parent_embedding(self):
        """The persistent [B, embed_dim] buffer the selections hand out, allocated on first use."""
        if self._parent_emb is None:
            self._parent_emb = torch.empty(self.batch, self.cfg.embed_dim, dtype=torch.float32, device=self.device)
        return self._parent_emb

    def _root(self, entry, prior_logits, value, embedding, width, key, invalid_actions, noise, noise_name, fraction=None):
        """RootFnOutput (embedding: [B, width]) + the policy's [B, A] noise -> `entry`; fraction: the Dirichlet roots'."""
        B, A = self.batch, self.cfg.num_actions
        pl = self._f32(prior_logits, (B, A), "prior_logits")
        v = self._f32(value, (B,), "value")
        emb = self._f32(torch.as_tensor(embedding, device=self.device).reshape(B, -1), (B, width), "embedding")
        inv = self._u8(invalid_actions, (B, A), "invalid_actions")
        nz = self._f32(noise, (B, A), noise_name)
        tail = () if fraction is None else (C.c_float(fraction if nz is not None else 0.0),)
        kw = (C.c_uint32 * 2)(*key_words(key))
        _lib.check(entry(self._h, _ptr(pl), _ptr(v), _ptr(emb), _ptr(inv), _ptr(nz), *tail, C.byref(kw), self._stream()),
                   self._h)
        self._keep = (pl, v, emb, inv, nz)
        self._parent_embedding()

    def root(self, prior_logits, value, embedding, key=0, invalid_actions=None,
             dirichlet_noise=None, dirichlet_fraction: float = 0.25):
        """RootFnOutput -> tree (mctx muzero_policy prelude + instantiate_tree_from_root)."""
        self._root(self._L.mzs_root, prior_logits, value, embedding, self.cfg.embed_dim, key, invalid_actions,
                   dirichlet_noise, "dirichlet_noise", dirichlet_fraction)

    def root_gumbel(self, prior_logits, value, embedding, key=0, invalid_actions=None, gumbel=None):
        """Gumbel MuZero root (mctx gumbel_muzero_policy prelude): invalid-action mask only, root Gumbel
        noise drawn from the key (or injected)."""
        self._root(self._L.mzs_root_gumbel, prior_logits, value, embedding, self.cfg.embed_dim, key, invalid_actions,
                   gumbel, "gumbel")

    def select(self, sim: int):
        """One mctx simulate(): returns (action [B] int32, parent embedding [B,E])."""
        if self._parent_emb is None:
            raise ValueError("root() first")
        _lib.check(self._L.mzs_select(self._h, sim, _ptr(self.action), _ptr(self._parent_emb),
                                      self._stream()), self._h)
        return self.action, self._parent_emb

    def _recurrent_outputs(self, reward, discount, prior_logits, value, next_embedding):
        """RecurrentFnOutput + next embedding as the checked float32 tensors the expansion entries read."""
        B, A, E = self.batch, self.cfg.num_actions, self.cfg.embed_dim
        return (self._f32(reward, (B,), "reward"), self._f32(discount, (B,), "discount"),
                self._f32(prior_logits, (B, A), "prior_logits"), self._f32(value, (B,), "value"),
                self._f32(torch.as_tensor(next_embedding, device=self.device).reshape(B, -1), (B, E), "next_embedding"))

    def expand_backup(self, sim: int, reward, discount, prior_logits, value, next_embedding):
        """RecurrentFnOutput + next embedding -> expand + backward."""
        keep = self._recurrent_outputs(reward, discount, prior_logits, value, next_embedding)
        _lib.check(self._L.mzs_expand_backup(self._h, sim, *map(_ptr, keep), self._stream()), self._h)
        self._keep = keep

    def expand_backup_select(self, sim: int, reward, discount, prior_logits, value, next_embedding):
        """expand_backup(sim) and select(sim + 1) in ONE launch (mzs_expand_backup_select): returns the next
        simulation's (action, parent embedding) -- the same persistent buffers select() hands out -- or None after
        the last simulation."""
        if self._parent_emb is None:
            raise ValueError("root() first")
        r, d, pl, v, ne = self._recurrent_outputs(reward, discount, prior_logits, value, next_embedding)
        pe = self._parent_emb
        if ne.untyped_storage().data_ptr() == pe.untyped_storage().data_ptr():
            # an identity (or slicing / offset-view) recurrent_fn: the launch's tail overwrites the buffer select()
            # handed out while the expansion still reads `ne` -- any view of that storage is copied first
            ne = ne.clone()
        _lib.check(self._L.mzs_expand_backup_select(self._h, sim, _ptr(r), _ptr(d), _ptr(pl), _ptr(v), _ptr(ne),
                                                    _ptr(self.action), _ptr(self._parent_emb), self._stream()),
                   self._h)
        self._keep = (r, d, pl, v, ne)
        return (self.action, self._parent_emb) if sim + 1 < self.cfg.num_simulations else None

    def _finish(self, entry, temperature, gumbel, with_tree) -> PolicyOutput:
        B, A = self.batch, self.cfg.num_actions
        gum = self._f32(gumbel, (B, A), "gumbel")
        _lib.check(entry(self._h, C.c_float(temperature), _ptr(gum), _ptr(self.action), _ptr(self.action_weights),
                         _ptr(self.search_value), _ptr(self.depth_sum), self._stream()), self._h)
        self._keep = (gum,)
        return PolicyOutput(self.action, self.action_weights, self._export_tree() if with_tree else None)

    def finish(self, temperature: float = 1.0, gumbel=None, with_tree: bool = False) -> PolicyOutput:
        return self._finish(self._L.mzs_finish, temperature, gumbel, with_tree)

    def _run_loop(self, do_root, loop, graph, gkey, fns, graph_version):
        """The simulation loop of a rooted tree: eager, or (graph) captured once per (gkey, graph_version) and replayed;
        `fns`: the callables the capture froze, kept alive with it."""
        if not graph:
            return loop()
        entry = self._graphs.get(gkey)
        if entry is not None and entry[3] != graph_version:
            entry = None
        if entry is None:
            # warm-up run (lazy library initialisation must not happen under capture), then the tree
            # is rebuilt from the same root and the loop is captured (capture records, it does not run)
            with torch.no_grad():
                side = torch.cuda.Stream(device=self.device)
                side.wait_stream(torch.cuda.current_stream(self.device))
                with torch.cuda.stream(side):
                    loop()
                torch.cuda.current_stream(self.device).wait_stream(side)
                do_root()
                g = torch.cuda.CUDAGraph()
                with capture(g):
                    loop()
            entry = self._graphs[gkey] = (g, fns, self._keep, graph_version)
        entry[0].replay()

    def search(self, root_fn_output, recurrent_fn, key=0, invalid_actions=None,
               dirichlet_noise=None, dirichlet_fraction=0.25, temperature=1.0, gumbel=None,
               with_tree=False, graph=False, graph_key=None, graph_version=0, native_loop=None) -> PolicyOutput:
        """mctx.muzero_policy with a caller-supplied recurrent_fn(action, embedding) ->
        (reward, discount, prior_logits, value, next_embedding) of torch tensors.

        graph=True captures the S x (select -> recurrent_fn -> expand_backup) loop into ONE hipGraph
        (torch.cuda.CUDAGraph; our kernels are launched on torch's current stream, so the capture sees
        them) and replays it on later calls: the loop is launch-bound -- two tree kernels plus the
        plugin's own small kernels per simulation -- and a graph launch removes the per-kernel host cost.
        recurrent_fn must then be capture-safe (no host synchronisation, static shapes); the per-call
        PRNG keys live in device memory (root) or in the un-captured root/finish calls.  `graph_version`
        is the caller's weights version: host-side work of recurrent_fn (e.g. re-packing convolution weights)
        is frozen into a capture, so a new version re-captures and replaces the old graph.

        `native_loop(handle, sim_begin, sim_end)`: nets whose recurrent_fn the library evaluates itself (the reference's
        ResNet nets: ResNetDynamic.hip_search -> mzs_resnet_search) run the WHOLE simulation loop as one launch -- every
        root advanced by its own workgroup(s), recurrent_fn and the tree update back to back, no per-simulation launch
        and no row copies; `recurrent_fn` is then only the fall-back (a tree without cached decisions).  Every edge already
        expanded on the handle must carry the same discount as mzs_resnet_search's `discount` argument: the LDS tree
        build does not store per-edge discounts and applies the argument to existing edges, so a tree continued from
        expand_backup[_select] calls with other discounts gives results that depend on MZS_SEARCH_LDS_TREE."""
        prior_logits, value, embedding = root_fn_output

        def do_root():
            if self.cfg.policy == "gumbel":
                self.root_gumbel(prior_logits, value, embedding, key, invalid_actions, gumbel)
            else:
                self.root(prior_logits, value, embedding, key, invalid_actions, dirichlet_noise,
                          dirichlet_fraction)

        def loop():
            # select(0), then S x (recurrent_fn -> expand + backward of sim AND the selection of sim + 1 in one launch)
            nxt = self.select(0)
            for sim in range(self.cfg.num_simulations):
                nxt = self.expand_backup_select(sim, *recurrent_fn(*nxt))

        do_root()
        if native_loop is not None and getattr(self, "_native_loop_unusable", False):
            native_loop = None  # (found out on an earlier call: this handle's tree has no cached decisions)
        if native_loop is not None:
            self.select(0)  # simulate() of simulation 0; every later one is the tail of its predecessor inside the launch
            ev = getattr(self, "time_native_loop", None)  # (start, end) events of a profiler (bench.py), else None
            try:
                if ev:
                    ev[0].record()
                native_loop(self, 0, self.cfg.num_simulations)
                if ev:
                    ev[1].record()
            except _lib.NoCachedDecisions:
                native_loop = None  # (trees beyond the cached-decision budget keep the per-simulation launches)
                self._native_loop_unusable = True
                do_root()  # select(0) above has already counted simulation 0's depth; the fall-back loop starts from the root again
        if native_loop is None:
            gkey = graph_key if graph_key is not None else fn_identity(recurrent_fn)
            self._run_loop(do_root, loop, graph, gkey, recurrent_fn, graph_version)
        return self.finish(temperature, None if self.cfg.policy == "gumbel" else gumbel, with_tree)

    # ------------------------------------------------------------------ step-wise path, stochastic policy
    def root_stochastic(self, prior_logits, value, embedding, key=0, invalid_actions=None, dirichlet_noise=None,
                        dirichlet_fraction: float = 0.25):
        """RootFnOutput -> tree (mctx stochastic_muzero_policy prelude): the MuZero root over the A actions, the chance
        slots padded with -inf / invalid.  embedding: the root's STATE embedding [B, state_embed_dim]."""
        self._root(self._L.mzs_root_stochastic, prior_logits, value, embedding, self._es, key, invalid_actions,
                   dirichlet_noise, "dirichlet_noise", dirichlet_fraction)

    def select_stochastic(self, sim: int):
        """One simulate() over decision and chance nodes: (slot [B] int32 in [0, A + C), parent_is_decision [B] int32,
        parent embedding [B, embed_dim] -- the parent's own kind of embedding, zero-padded)."""
        pe = self._parent_embedding()
        _lib.check(self._L.mzs_select_stochastic(self._h, sim, _ptr(self.action), _ptr(self.parent_is_decision), _ptr(pe),
                                                 self._stream()), self._h)
        return self.action, self.parent_is_decision, pe

    def expand_backup_stochastic(self, sim: int, decision_out, afterstate_embedding, chance_out, state_embedding):
        """Both functions' outputs for every root (DecisionRecurrentFnOutput + afterstate embedding,
        ChanceRecurrentFnOutput + state embedding): the kernel takes, per root, the set of its parent's kind."""
        B, A, Cn = self.batch, self.cfg.num_actions, self.cfg.num_chance_outcomes
        dev = self.device
        keep = (self._f32(decision_out[0], (B, Cn), "chance_logits"), self._f32(decision_out[1], (B,), "afterstate_value"),
                self._f32(torch.as_tensor(afterstate_embedding, device=dev).reshape(B, -1), (B, self._ea), "afterstate_embedding"),
                self._f32(chance_out[0], (B, A), "action_logits"), self._f32(chance_out[1], (B,), "value"),
                self._f32(chance_out[2], (B,), "reward"), self._f32(chance_out[3], (B,), "discount"),
                self._f32(torch.as_tensor(state_embedding, device=dev).reshape(B, -1), (B, self._es), "state_embedding"))
        o = _lib.args(MzsStochasticOutputs, **{n: t.data_ptr() for n, t in zip(STOCHASTIC_OUTPUT_FIELDS, keep)})
        _lib.check(self._L.mzs_expand_backup_stochastic(self._h, sim, C.byref(o), self._stream()), self._h)
        self._keep = keep

    def finish_stochastic(self, temperature: float = 1.0, gumbel=None, with_tree: bool = False) -> PolicyOutput:
        """Summary and sample over the A actions; with_tree: the full tree, children arrays [B, N, A + C]."""
        return self._finish(self._L.mzs_finish_stochastic, temperature, gumbel, with_tree)

    def set_stochastic_mlp_weights(self, weights: dict, support_size: int = 10, discount: float = 0.99):
        """Weights of the default stochastic MLP family (nn.stochastic_mlp_weights: 28 arrays, haiku layout w[in][out]) for
        search_stochastic_mlp.  The handle must run the stochastic policy with both embeddings embed_dim wide."""
        A, Cn, E = self.cfg.num_actions, self.cfg.num_chance_outcomes, self.cfg.embed_dim
        F, H = 2 * support_size + 1, 16
        heads = {"ad": (E + A, E), "av": (E, F), "ac": (E, Cn), "cr": (E + Cn, F), "cn": (E + Cn, E), "pv": (E, F),
                 "pp": (E, A)}
        shapes = {}
        for h, (i, o) in heads.items():
            shapes.update({f"{h}_w1": (i, H), f"{h}_b1": (H,), f"{h}_w2": (H, o), f"{h}_b2": (o,)})
        keep = {n: self._f32(weights[n], shapes[n], n) for n in STOCHASTIC_MLP_WEIGHT_NAMES}
        w = _lib.args(MzsStochasticMlpWeights, support_size=support_size, discount=discount,
                      **{n: keep[n].data_ptr() for n in STOCHASTIC_MLP_WEIGHT_NAMES})
        _lib.check(self._L.mzs_mlp_set_stochastic_weights(self._h, C.byref(w)), self._h)
        self._stochastic_weights = keep  # keep the device buffers alive

    def set_stochastic_representation(self, repr_w, repr_b):
        """The default Representation's weights (nn.stochastic_root_weights: repr_w [obs_dim, embed_dim], repr_b
        [embed_dim], haiku layout) for the library's own root inference: stochastic_mlp_root and
        search_stochastic_mlp(None, obs=...).  obs_dim is repr_w's first dimension."""
        E = self.cfg.embed_dim
        w = torch.as_tensor(repr_w, device=self.device)
        if w.ndim != 2 or w.shape[0] < 1:
            raise ValueError(f"repr_w: expected shape (obs_dim >= 1, {E}), got {tuple(w.shape)}")
        keep = (self._f32(w, (w.shape[0], E), "repr_w"), self._f32(repr_b, (E,), "repr_b"))
        _lib.check(self._L.mzs_mlp_set_stochastic_representation(self._h, int(w.shape[0]), _ptr(keep[0]), _ptr(keep[1])), self._h)
        self._stochastic_repr = keep  # keep the device buffers alive

    def _stochastic_obs(self, obs):
        if self._stochastic_weights is None:
            raise ValueError("set_stochastic_mlp_weights() first")
        if self._stochastic_repr is None:
            raise ValueError("set_stochastic_representation() first")
        return self._f32(obs, (self.batch, self._stochastic_repr[0].shape[0]), "obs")

    def stochastic_mlp_root(self, obs):
        """Root inference of the bound default family on obs [B, obs_dim] in ONE launch (mzs_mlp_stochastic_root), no torch
        module -> (prior_logits [B, A], value [B], embedding [B, embed_dim]): RootFnOutput in persistent buffers of the
        handle (value is `root_value`), overwritten by the next call."""
        obs = self._stochastic_obs(obs)
        if self._stochastic_root is None:
            B, A, E = self.batch, self.cfg.num_actions, self.cfg.embed_dim
            with torch.cuda.device(self.device):
                self._stochastic_root = (torch.empty(B, A, dtype=torch.float32, device=self.device),
                                         torch.empty(B, E, dtype=torch.float32, device=self.device))
        logits, emb = self._stochastic_root
        _lib.check(self._L.mzs_mlp_stochastic_root(self._h, _ptr(obs), _ptr(logits), _ptr(self.root_value), _ptr(emb),
                                                   self._stream()), self._h)
        self._keep = (obs,)
        return logits, self.root_value, emb

    def stochastic_mlp_recurrent(self, slot, parent_is_decision, parent_embedding):
        """The decision or the chance function of the bound default family for every root, by its parent's kind, in ONE
        launch (mzs_mlp_stochastic_recurrent) -> the MzsStochasticOutputs block of the handle's persistent output arrays,
        which expand_backup_stochastic_outputs takes.  Rows of the other kind keep what they held."""
        if self._stochastic_weights is None:
            raise ValueError("set_stochastic_mlp_weights() first")
        if self._stochastic_out is None:
            B, A, Cn, E = self.batch, self.cfg.num_actions, self.cfg.num_chance_outcomes, self.cfg.embed_dim
            with torch.cuda.device(self.device):
                bufs = [torch.zeros(B * n, dtype=torch.float32, device=self.device) for n in (Cn, 1, E, A, 1, 1, 1, E)]
            o = _lib.args(MzsStochasticOutputs, **{n: t.data_ptr() for n, t in zip(STOCHASTIC_OUTPUT_FIELDS, bufs)})
            self._stochastic_out = (o, bufs)
        o = self._stochastic_out[0]
        _lib.check(self._L.mzs_mlp_stochastic_recurrent(self._h, _ptr(slot), _ptr(parent_is_decision), _ptr(parent_embedding),
                                                        C.byref(o), self._stream()), self._h)
        return o

    def expand_backup_stochastic_outputs(self, sim: int, outputs):
        """expand_backup_stochastic on a filled MzsStochasticOutputs block (stochastic_mlp_recurrent's)."""
        _lib.check(self._L.mzs_expand_backup_stochastic(self._h, sim, C.byref(outputs), self._stream()), self._h)

    def _search_stochastic(self, root_fn_output, recurrent_expand, gkey, fns, key, invalid_actions, dirichlet_noise,
                           dirichlet_fraction, temperature, gumbel, with_tree, graph, graph_version) -> PolicyOutput:
        """The stochastic search around `recurrent_expand(sim, slot, parent_is_decision, parent_embedding)`, which evaluates
        the functions and expands: root, S x (select -> recurrent_expand), eager or as one captured graph, finish."""
        prior_logits, value, embedding = root_fn_output

        def do_root():
            self.root_stochastic(prior_logits, value, embedding, key, invalid_actions, dirichlet_noise, dirichlet_fraction)

        def loop():
            for sim in range(self.cfg.num_simulations):
                recurrent_expand(sim, *self.select_stochastic(sim))

        do_root()
        self._run_loop(do_root, loop, graph, gkey, fns, graph_version)
        return self.finish_stochastic(temperature, gumbel, with_tree)

    def _search_stochastic_one_launch(self, root_fn_output, gkey, key, invalid_actions, dirichlet_noise, dirichlet_fraction,
                                      temperature, gumbel, with_tree, graph, graph_version, obs=None, draw=None,
                                      noise_out=None) -> PolicyOutput:
        """The whole search as ONE launch (mzs_mlp_stochastic_search; with `obs` instead of root_fn_output
        mzs_mlp_stochastic_search_obs: root inference inside it, the root's value into `root_value`).  graph: that launch
        captured as a one-node graph per (gkey, which optional inputs are there, with_tree, graph_version) -- the inputs
        then travel through persistent buffers and key, temperature and dirichlet_fraction through the entry's device
        block, so a replay sees this call's values.

        draw: the Dirichlet alpha of a root noise drawn inside the launch (mzs_mlp_stochastic_search_draw; no
        dirichlet_noise then); noise_out: None, True (the handle's own buffer) or the caller's float32 [B, A] tensor for
        the drawn rows, `root_noise` afterwards.  A captured launch of this variant has its own graph, reads alpha from
        the device block too and writes the rows to the handle's buffer (a caller's tensor is filled from it)."""
        B, A, S = self.batch, self.cfg.num_actions, self.cfg.num_simulations
        noise = None
        if draw is not None and noise_out is not None:
            if noise_out is True or graph:
                if self._root_noise is None:
                    with torch.cuda.device(self.device):
                        self._root_noise = torch.empty(B, A, dtype=torch.float32, device=self.device)
                noise = self._root_noise
            if noise_out is not True:
                if not (isinstance(noise_out, torch.Tensor) and noise_out.dtype == torch.float32 and noise_out.is_contiguous()
                        and tuple(noise_out.shape) == (B, A) and noise_out.device == self.action.device):
                    raise ValueError(f"noise_out: expected True or a contiguous float32 tensor of shape {(B, A)} on {self.device}")
                noise = noise if graph else noise_out
        if obs is not None:
            ins = dict(obs=self._stochastic_obs(obs))
        else:
            prior_logits, value, embedding = root_fn_output
            ins = dict(prior_logits=self._f32(prior_logits, (B, A), "prior_logits"), value=self._f32(value, (B,), "value"),
                       embedding=self._f32(torch.as_tensor(embedding, device=self.device).reshape(B, -1), (B, self._es),
                                           "embedding"))
        ins.update(invalid_actions=self._u8(invalid_actions, (B, A), "invalid_actions"),
                   dirichlet_noise=self._f32(dirichlet_noise, (B, A), "dirichlet_noise"),
                   gumbel=self._f32(gumbel, (B, A), "gumbel"))
        fraction = dirichlet_fraction if ins["dirichlet_noise"] is not None or draw is not None else 0.0
        kw = (C.c_uint32 * 2)(*key_words(key))
        words = 4 + 2 * S + (3 if draw is not None else 0)  # the device block of the entry taken

        def launch(tensors, block):
            a = _lib.args(MzsStochasticSearchArgs, export_tree=int(bool(with_tree)), key=tuple(kw), dirichlet_fraction=fraction,
                          temperature=temperature, device_block=None if block is None else block.data_ptr(),
                          action=self.action.data_ptr(), action_weights=self.action_weights.data_ptr(),
                          search_value=self.search_value.data_ptr(), depth_sum=self.depth_sum.data_ptr(),
                          **{n: None if t is None else t.data_ptr() for n, t in tensors.items() if n != "obs"})
            if draw is not None:
                _lib.check(self._L.mzs_mlp_stochastic_search_draw(self._h, C.byref(a), _ptr(tensors.get("obs")),
                                                                  _ptr(self.root_value), draw, _ptr(noise), self._stream()),
                           self._h)
            elif obs is None:
                _lib.check(self._L.mzs_mlp_stochastic_search(self._h, C.byref(a), self._stream()), self._h)
            else:
                _lib.check(self._L.mzs_mlp_stochastic_search_obs(self._h, C.byref(a), _ptr(tensors["obs"]), _ptr(self.root_value),
                                                                 self._stream()), self._h)

        if not graph:
            launch(ins, None)
            self._keep = tuple(ins.values())
        else:
            gk = ((gkey, "one_launch", tuple(t is not None for t in ins.values()), bool(with_tree))
                  + (("obs",) if obs is not None else ()) + (("draw", noise is not None) if draw is not None else ()))
            entry = self._graphs.get(gk)
            if entry is not None and entry[3] != graph_version:
                entry = None
            if entry is None:
                with torch.cuda.device(self.device):
                    bufs = {n: None if t is None else torch.empty_like(t) for n, t in ins.items()}
                    host = torch.empty(words, dtype=torch.int32).pin_memory()
                    block = torch.empty(words, dtype=torch.int32, device=self.device)
                stage = (bufs, host, block, torch.cuda.Event())
            else:
                stage = entry[1]
            bufs, host, block, ev = stage
            for n, t in ins.items():
                if t is not None:
                    bufs[n].copy_(t)
            ev.synchronize()  # the previous upload has left the pinned block (no-op when it has, or never ran)
            if draw is not None:
                _lib.check(self._L.mzs_stochastic_search_block_draw(C.byref(kw), S, temperature, fraction, draw, host.data_ptr()))
            else:
                _lib.check(self._L.mzs_stochastic_search_block(C.byref(kw), S, temperature, fraction, host.data_ptr()))
            with torch.cuda.device(self.device):
                block.copy_(host, non_blocking=True)
                ev.record(torch.cuda.current_stream(self.device))
            if entry is None:
                # warm-up run (the handle's first call may allocate; not under capture), then the capture (it records only)
                side = torch.cuda.Stream(device=self.device)
                side.wait_stream(torch.cuda.current_stream(self.device))
                with torch.cuda.stream(side):
                    launch(bufs, block)
                torch.cuda.current_stream(self.device).wait_stream(side)
                g = torch.cuda.CUDAGraph()
                with capture(g):
                    launch(bufs, block)
                entry = self._graphs[gk] = (g, stage, (self._stochastic_weights, self._stochastic_repr), graph_version)
            entry[0].replay()
            if noise is not None and noise_out is not True:
                noise_out.copy_(noise)
                noise = noise_out
        self.root_noise = noise
        return PolicyOutput(self.action, self.action_weights, self._export_tree() if with_tree else None)

    def search_stochastic_mlp(self, root_fn_output=None, key=0, invalid_actions=None, dirichlet_noise=None, dirichlet_fraction=0.25,
                              temperature=1.0, gumbel=None, with_tree=False, graph=False, graph_key=None,
                              graph_version=0, one_launch=False, obs=None, draw_dirichlet=None, noise_out=None) -> PolicyOutput:
        """search_stochastic with the two callables replaced by the library's own evaluation of the default stochastic MLP
        family (set_stochastic_mlp_weights): three launches per simulation -- select, the function of each root's parent
        kind, expand + backward -- and no torch op.  Arguments as search_stochastic; the kernel reads the bound weight
        arrays at every launch, so a captured loop sees in-place weight updates (a re-bound array: new graph_version).

        one_launch=True: root set-up, every simulation and the finish in ONE launch with the tree in LDS
        (mzs_mlp_stochastic_search) -- the same arguments, the same return value, the same bits; a captured graph is one
        kernel node.  A shape `stochastic_plan` declines is then a ValueError naming the limit.

        `obs` [B, obs_dim] INSTEAD of root_fn_output (pass None for it): root inference by the library as well
        (set_stochastic_representation; embed_dim <= 64) -- inside the one launch with one_launch=True
        (mzs_mlp_stochastic_search_obs), else one more launch in front of the loop (stochastic_mlp_root).  The root's
        network value is then in `root_value`.  graph=True as before: a captured launch reads `obs` from a persistent
        buffer, a replay sees the call's own observations.

        draw_dirichlet=alpha (one_launch=True only, no dirichlet_noise): the root noise is drawn INSIDE that launch
        (mzs_mlp_stochastic_search_draw) -- every root's wavefront draws its row of jax.random.dirichlet(split(key, 3)[1],
        full([A], alpha), (global_batch,)), the bits of model._dirichlet / mzs_dirichlet, and mixes it in with
        dirichlet_fraction: the results are those of passing that array as dirichlet_noise.  noise_out: a float32 [B, A]
        device tensor that receives the drawn rows, or True for a buffer of the handle; either way they are in
        `root_noise` afterwards (None when not asked for).  graph=True: still one kernel node, no noise staged; alpha
        travels through the device block like the key."""
        if (root_fn_output is None) == (obs is None):
            raise ValueError("search_stochastic_mlp takes either root_fn_output or obs=, not both and not neither")
        if draw_dirichlet is not None:
            if not one_launch:
                raise ValueError("draw_dirichlet needs one_launch=True: the noise is drawn inside the one-launch kernel")
            if dirichlet_noise is not None:
                raise ValueError("draw_dirichlet and dirichlet_noise exclude each other: the kernel draws the noise or reads it")
            draw_dirichlet = float(draw_dirichlet)
            if not (0.0 < draw_dirichlet < float("inf")):
                raise ValueError(f"draw_dirichlet: alpha must be positive and finite, got {draw_dirichlet}")
        elif noise_out is not None:
            raise ValueError("noise_out needs draw_dirichlet=alpha")
        if self._stochastic_weights is None:
            raise ValueError("set_stochastic_mlp_weights() first")
        if obs is not None and self._stochastic_repr is None:
            raise ValueError("set_stochastic_representation() first")
        if one_launch:
            return self._search_stochastic_one_launch(root_fn_output, graph_key if graph_key is not None else "stochastic_mlp",
                                                      key, invalid_actions, dirichlet_noise, dirichlet_fraction, temperature,
                                                      gumbel, with_tree, graph, graph_version, obs, draw_dirichlet, noise_out)
        if obs is not None:
            root_fn_output = self.stochastic_mlp_root(obs)

        def recurrent_expand(sim, slot, kind, pemb):
            self.expand_backup_stochastic_outputs(sim, self.stochastic_mlp_recurrent(slot, kind, pemb))

        gkey = graph_key if graph_key is not None else "stochastic_mlp"
        return self._search_stochastic(root_fn_output, recurrent_expand, gkey, self._stochastic_weights, key, invalid_actions,
                                       dirichlet_noise, dirichlet_fraction, temperature, gumbel, with_tree, graph, graph_version)

    def search_stochastic(self, root_fn_output, decision_fn, chance_fn, key=0, invalid_actions=None, dirichlet_noise=None,
                          dirichlet_fraction=0.25, temperature=1.0, gumbel=None, with_tree=False, graph=False,
                          graph_key=None, graph_version=0) -> PolicyOutput:
        """mctx.stochastic_muzero_policy with caller-supplied functions of torch tensors:
        decision_fn(action [B], state_embedding [B, state_embed_dim]) -> (DecisionRecurrentFnOutput, afterstate_embedding),
        chance_fn(outcome [B], afterstate_embedding [B, afterstate_embed_dim]) -> (ChanceRecurrentFnOutput, state_embedding).

        As in mctx BOTH functions are evaluated on all rows in every simulation -- the decision function at action
        clamp(slot, 0, A - 1), the chance function at outcome clamp(slot - A, 0, C - 1), each on the parent row cut to its
        own width -- and the expansion kernel keeps, per root, the half that matches the parent's kind.  key, noise,
        invalid_actions, temperature, gumbel ([B, A]), with_tree and graph= / graph_key= / graph_version= as in search()."""
        A, Cn = self.cfg.num_actions, self.cfg.num_chance_outcomes

        def recurrent_expand(sim, slot, _, pemb):
            d_out, after = decision_fn(slot.clamp(0, A - 1), pemb[:, :self._es])
            c_out, state = chance_fn((slot - A).clamp(0, Cn - 1), pemb[:, :self._ea])
            self.expand_backup_stochastic(sim, d_out, after, c_out, state)

        gkey = graph_key if graph_key is not None else (fn_identity(decision_fn), fn_identity(chance_fn))
        return self._search_stochastic(root_fn_output, recurrent_expand, gkey, (decision_fn, chance_fn), key, invalid_actions,
                                       dirichlet_noise, dirichlet_fraction, temperature, gumbel, with_tree, graph, graph_version)
