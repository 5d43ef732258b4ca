"""Policy adapters of the reference (muax/policy.py): a uniform __call__(params, rng_key, root,
recurrent_fn, **kwargs) over the search implementations -- here the HIP search instead of mctx."""
from __future__ import annotations

from abc import ABC, abstractmethod

from .search import MuZeroSearch, PolicyOutput, SearchConfig, fn_identity


def _search_config(kwargs, num_actions, embed_dim, puct=True, **fields):
    """The keyword arguments every policy takes (and, `puct`, those of the pUCT rule) with the reference's defaults, plus the
    policy's own SearchConfig `fields` -> (cache key, SearchConfig)."""
    get = kwargs.get
    common = dict(max_depth=get("max_depth"), global_batch=get("global_batch"), root_offset=get("root_offset", 0))
    if puct:
        common.update(tiebreak=get("tiebreak", True), pb_c_init=get("pb_c_init", 1.25),
                      pb_c_base=float(get("pb_c_base", 19652)))
    cfg = SearchConfig(num_actions, get("num_simulations", 5), embed_dim, **common, **fields)
    return (num_actions, cfg.num_simulations, embed_dim) + tuple(common.values()) + tuple(fields.values()), cfg


def _flat_recurrent(recurrent_fn, params, batch, shape):
    """recurrent_fn in the search's calling convention: flat embedding rows in and out."""
    def rec(action, flat_emb):
        (reward, discount, logits, v), nxt = recurrent_fn(params, None, action, flat_emb.reshape((batch,) + shape))
        return reward, discount, logits, v, nxt.reshape(batch, -1)
    return rec


class Policy(ABC):
    """muax/policy.py:7-10.  One search handle per (batch, device, configuration), kept for the policy's lifetime."""

    def __init__(self):
        self._handles = {}

    def _handle(self, batch, device, cfg_key, cfg):
        key = (batch, cfg_key, str(device))
        if key not in self._handles:
            self._handles[key] = MuZeroSearch(batch, cfg, device)
        return self._handles[key]

    @abstractmethod
    def __call__(self, params, rng_key, root, recurrent_fn=None, decision_recurrent_fn=None,
                 chance_recurrent_fn=None, **kwargs):
        pass


class MuZeroPolicy(Policy):
    """muax/policy.py:13-30: mctx.muzero_policy with the same keyword defaults.

    `root` is (prior_logits [B,A], value [B], embedding [B,...]) as in mctx.RootFnOutput;
    `recurrent_fn(params, rng_key, action, embedding)` returns ((reward, discount, prior_logits, value),
    next_embedding) as in muax/model.py:265-282.  Runs the step-wise HIP search (any plugin nets)."""

    def __call__(self, params, rng_key, root, recurrent_fn, **kwargs) -> PolicyOutput:
        prior_logits, value, embedding = root
        if kwargs.get("qtransform") not in (None, "qtransform_by_parent_and_siblings"):
            raise ValueError("only qtransform_by_parent_and_siblings is implemented")
        B, A = prior_logits.shape
        emb = embedding.reshape(B, -1)
        h = self._handle(B, prior_logits.device, *_search_config(kwargs, A, emb.shape[1]))
        shape = tuple(embedding.shape[1:])
        return h.search((prior_logits, value, emb), _flat_recurrent(recurrent_fn, params, B, shape), key=rng_key,
                        invalid_actions=kwargs.get("invalid_actions"),
                        dirichlet_noise=kwargs.get("dirichlet_noise"),
                        dirichlet_fraction=kwargs.get("dirichlet_fraction", 0.25),
                        temperature=kwargs.get("temperature", 1.0), gumbel=kwargs.get("gumbel"),
                        with_tree=kwargs.get("with_tree", False), graph=kwargs.get("graph", False),
                        graph_key=(fn_identity(recurrent_fn), id(params), shape),
                        graph_version=kwargs.get("graph_version", 0), native_loop=kwargs.get("native_loop"))


class GumbelMuZeroPolicy(Policy):
    """muax/policy.py:33-47: mctx.gumbel_muzero_policy with the same keyword defaults
    (max_num_considered_actions=16, gumbel_scale=1).  Runs on the step-wise HIP kernels.

    qtransform: mctx's own default for this policy is qtransform_completed_by_mix_value, which is what
    this adapter uses when called directly.  Note the reference quirk one level up: MuZero._plan always
    substitutes qtransform_by_parent_and_siblings when none is given (muax/model.py:230-231), so going
    through MuZero.act the Gumbel search runs with THAT transform unless one is passed explicitly --
    muax_amd.MuZero reproduces this."""

    def __call__(self, params, rng_key, root, recurrent_fn=None, decision_recurrent_fn=None,
                 chance_recurrent_fn=None, **kwargs) -> PolicyOutput:
        prior_logits, value, embedding = root
        B, A = prior_logits.shape
        emb = embedding.reshape(B, -1)
        qt = kwargs.get("qtransform") or "qtransform_completed_by_mix_value"
        h = self._handle(B, prior_logits.device, *_search_config(
            kwargs, A, emb.shape[1], puct=False, tiebreak=False, policy="gumbel", qtransform=getattr(qt, "__name__", qt),
            max_num_considered_actions=kwargs.get("max_num_considered_actions", 16),
            gumbel_scale=float(kwargs.get("gumbel_scale", 1))))
        shape = tuple(embedding.shape[1:])
        return h.search((prior_logits, value, emb), _flat_recurrent(recurrent_fn, params, B, shape), key=rng_key,
                        invalid_actions=kwargs.get("invalid_actions"), gumbel=kwargs.get("gumbel"),
                        with_tree=kwargs.get("with_tree", False), graph=kwargs.get("graph", False),
                        graph_key=(fn_identity(recurrent_fn), id(params), shape),
                        graph_version=kwargs.get("graph_version", 0), native_loop=kwargs.get("native_loop"))


class StochasticMuZeroPolicy(Policy):
    """muax/policy.py:50-67: mctx.stochastic_muzero_policy with the same keyword defaults, on the step-wise HIP
    kernels (chance nodes at odd depth, MuZeroSearch.search_stochastic).

    `root` is (prior_logits [B,A], value [B], state embedding [B,...]);
    `decision_recurrent_fn(params, rng_key, action, state_embedding)` returns
    (DecisionRecurrentFnOutput(chance_logits [B,C], afterstate_value [B]), afterstate_embedding) and
    `chance_recurrent_fn(params, rng_key, chance_outcome, afterstate_embedding)` returns
    (ChanceRecurrentFnOutput(action_logits [B,A], value, reward, discount [B]), state_embedding), as in mctx.
    The number of chance outcomes and the afterstate embedding's shape come from the `num_chance_outcomes=` and
    `afterstate_shape=` kwargs; without both, one dummy decision call at action 0 supplies them, as mctx does.
    The returned search_tree is the decision slice [..., :A] of the children arrays (mctx's masked tree)."""

    def __init__(self):
        super().__init__()
        self._shapes = {}

    def __call__(self, params, rng_key, root, recurrent_fn=None, decision_recurrent_fn=None,
                 chance_recurrent_fn=None, **kwargs) -> PolicyOutput:
        if decision_recurrent_fn is None or chance_recurrent_fn is None:
            raise ValueError("StochasticMuZeroPolicy needs decision_recurrent_fn and chance_recurrent_fn")
        qt = kwargs.get("qtransform")
        if getattr(qt, "__name__", qt) not in (None, "qtransform_by_parent_and_siblings"):
            raise ValueError("only qtransform_by_parent_and_siblings is implemented")
        prior_logits, value, embedding = root
        B, A = prior_logits.shape
        emb = embedding.reshape(B, -1)
        shape = tuple(embedding.shape[1:])
        C, after_shape = kwargs.get("num_chance_outcomes"), kwargs.get("afterstate_shape")
        if C is None or after_shape is None:
            skey = (fn_identity(decision_recurrent_fn), B, shape)
            if skey not in self._shapes:
                import torch
                with torch.no_grad():
                    out, after = decision_recurrent_fn(params, None, torch.zeros(B, dtype=torch.int32, device=emb.device),
                                                       embedding)
                self._shapes[skey] = (int(out[0].shape[-1]), tuple(after.shape[1:]))
            C, after_shape = self._shapes[skey]
        after_shape = tuple(after_shape)
        Es, Ea = emb.shape[1], 1
        for n in after_shape:
            Ea *= int(n)
        h = self._handle(B, prior_logits.device, *_search_config(
            kwargs, A, max(Es, Ea), policy="stochastic", num_chance_outcomes=int(C), state_embed_dim=Es, afterstate_embed_dim=Ea))

        def decision(action, flat_state):
            out, after = decision_recurrent_fn(params, None, action, flat_state.reshape((B,) + shape))
            return out, after.reshape(B, -1)

        def chance(outcome, flat_after):
            out, state = chance_recurrent_fn(params, None, outcome, flat_after.reshape((B,) + after_shape))
            return out, state.reshape(B, -1)

        out = h.search_stochastic((prior_logits, value, emb), decision, chance, key=rng_key,
                                  invalid_actions=kwargs.get("invalid_actions"),
                                  dirichlet_noise=kwargs.get("dirichlet_noise"),
                                  dirichlet_fraction=kwargs.get("dirichlet_fraction", 0.25),
                                  temperature=kwargs.get("temperature", 1.0), gumbel=kwargs.get("gumbel"),
                                  with_tree=kwargs.get("with_tree", False), graph=kwargs.get("graph", False),
                                  graph_key=(fn_identity(decision_recurrent_fn), fn_identity(chance_recurrent_fn),
                                             id(params), shape),
                                  graph_version=kwargs.get("graph_version", 0))
        t = out.search_tree
        if t is not None:  # mctx _mask_tree(tree, num_actions, 'decision')
            t = t._replace(**{f: getattr(t, f)[..., :A] for f in t._fields if f.startswith("children_")})
        return PolicyOutput(out.action, out.action_weights, t)
