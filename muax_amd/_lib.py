"""ctypes binding of include/mzsearch.h (the C-ABI of the HIP search library).

The product path has NO CPU fallback: if libmzsearch.so is missing, or there is
no gfx950 device, the calls below raise.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _build

_vp = C.c_void_p  # device pointers travel as integers

MZS_OK, MZS_E_INVALID, MZS_E_UNSUPPORTED, MZS_E_RUNTIME, MZS_E_NODEVICE = 0, -1, -2, -3, -4


class MzsConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("device", C.c_int32), ("batch", C.c_int32),
                ("num_actions", C.c_int32), ("num_simulations", C.c_int32), ("embed_dim", C.c_int32),
                ("max_depth", C.c_int32), ("qtransform", C.c_int32), ("tiebreak", C.c_int32),
                ("policy", C.c_int32), ("pb_c_init", C.c_float), ("pb_c_base", C.c_float),
                ("global_batch", C.c_int64), ("root_offset", C.c_int64),
                ("max_num_considered_actions", C.c_int32), ("gumbel_scale", C.c_float),
                ("num_chance_outcomes", C.c_int32), ("state_embed_dim", C.c_int32),
                ("afterstate_embed_dim", C.c_int32), ("reserved0", C.c_int32)]


# the eight arrays of mzs_stochastic_outputs, in the struct's order: the decision function's three, the chance function's five
STOCHASTIC_OUTPUT_FIELDS = ("chance_logits", "afterstate_value", "afterstate_embedding", "action_logits", "value", "reward",
                            "discount", "state_embedding")


class MzsStochasticOutputs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("reserved0", C.c_int32)] + [(n, _vp) for n in STOCHASTIC_OUTPUT_FIELDS]


# the seven Linear(16)-elu-Linear stacks of mzs_stochastic_mlp_weights, in the struct's order
STOCHASTIC_MLP_HEADS = ["ad", "av", "ac", "cr", "cn", "pv", "pp"]
STOCHASTIC_MLP_WEIGHT_NAMES = [f"{h}_{a}" for h in STOCHASTIC_MLP_HEADS for a in ("w1", "b1", "w2", "b2")]


class MzsStochasticMlpWeights(C.Structure):
    _fields_ = ([("struct_size", C.c_int32), ("support_size", C.c_int32), ("discount", C.c_float), ("reserved0", C.c_float)]
                + [(n, _vp) for n in STOCHASTIC_MLP_WEIGHT_NAMES])


class MzsStochasticSearchArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("export_tree", C.c_int32), ("prior_logits", _vp), ("value", _vp),
                ("embedding", _vp), ("invalid_actions", _vp), ("dirichlet_noise", _vp), ("gumbel", _vp),
                ("key", C.c_uint32 * 2), ("dirichlet_fraction", C.c_float), ("temperature", C.c_float),
                ("device_block", _vp), ("action", _vp), ("action_weights", _vp), ("search_value", _vp),
                ("depth_sum", _vp)]


# the 34 arrays of mzs_stochastic_train_weights (the fused stochastic training step), in the struct's order
STOCHASTIC_TRAIN_WEIGHT_NAMES = ["repr_w", "repr_b"] + STOCHASTIC_MLP_WEIGHT_NAMES + ["en_w1", "en_b1", "en_w2", "en_b2"]


class MzsStochasticTrainWeights(C.Structure):
    _fields_ = ([("struct_size", C.c_int32), ("obs_dim", C.c_int32), ("support_size", C.c_int32), ("reserved0", C.c_int32)]
                + [(n, _vp) for n in STOCHASTIC_TRAIN_WEIGHT_NAMES])


class MzsStochasticTrainArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("device", C.c_int32), ("batch", C.c_int32), ("unroll_steps", C.c_int32),
                ("num_actions", C.c_int32), ("num_chance_outcomes", C.c_int32), ("embed_dim", C.c_int32),
                ("reserved0", C.c_int32), ("obs", _vp), ("actions", _vp), ("rewards", _vp), ("returns", _vp),
                ("policy", _vp), ("sample_weight", _vp), ("loss_scale", C.c_float), ("l2_coeff", C.c_float),
                ("vqvae_beta", C.c_float), ("reserved1", C.c_float), ("loss", _vp), ("grads", _vp), ("workspace", _vp),
                ("workspace_bytes", C.c_int64)]


MLP_WEIGHT_NAMES = ["repr_w", "repr_b", "pv_w1", "pv_b1", "pv_w2", "pv_b2", "pp_w1", "pp_b1", "pp_w2",
                    "pp_b2", "dr_w1", "dr_b1", "dr_w2", "dr_b2", "dn_w1", "dn_b1", "dn_w2", "dn_b2"]


class MzsMlpWeights(C.Structure):
    _fields_ = ([("struct_size", C.c_int32), ("obs_dim", C.c_int32), ("support_size", C.c_int32),
                 ("recurrent_pred_on", C.c_int32), ("discount", C.c_float), ("reserved0", C.c_float)]
                + [(n, _vp) for n in MLP_WEIGHT_NAMES])


TREE_FIELDS = ["node_visits", "raw_values", "node_values", "parents", "action_from_parent",
               "children_index", "children_prior_logits", "children_values", "children_visits",
               "children_rewards", "children_discounts", "embeddings"]
TREE_INT_FIELDS = {"node_visits", "parents", "action_from_parent", "children_index", "children_visits"}


class MzsTreeView(C.Structure):
    _fields_ = [(n, _vp) for n in TREE_FIELDS]


class MzsActArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("reserved0", C.c_int32), ("obs", _vp),
                ("dirichlet_noise", _vp), ("invalid_actions", _vp), ("gumbel", _vp),
                ("key", C.c_uint32 * 2), ("dirichlet_fraction", C.c_float), ("temperature", C.c_float),
                ("action", _vp), ("action_weights", _vp), ("root_value", _vp), ("search_value", _vp),
                ("depth_sum", _vp), ("tree", C.POINTER(MzsTreeView))]


class MzsActHostArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("draw_dirichlet", C.c_int32), ("obs", _vp), ("dirichlet_noise", _vp),
                ("invalid_actions", _vp), ("key", C.c_uint32 * 2), ("dirichlet_fraction", C.c_float),
                ("dirichlet_alpha", C.c_float), ("temperature", C.c_float), ("reserved0", C.c_float),
                ("action", _vp), ("action_weights", _vp), ("root_value", _vp)]


class MzsTrainArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("device", C.c_int32), ("batch", C.c_int32),
                ("unroll_steps", C.c_int32), ("num_actions", C.c_int32), ("embed_dim", C.c_int32),
                ("obs", _vp), ("actions", _vp), ("rewards", _vp), ("returns", _vp), ("policy", _vp),
                ("loss_scale", C.c_float), ("l2_coeff", C.c_float), ("loss", _vp), ("grads", _vp),
                ("workspace", _vp), ("workspace_bytes", C.c_int64)]


class MzsTowerArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("device", C.c_int32), ("batch", C.c_int32), ("blocks", C.c_int32),
                ("normalize", C.c_int32), ("num_actions", C.c_int32), ("x", _vp), ("action", _vp),
                ("stem_w", _vp), ("conv_w", _vp), ("ln", _vp), ("y", _vp)]
    HEAD_FIELDS = ["r_c1", "r_c2", "r_l1", "r_b1", "r_l2", "r_b2", "v_c1", "v_c2", "v_l1", "v_b1", "v_l2", "v_b2",
                   "p_c1", "p_l1", "p_b1", "p_l2", "p_b2"]
    _fields_ += [(n, _vp) for n in HEAD_FIELDS] + [("reward", _vp), ("value", _vp), ("prior_logits", _vp),
                                                   ("support_size", C.c_int32), ("reserved0", C.c_int32),
                                                   ("pair_scratch", _vp), ("pair_scratch_bytes", C.c_int64)]


class MzsLayerNormArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("device", C.c_int32), ("batch", C.c_int32), ("n", C.c_int32),
                ("channels", C.c_int32), ("relu", C.c_int32), ("eps", C.c_float),
                ("x", _vp), ("scale", _vp), ("offset", _vp), ("x2", _vp), ("scale2", _vp), ("offset2", _vp),
                ("residual", _vp), ("y", _vp), ("workspace", _vp), ("workspace_bytes", C.c_int64)]


class MzsEzHead(C.Structure):
    FIELDS = ["ln_in", "c1", "ln_mid", "fc", "ln_vec", "out_w", "out_b"]
    _fields_ = [(n, _vp) for n in FIELDS]


class MzsEzArgs(C.Structure):
    WEIGHTS = ["d_ln_in", "d_conv", "d_ln0", "d_conv0", "d_ln1", "d_conv1", "p_ln0", "p_conv0", "p_ln1", "p_conv1"]
    _fields_ = ([("struct_size", C.c_int32), ("device", C.c_int32), ("batch", C.c_int32), ("channels", C.c_int32),
                 ("num_actions", C.c_int32), ("support_size", C.c_int32), ("x", _vp), ("action", _vp), ("y", _vp),
                 ("reward", _vp), ("value", _vp), ("prior_logits", _vp)] + [(n, _vp) for n in WEIGHTS]
                + [("r", MzsEzHead), ("v", MzsEzHead), ("p", MzsEzHead)])


class MzsConv3x3Args(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("device", C.c_int32), ("batch", C.c_int32), ("height", C.c_int32),
                ("width", C.c_int32), ("channels", C.c_int32), ("relu", C.c_int32), ("reserved0", C.c_int32),
                ("x", _vp), ("w_packed", _vp), ("y", _vp)]


class MzsRootTailArgs(C.Structure):
    HEAD_FIELDS = ["v_c1", "v_c2", "v_l1", "v_b1", "v_l2", "v_b2", "p_c1", "p_l1", "p_b1", "p_l2", "p_b2"]
    _fields_ = ([("struct_size", C.c_int32), ("device", C.c_int32), ("batch", C.c_int32), ("height", C.c_int32),
                 ("width", C.c_int32), ("num_actions", C.c_int32), ("support_size", C.c_int32), ("normalize", C.c_int32),
                 ("x", _vp)] + [(n, _vp) for n in HEAD_FIELDS] + [("embedding", _vp), ("value", _vp), ("prior_logits", _vp)])


class MzsConv3x3sArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("device", C.c_int32), ("batch", C.c_int32), ("height", C.c_int32),
                ("width", C.c_int32), ("in_channels", C.c_int32), ("out_channels", C.c_int32), ("relu", C.c_int32),
                ("in_div", C.c_float), ("reserved0", C.c_int32), ("x", _vp), ("w_packed", _vp), ("y", _vp)]


class MzsResblockArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("device", C.c_int32), ("batch", C.c_int32), ("height", C.c_int32),
                ("width", C.c_int32), ("channels", C.c_int32), ("eps", C.c_float), ("reserved0", C.c_int32),
                ("x", _vp), ("w_proj", _vp), ("w0", _vp), ("w1", _vp), ("proj_scale", _vp), ("proj_offset", _vp),
                ("ln0_scale", _vp), ("ln0_offset", _vp), ("ln1_scale", _vp), ("ln1_offset", _vp), ("y", _vp),
                ("workspace", _vp), ("workspace_bytes", C.c_int64)]


class MzsReplayArena(C.Structure):
    _fields_ = ([("struct_size", C.c_int32), ("device", C.c_int32), ("max_steps", C.c_int64), ("capacity", C.c_int32),
                 ("obs_dim", C.c_int32), ("num_actions", C.c_int32), ("reserved0", C.c_int32)]
                + [(n, _vp) for n in ("obs", "a", "r", "Rn", "v", "done", "pi", "w", "cw", "t_start", "t_len", "t_w",
                                      "t_serial", "c_start", "c_len", "c_CW", "c_serial")])


class MzsReplayStoreArgs(C.Structure):
    _fields_ = ([("struct_size", C.c_int32), ("episodes", C.c_int32), ("stream_steps", C.c_int64), ("raw", C.c_int32),
                 ("n_step", C.c_int32), ("weight_mode", C.c_int32), ("has_alpha", C.c_int32), ("alpha", C.c_double)]
                + [(n, _vp) for n in ("desc_host", "desc", "serial", "ep_w", "gpow", "obs", "a", "pi", "r", "v", "Rn",
                                      "done", "w")])


class MzsReplaySampleArgs(C.Structure):
    _fields_ = ([("struct_size", C.c_int32), ("count", C.c_int32), ("batch", C.c_int32), ("k_steps", C.c_int32),
                 ("sample_per_trajectory", C.c_int32), ("key", C.c_uint32 * 2), ("obs_steps", C.c_int32)]
                + [(n, _vp) for n in ("obs", "a", "r", "Rn", "v", "done", "pi", "w", "serial", "start")])


class MzsReplayIsArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("normalize", C.c_int32), ("beta", C.c_double), ("num_windows", C.c_double),
                ("isw", _vp), ("scratch", _vp)]


class MzsReplayGatherArgs(C.Structure):
    _fields_ = ([("struct_size", C.c_int32), ("episodes", C.c_int32), ("stream_rows", C.c_int64),
                 ("rows_padded", C.c_int64)] + [(n, _vp) for n in ("desc", "desc_host", "obs")])


class MzsReplayReanalyseArgs(C.Structure):
    _fields_ = ([("struct_size", C.c_int32), ("episodes", C.c_int32), ("stream_rows", C.c_int64),
                 ("rows_padded", C.c_int64), ("desc", _vp), ("desc_host", _vp), ("n_step", C.c_int32),
                 ("weight_mode", C.c_int32), ("has_alpha", C.c_int32), ("reserved0", C.c_int32), ("alpha", C.c_double)]
                + [(n, _vp) for n in ("gpow", "pi", "v")])


class MzsReplayUpdateArgs(C.Structure):
    _fields_ = ([("struct_size", C.c_int32), ("head", C.c_int32), ("count", C.c_int32), ("batch", C.c_int32),
                 ("k_prio", C.c_int32), ("weight_mode", C.c_int32), ("alpha", C.c_double), ("eps", C.c_double)]
                + [(n, _vp) for n in ("serial", "start", "prio", "owner", "touched")])


class MzsReplayRing(C.Structure):
    _fields_ = ([("struct_size", C.c_int32), ("device", C.c_int32), ("ring_steps", C.c_int32), ("num_envs", C.c_int32),
                 ("obs_dim", C.c_int32), ("num_actions", C.c_int32)] + [(n, _vp) for n in ("obs", "a", "r", "v", "pi")])


class MzsReplayStageArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("row", C.c_int32)] + [(n, _vp) for n in ("obs", "a", "v", "pi")]


class MzsReplayStoreStepsArgs(C.Structure):
    _fields_ = ([("struct_size", C.c_int32), ("episodes", C.c_int32), ("n_step", C.c_int32), ("weight_mode", C.c_int32),
                 ("has_alpha", C.c_int32), ("reserved0", C.c_int32), ("alpha", C.c_double)]
                + [(n, _vp) for n in ("desc_host", "desc", "serial", "gpow")])


class MzsReplayPlanArgs(C.Structure):
    _fields_ = ([("struct_size", C.c_int32), ("row0", C.c_int32), ("steps", C.c_int32), ("min_length", C.c_int32),
                 ("max_out", C.c_int32), ("reserved0", C.c_int32)]
                + [(n, _vp) for n in ("done", "open_len", "open_ret", "ep", "ret", "counts", "scratch")])


def replay_plan_scratch(num_envs: int) -> int:
    """int32 elements of `scratch` that mzs_replay_plan_steps needs for `num_envs` environments (include/mzsearch.h)."""
    return int(num_envs) + (int(num_envs) + 255) // 256


class MzsEnvCartPole(C.Structure):
    _fields_ = ([("struct_size", C.c_int32), ("device", C.c_int32), ("num_envs", C.c_int32),
                 ("max_episode_steps", C.c_int32), ("key", C.c_uint32 * 2)]
                + [(n, _vp) for n in ("state", "t", "draws")])


class MzsEnvStepArgs(C.Structure):
    _fields_ = ([("struct_size", C.c_int32), ("reserved0", C.c_int32)]
                + [(n, _vp) for n in ("a", "obs_out", "r_out", "done_out")])


MZS_ENV_ACROBOT, MZS_ENV_MOUNTAINCAR = 1, 2


class MzsEnvClassic(C.Structure):
    _fields_ = ([("struct_size", C.c_int32), ("device", C.c_int32), ("kind", C.c_int32), ("num_envs", C.c_int32),
                 ("max_episode_steps", C.c_int32), ("key", C.c_uint32 * 2)]
                + [(n, _vp) for n in ("state", "t", "draws")])


class MzsEnv2048(C.Structure):
    _fields_ = ([("struct_size", C.c_int32), ("device", C.c_int32), ("num_envs", C.c_int32),
                 ("max_episode_steps", C.c_int32), ("key", C.c_uint32 * 2), ("reward_shift", C.c_int32),
                 ("reserved0", C.c_int32)]
                + [(n, _vp) for n in ("board", "t", "draws", "invalid")])


class MzsUnrollArgs(C.Structure):
    _fields_ = ([("struct_size", C.c_int32), ("device", C.c_int32), ("batch", C.c_int32), ("row_steps", C.c_int32),
                 ("k_prio", C.c_int32), ("num_actions", C.c_int32), ("embed_dim", C.c_int32), ("reserved0", C.c_int32)]
                + [(n, _vp) for n in ("obs", "actions", "returns", "values", "prio")])


class MzsStochasticUnrollArgs(C.Structure):
    _fields_ = ([("struct_size", C.c_int32), ("device", C.c_int32), ("batch", C.c_int32), ("row_steps", C.c_int32),
                 ("k_prio", C.c_int32), ("num_actions", C.c_int32), ("num_chance_outcomes", C.c_int32),
                 ("embed_dim", C.c_int32)]
                + [(n, _vp) for n in ("obs", "actions", "returns", "values", "prio", "codes")])


def args(cls, **fields):
    """A `cls` argument struct with `struct_size` set and the given fields assigned (a tuple fills an array field)."""
    a = cls()
    a.struct_size = C.sizeof(cls)
    for name, value in fields.items():
        setattr(a, name, value)
    return a


# The two tables below ARE the binding: every `typedef struct` and every function of include/mzsearch.h, in the header's
# order.  tests/test_abi_cpu.py compares both with the header, and every struct's layout with the host compiler's.
STRUCTS = {
    "mzs_config": MzsConfig,
    "mzs_mlp_weights": MzsMlpWeights,
    "mzs_tree_view": MzsTreeView,
    "mzs_act_args": MzsActArgs,
    "mzs_act_host_args": MzsActHostArgs,
    "mzs_stochastic_outputs": MzsStochasticOutputs,
    "mzs_stochastic_mlp_weights": MzsStochasticMlpWeights,
    "mzs_stochastic_search_args": MzsStochasticSearchArgs,
    "mzs_ez_head": MzsEzHead,
    "mzs_ez_args": MzsEzArgs,
    "mzs_layernorm_args": MzsLayerNormArgs,
    "mzs_train_args": MzsTrainArgs,
    "mzs_stochastic_train_weights": MzsStochasticTrainWeights,
    "mzs_stochastic_train_args": MzsStochasticTrainArgs,
    "mzs_tower_args": MzsTowerArgs,
    "mzs_root_tail_args": MzsRootTailArgs,
    "mzs_conv3x3_args": MzsConv3x3Args,
    "mzs_conv3x3s_args": MzsConv3x3sArgs,
    "mzs_resblock_args": MzsResblockArgs,
    "mzs_replay_arena": MzsReplayArena,
    "mzs_replay_store_args": MzsReplayStoreArgs,
    "mzs_replay_sample_args": MzsReplaySampleArgs,
    "mzs_replay_is_args": MzsReplayIsArgs,
    "mzs_replay_gather_args": MzsReplayGatherArgs,
    "mzs_replay_reanalyse_args": MzsReplayReanalyseArgs,
    "mzs_replay_update_args": MzsReplayUpdateArgs,
    "mzs_replay_ring": MzsReplayRing,
    "mzs_replay_stage_args": MzsReplayStageArgs,
    "mzs_replay_store_steps_args": MzsReplayStoreStepsArgs,
    "mzs_replay_plan_args": MzsReplayPlanArgs,
    "mzs_env_cartpole": MzsEnvCartPole,
    "mzs_env_step_args": MzsEnvStepArgs,
    "mzs_env_classic": MzsEnvClassic,
    "mzs_env_2048": MzsEnv2048,
    "mzs_unroll_args": MzsUnrollArgs,
    "mzs_stochastic_unroll_args": MzsStochasticUnrollArgs,
}

_P, _i32, _i64, _f32 = C.POINTER, C.c_int32, C.c_int64, C.c_float
_key, _plan = _P(C.c_uint32 * 2), _P(C.c_int32 * 4)  # `const uint32_t key[2]` (host values), `int32_t out[4]`
_arena, _ring, _step = _P(MzsReplayArena), _P(MzsReplayRing), _P(MzsEnvStepArgs)

# name -> (restype, argtypes)
ENTRIES = {
    "mzs_abi_version": (C.c_int, []),
    "mzs_last_error": (C.c_char_p, [_vp]),
    "mzs_create": (C.c_int, [_P(MzsConfig), _P(_vp)]),
    "mzs_destroy": (C.c_int, [_vp]),
    # fused path: whole act() for the default MLP trio in one launch
    "mzs_mlp_set_weights": (C.c_int, [_vp, _P(MzsMlpWeights)]),
    "mzs_act_mlp": (C.c_int, [_vp, _P(MzsActArgs), _vp]),
    # the same from HOST memory
    "mzs_act_mlp_host": (C.c_int, [_vp, _P(MzsActHostArgs), _vp]),
    # step-wise path: any repr/pred/dyn plugin nets run by the caller
    "mzs_root": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _f32, _key, _vp]),
    "mzs_root_gumbel": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _key, _vp]),
    "mzs_select": (C.c_int, [_vp, _i32, _vp, _vp, _vp]),
    "mzs_expand_backup": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mzs_expand_backup_select": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mzs_finish": (C.c_int, [_vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mzs_tree_export": (C.c_int, [_vp, _P(MzsTreeView), _vp]),
    # step-wise path, stochastic policy
    "mzs_root_stochastic": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _f32, _key, _vp]),
    "mzs_select_stochastic": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp]),
    "mzs_expand_backup_stochastic": (C.c_int, [_vp, _i32, _P(MzsStochasticOutputs), _vp]),
    "mzs_finish_stochastic": (C.c_int, [_vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp]),
    # the default stochastic MLP family evaluated by the library
    "mzs_mlp_set_stochastic_weights": (C.c_int, [_vp, _P(MzsStochasticMlpWeights)]),
    "mzs_mlp_stochastic_recurrent": (C.c_int, [_vp, _vp, _vp, _vp, _P(MzsStochasticOutputs), _vp]),
    # the WHOLE stochastic search of the bound family in ONE launch
    "mzs_mlp_stochastic_plan": (C.c_int, [_i32] * 5 + [_plan]),
    "mzs_mlp_stochastic_search": (C.c_int, [_vp, _P(MzsStochasticSearchArgs), _vp]),
    "mzs_stochastic_search_block": (C.c_int, [_key, _i32, _f32, _f32, _vp]),
    # root inference of the bound family evaluated by the library
    "mzs_mlp_set_stochastic_representation": (C.c_int, [_vp, _i32, _vp, _vp]),
    "mzs_mlp_stochastic_root": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "mzs_mlp_stochastic_search_obs": (C.c_int, [_vp, _P(MzsStochasticSearchArgs), _vp, _vp, _vp]),
    # the root exploration noise drawn inside the one launch
    "mzs_mlp_stochastic_search_draw": (C.c_int, [_vp, _P(MzsStochasticSearchArgs), _vp, _vp, _f32, _vp, _vp]),
    "mzs_stochastic_search_block_draw": (C.c_int, [_key, _i32, _f32, _f32, _f32, _vp]),
    # recurrent_fn of the EfficientZero-style nets
    "mzs_ez_recurrent": (C.c_int, [_P(MzsEzArgs), _vp]),
    # fused LayerNorm of the convolutional plugin nets
    "mzs_layernorm_act": (C.c_int, [_P(MzsLayerNormArgs), _vp]),
    "mzs_layernorm_workspace_bytes": (_i64, [_i32, _i32]),
    # device self-test
    "mzs_selftest": (C.c_int, [_i32, _P(_i64 * 4)]),
    # root exploration noise
    "mzs_dirichlet": (C.c_int, [_i32, _key, _f32, _i32, _i32, _i64, _i64, _vp, _vp]),
    # training step of the default MLP trio
    "mzs_mlp_num_params": (_i64, [_i32] * 4),
    "mzs_mlp_train_workspace_bytes": (_i64, [_i32] * 5),
    "mzs_mlp_loss_grad": (C.c_int, [_P(MzsMlpWeights), _P(MzsTrainArgs), _vp]),
    "mzs_mlp_loss_grad_weighted": (C.c_int, [_P(MzsMlpWeights), _P(MzsTrainArgs), _vp, _vp]),
    # training step of the default stochastic MLP family
    "mzs_stochastic_mlp_num_params": (_i64, [_i32] * 5),
    "mzs_stochastic_mlp_train_workspace_bytes": (_i64, [_i32] * 6),
    "mzs_stochastic_mlp_loss_grad": (C.c_int, [_P(MzsStochasticTrainWeights), _P(MzsStochasticTrainArgs), _vp]),
    # next-state tower of the ResNet dynamics net, and the tail of root inference with those nets
    "mzs_resnet_tower": (C.c_int, [_P(MzsTowerArgs), _vp]),
    "mzs_tower_pair_scratch_bytes": (_i64, [_i32]),
    "mzs_resnet_root_tail": (C.c_int, [_P(MzsRootTailArgs), _vp]),
    # 3x3 convolutions, stems and whole residual blocks of the representation nets
    "mzs_conv3x3_nhwc": (C.c_int, [_P(MzsConv3x3Args), _vp]),
    "mzs_conv3x3_stride2_nhwc": (C.c_int, [_P(MzsConv3x3sArgs), _vp]),
    "mzs_resblock_v1": (C.c_int, [_P(MzsResblockArgs), _vp]),
    "mzs_resblock_workspace_bytes": (_i64, [_i32] * 4),
    "mzs_resblock_v2": (C.c_int, [_P(MzsResblockArgs), _vp]),
    "mzs_resblock_v2_workspace_bytes": (_i64, [_i32] * 4),
    # fused-kernel instances built on demand, and the routes for shapes without one
    "mzs_register_fused_dispatch": (C.c_int, [_vp, _i32]),
    "mzs_register_fused_dispatch_muzero": (C.c_int, [_vp, _i32]),
    "mzs_fused_jit_abi": (C.c_int, []),
    "mzs_register_train_dispatch": (C.c_int, [_vp, _i32, _i32, _i32, _i32]),
    "mzs_train_jit_abi": (C.c_int, []),
    "mzs_register_stochastic_train_dispatch": (C.c_int, [_vp] + [_i32] * 6),
    "mzs_stochastic_train_jit_abi": (C.c_int, []),
    "mzs_mlp_allow_generic": (C.c_int, [_vp, _i32]),
    "mzs_mlp_allow_wide": (C.c_int, [_vp, _i32]),
    "mzs_mlp_allow_wide_gumbel": (C.c_int, [_vp, _i32]),
    "mzs_mlp_wide_plan": (C.c_int, [_i32] * 4 + [_plan]),
    "mzs_mlp_wide_plan_policy": (C.c_int, [_i32] * 5 + [_plan]),
    # the simulation loop of a search with the ResNet nets in ONE launch
    "mzs_resnet_search": (C.c_int, [_vp, _P(MzsTowerArgs), _f32, _i32, _i32, _vp]),
    # device-resident trajectory replay
    "mzs_replay_store": (C.c_int, [_arena, _P(MzsReplayStoreArgs), _vp]),
    "mzs_replay_refresh": (C.c_int, [_arena, _i32, _i32, _i32, _vp]),
    "mzs_replay_sample": (C.c_int, [_arena, _P(MzsReplaySampleArgs), _vp]),
    "mzs_replay_sample_is": (C.c_int, [_arena, _P(MzsReplaySampleArgs), _P(MzsReplayIsArgs), _vp]),
    "mzs_replay_gather_obs": (C.c_int, [_arena, _P(MzsReplayGatherArgs), _vp]),
    "mzs_replay_reanalyse": (C.c_int, [_arena, _P(MzsReplayReanalyseArgs), _vp]),
    "mzs_replay_update_priorities": (C.c_int, [_arena, _P(MzsReplayUpdateArgs), _vp]),
    # collection on the device: steps staged in a ring, episodes cut in the store launch
    "mzs_replay_stage": (C.c_int, [_ring, _P(MzsReplayStageArgs), _vp]),
    "mzs_replay_store_steps": (C.c_int, [_arena, _ring, _P(MzsReplayStoreStepsArgs), _vp]),
    "mzs_replay_plan_steps": (C.c_int, [_ring, _P(MzsReplayPlanArgs), _vp]),
    # vector environments stepped on the device: the cart-pole; Acrobot and MountainCar; 2048
    "mzs_env_cartpole_reset": (C.c_int, [_P(MzsEnvCartPole), _vp, _vp]),
    "mzs_env_cartpole_step": (C.c_int, [_P(MzsEnvCartPole), _step, _vp]),
    "mzs_env_classic_reset": (C.c_int, [_P(MzsEnvClassic), _vp, _vp]),
    "mzs_env_classic_step": (C.c_int, [_P(MzsEnvClassic), _step, _vp]),
    "mzs_env_2048_reset": (C.c_int, [_P(MzsEnv2048), _vp, _vp]),
    "mzs_env_2048_step": (C.c_int, [_P(MzsEnv2048), _step, _vp]),
    "mzs_env_2048_mask": (C.c_int, [_i32, _vp, _vp, _i32, _vp]),
    # forward value unroll of the default MLP trio
    "mzs_mlp_unroll_values": (C.c_int, [_P(MzsMlpWeights), _P(MzsUnrollArgs), _vp]),
    # ... and of the default stochastic MLP family
    "mzs_stochastic_mlp_unroll_values": (C.c_int, [_P(MzsStochasticTrainWeights), _P(MzsStochasticUnrollArgs), _vp]),
}
EXPORTED_SYMBOLS = list(ENTRIES)

_lib = None


def load(build_if_missing: bool = True):
    """Load muax_amd/lib/libmzsearch.so; raises RuntimeError if it cannot be had."""
    global _lib
    if _lib is not None:
        return _lib
    # MUAX_AMD_LIB: tools only (A/B builds of the same ABI under tools/bin); the product always loads the in-tree library
    path = os.environ.get("MUAX_AMD_LIB") or _build.LIB_PATH
    if not os.path.exists(path):
        if not build_if_missing:
            raise RuntimeError(f"{path} is missing: build it with `python -m muax_amd._build`")
        _build.build()
    L = C.CDLL(path)
    for name, (restype, argtypes) in ENTRIES.items():
        f = getattr(L, name)  # (AttributeError: the shared object lacks a declared entry)
        f.restype, f.argtypes = restype, argtypes
    if L.mzs_abi_version() != 1:
        raise RuntimeError("libmzsearch.so ABI version mismatch")
    _lib = L
    return L


class Unsupported(ValueError):
    """MZS_E_UNSUPPORTED: the arguments are well formed, the library has no kernel for this configuration."""


class NoKernelInstance(Unsupported):
    """No instance of the fused act() / training kernel for this shape: one may be built on demand (muax_amd/_jit.py)."""


class TooLargeForLds(Unsupported):
    """The shape is beyond what the kernel keeps in the LDS of a workgroup / a CU."""


class NoCachedDecisions(Unsupported):
    """The handle's tree is walked level by level; the entry needs the cached decisions of mz_step_jump.cuh."""


# MZS_E_UNSUPPORTED is one status code: the library's message tells WHICH refusal it is.  The only place where a message
# of the library is inspected -- callers catch the classes.
_REFUSALS = (("no fused kernel instance", NoKernelInstance), ("no kernel instance", NoKernelInstance),
             ("too large for the LDS", TooLargeForLds), ("cached decisions", NoCachedDecisions))


def check(code: int, handle=None):
    """Map C-ABI status codes onto Python exceptions (ValueError for bad arguments, as the
    reference raises for bad shapes/arguments -- its subclass Unsupported, or the more specific class of _REFUSALS, for
    a configuration without a kernel; RuntimeError for device failures).  The library's message is the exception's text."""
    if code == MZS_OK:
        return
    msg = load().mzs_last_error(handle)
    msg = msg.decode() if msg else f"mzsearch error {code}"
    if code == MZS_E_UNSUPPORTED:
        raise next((cls for words, cls in _REFUSALS if words in msg), Unsupported)(msg)
    if code == MZS_E_INVALID:
        raise ValueError(msg)
    raise RuntimeError(msg)
