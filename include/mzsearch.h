/*
 * mzsearch.h -- C-ABI of the MI355X-native batched MuZero search.
 *
 * This is the drop-in boundary for the one path this repository accelerates:
 * what muax.MuZero._plan hands to mctx.muzero_policy (reference
 * muax/model.py:222-243, muax/policy.py:13-30) and the two callbacks mctx makes
 * into muax (root inference muax/model.py:251-263, recurrent inference
 * muax/model.py:265-282).  The reference has no FFI of its own (it is pure
 * Python on JAX); INTEGRATION.md shows the ctypes stub a muax maintainer would
 * add.  Plain pointers and sizes only; every pointer is a DEVICE pointer owned
 * by the caller (PyTorch) unless stated, borrowed for the duration of the call.
 * All kernels are enqueued on the caller's HIP stream (`stream` is a
 * hipStream_t passed as void*); no entry point synchronises.
 *
 * There is NO CPU fallback behind this ABI: mzs_create fails without a gfx950
 * device.
 *
 * Layout of batched arrays follows mctx: row-major [B], [B,A], [B,E], and for
 * tree views [B,N], [B,N,A], [B,N,E] with N = num_simulations + 1.
 */
#ifndef MZSEARCH_H
#define MZSEARCH_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MZS_ABI_VERSION 1

enum {
  MZS_OK = 0,
  MZS_E_INVALID = -1,     /* bad argument (shape, null, range) -> ValueError */
  MZS_E_UNSUPPORTED = -2, /* configuration has no kernel instance             */
  MZS_E_RUNTIME = -3,     /* HIP runtime error                                 */
  MZS_E_NODEVICE = -4     /* no gfx950 device                                  */
};

typedef struct mzs_handle mzs_handle;

/* Search configuration: the keyword arguments of MuZero.act that reach
 * mctx.muzero_policy (muax/model.py:82-96), plus the batch geometry. */
typedef struct {
  int32_t struct_size;     /* sizeof(mzs_config), for ABI checking */
  int32_t device;          /* HIP device ordinal */
  int32_t batch;           /* B: roots held by this handle (this GPU's shard) */
  int32_t num_actions;     /* A */
  int32_t num_simulations; /* S */
  int32_t embed_dim;       /* E: flattened embedding elements per node */
  int32_t max_depth;       /* <= 0: num_simulations (mctx default) */
  int32_t qtransform;      /* 0: qtransform_by_parent_and_siblings; 1: qtransform_completed_by_mix_value (gumbel policy only) */
  int32_t tiebreak;        /* 0: none; 1: JAX threefry stream (1e-7 * uniform); muzero policy only */
  int32_t policy;          /* 0: mctx.muzero_policy (muax/policy.py:13-30); 1: mctx.gumbel_muzero_policy (muax/policy.py:33-47);
                              2: mctx.stochastic_muzero_policy (muax/policy.py:50-67), step-wise entries *_stochastic only */
  float pb_c_init;         /* 1.25  */
  float pb_c_base;         /* 19652 */
  int64_t global_batch;    /* B of the un-sharded batch (PRNG stream layout); 0 -> batch */
  int64_t root_offset;     /* global index of local root 0 */
  int32_t max_num_considered_actions; /* gumbel policy: 16 (muax/policy.py:45) */
  float gumbel_scale;                 /* gumbel policy: 1.0 (muax/policy.py:46) */
  /* stochastic policy (0 for the others): C chance outcomes, num_actions + C <= 64 slots per node; the widths of the state
   * and afterstate embeddings (0: embed_dim), embed_dim = max of the two, below 256 */
  int32_t num_chance_outcomes;
  int32_t state_embed_dim;
  int32_t afterstate_embed_dim;
  int32_t reserved0;
} mzs_config;

/* Weights of the default MLP trio (muax/nn.py:59-115), haiku layout w[in][out],
 * float32 device pointers. hidden width is 16 as in the reference. */
typedef struct {
  int32_t struct_size;
  int32_t obs_dim;
  int32_t support_size;       /* F = 2*support_size+1 */
  int32_t recurrent_pred_on;  /* 0: child embedding (muax/model.py:272); 1: parent (frameworks/coax/model.py:448) */
  float discount;
  float reserved0;
  const float *repr_w, *repr_b;               /* [obs,E] [E]   */
  const float *pv_w1, *pv_b1, *pv_w2, *pv_b2; /* [E,16] [16] [16,F] [F] */
  const float *pp_w1, *pp_b1, *pp_w2, *pp_b2; /* [E,16] [16] [16,A] [A] */
  const float *dr_w1, *dr_b1, *dr_w2, *dr_b2; /* [E+A,16] [16] [16,F] [F] */
  const float *dn_w1, *dn_b1, *dn_w2, *dn_b2; /* [E+A,16] [16] [16,E] [E] */
} mzs_mlp_weights;

/* Caller-owned output arrays in mctx.Tree layout (search_tree of PolicyOutput).
 * Either every pointer is set or the struct pointer is NULL. */
typedef struct {
  int32_t *node_visits;            /* [B,N]   */
  float *raw_values;               /* [B,N]   */
  float *node_values;              /* [B,N]   */
  int32_t *parents;                /* [B,N]   */
  int32_t *action_from_parent;     /* [B,N]   */
  int32_t *children_index;         /* [B,N,A] */
  float *children_prior_logits;    /* [B,N,A] */
  float *children_values;          /* [B,N,A] */
  int32_t *children_visits;        /* [B,N,A] */
  float *children_rewards;         /* [B,N,A] */
  float *children_discounts;       /* [B,N,A] */
  float *embeddings;               /* [B,N,E] */
} mzs_tree_view;

/* Per-call arguments of the fused act path. */
typedef struct {
  int32_t struct_size;
  int32_t reserved0;
  const float *obs;               /* [B,obs_dim] */
  const float *dirichlet_noise;   /* [B,A] or NULL (then dirichlet_fraction must be 0) */
  const uint8_t *invalid_actions; /* [B,A] 1 = invalid, or NULL */
  const float *gumbel;            /* [B,A] or NULL: drawn from `key` (muzero policy: the categorical's Gumbel;
                                     gumbel policy: the ROOT Gumbel noise, gumbel_scale * gumbel(split(key)[1])) */
  uint32_t key[2];                /* the rng_key given to MuZero.act (HOST values) */
  float dirichlet_fraction;       /* 0.25 */
  float temperature;              /* 1.0  */
  int32_t *action;                /* out [B] */
  float *action_weights;          /* out [B,A] */
  float *root_value;              /* out [B]: network value of the root (muax/model.py:243) */
  float *search_value;            /* out [B] or NULL: node_values[:,0] after search */
  int32_t *depth_sum;             /* out [B] or NULL: sum over simulations of selection depth */
  const mzs_tree_view *tree;      /* or NULL */
} mzs_act_args;

int mzs_abi_version(void);
const char *mzs_last_error(const mzs_handle *h); /* h may be NULL: last create error */

int mzs_create(const mzs_config *cfg, mzs_handle **out);
int mzs_destroy(mzs_handle *h);

/* ---- fused path: whole act() for the default MLP trio in one launch ---- */
int mzs_mlp_set_weights(mzs_handle *h, const mzs_mlp_weights *w);
int mzs_act_mlp(mzs_handle *h, const mzs_act_args *args, void *stream);

/* ---- the same from HOST memory: what the reference's act() does around its jitted _plan ----
 * muax.MuZero.act takes NumPy observations and returns NumPy / Python values, synchronising on the way out
 * (np.asarray / .item(), muax/model.py:160-179).  mzs_act_mlp_host is that whole round trip in one call: the
 * observations (and optional masks / noise) are copied into pinned memory owned by the handle, which the search kernel
 * reads -- and whose output half it writes -- directly (mapped host memory: no upload / download command), the root
 * noise is drawn on the device from split(key, 3)[1] unless given (mctx.muzero_policy's jax.random.dirichlet, see
 * mzs_dirichlet), and the call returns after synchronising `stream`.  All pointers here are HOST pointers.  (The handle allocates its staging buffers at the
 * first call; this is the only entry point that synchronises.) */
typedef struct {
  int32_t struct_size;
  int32_t draw_dirichlet;              /* muzero policy: 1 = draw the root noise from `key` with dirichlet_alpha */
  const float *obs;                    /* [B, obs_dim] */
  const float *dirichlet_noise;        /* [B, A] or NULL (NULL and draw_dirichlet == 0: no noise, fraction forced to 0) */
  const uint8_t *invalid_actions;      /* [B, A] or NULL */
  uint32_t key[2];
  float dirichlet_fraction, dirichlet_alpha, temperature, reserved0;
  int32_t *action;                     /* out [B] */
  float *action_weights;               /* out [B, A] */
  float *root_value;                   /* out [B] */
} mzs_act_host_args;
int mzs_act_mlp_host(mzs_handle *h, const mzs_act_host_args *args, void *stream);

/* ---- step-wise path: any repr/pred/dyn plugin nets run by the caller ----
 * mzs_root        <- RootFnOutput(prior_logits, value, embedding)  (muax/model.py:258-262)
 * mzs_select      -> (parent embedding, action) for recurrent_fn   (mctx simulate + expand gather)
 * mzs_expand_backup <- RecurrentFnOutput + next embedding            (muax/model.py:276-282)
 * mzs_finish      -> PolicyOutput(action, action_weights)           (mctx summary + categorical)
 * `key` is the act rng_key (host values); used only when tiebreak != 0 or gumbel == NULL. */
int mzs_root(mzs_handle *h, const float *prior_logits, const float *value,
             const float *embedding, const uint8_t *invalid_actions,
             const float *dirichlet_noise, float dirichlet_fraction,
             const uint32_t key[2], void *stream);
/* gumbel policy root: only mctx's invalid-action mask is applied to the logits; `gumbel` [B,A] is
 * the root Gumbel noise or NULL to draw gumbel_scale * jax.random.gumbel(split(key)[1], [B,A]). */
int mzs_root_gumbel(mzs_handle *h, const float *prior_logits, const float *value,
                    const float *embedding, const uint8_t *invalid_actions,
                    const float *gumbel, const uint32_t key[2], void *stream);
int mzs_select(mzs_handle *h, int32_t sim, int32_t *action_out,
               float *parent_embedding_out, void *stream);
int mzs_expand_backup(mzs_handle *h, int32_t sim, const float *reward,
                      const float *discount, const float *prior_logits,
                      const float *value, const float *next_embedding, void *stream);
/* mzs_expand_backup(sim) and mzs_select(sim + 1) in ONE launch (the workgroup that refreshed the root's cached
 * decision performs the next simulate() and gathers its parent's embedding row): one launch and one kernel boundary
 * fewer per simulation of a launch-bound loop.  After the last simulation only the expand + backward half runs and the
 * outputs are left untouched.  The caller must not call mzs_select for sim + 1 afterwards.  Same results as the two
 * separate calls, bit for bit. */
int mzs_expand_backup_select(mzs_handle *h, int32_t sim, const float *reward,
                             const float *discount, const float *prior_logits,
                             const float *value, const float *next_embedding,
                             int32_t *next_action_out, float *next_parent_embedding_out,
                             void *stream);
int mzs_finish(mzs_handle *h, float temperature, const float *gumbel,
               int32_t *action_out, float *action_weights_out,
               float *search_value_out, int32_t *depth_sum_out, void *stream);
int mzs_tree_export(mzs_handle *h, const mzs_tree_view *out, void *stream);

/* ---- step-wise path, stochastic policy (policy == 2): mctx.stochastic_muzero_policy with caller-run decision and chance
 * functions.  A = num_actions, C = num_chance_outcomes; the search is the MuZero search above over A' = A + C slots per
 * node (slots < A: actions, slots >= A: chance outcomes) -- same pUCT rule, qtransform_by_parent_and_siblings, key chain,
 * backup, max_depth and re-expansion -- with these differences:
 *   kind       the root and every even-depth node are decision nodes, odd-depth nodes chance nodes; max_depth and depth_sum
 *              count both kinds of level
 *   root       Dirichlet mix and invalid-action mask over the A actions as in mzs_root, the row then padded with C logits
 *              of -inf, the invalid mask with C ones
 *   selection  decision node: the MuZero rule over all A' slots (tie-break uniforms of length A'; chance slots have prior
 *              probability 0 and are not special-cased); chance node: slot i scores p_i / (visits_i + 1), p the softmax of
 *              the node's prior row, fp32, no noise, first maximum.  The key chain advances one split per level
 *   expansion  child of a decision node: a chance node, prior row [-inf x A, chance_logits], value afterstate_value, edge
 *              reward 0 and discount 1, the afterstate embedding; child of a chance node: a decision node, prior row
 *              [action_logits, -inf x C], value / reward / discount of the chance function, the state embedding.  Both
 *              embeddings live zero-padded in rows of embed_dim = max(state_embed_dim, afterstate_embed_dim) floats
 *   finish     visit summary and the categorical sample over the first A slots; action_weights [B, A]; the Gumbel row is
 *              drawn for shape [B, A]; search_value is the root's node value
 * The trees are walked level by level (no cached decisions).  The entries above refuse a stochastic handle and these refuse
 * any other; mzs_tree_export copies the A'-wide arrays ([B, N, A + C]). */
typedef struct {
  int32_t struct_size;                /* = sizeof(mzs_stochastic_outputs) */
  int32_t reserved0;
  /* decision function, evaluated at action clamp(slot, 0, A - 1) on the parent's first state_embed_dim floats */
  const float *chance_logits;         /* [B, C] */
  const float *afterstate_value;      /* [B] */
  const float *afterstate_embedding;  /* [B, afterstate_embed_dim] */
  /* chance function, evaluated at outcome clamp(slot - A, 0, C - 1) on the parent's first afterstate_embed_dim floats */
  const float *action_logits;         /* [B, A] */
  const float *value, *reward, *discount; /* [B] */
  const float *state_embedding;       /* [B, state_embed_dim] */
} mzs_stochastic_outputs;
/* prior_logits, invalid_actions, dirichlet_noise: [B, A]; embedding: [B, state_embed_dim] */
int mzs_root_stochastic(mzs_handle *h, const float *prior_logits, const float *value, const float *embedding,
                        const uint8_t *invalid_actions, const float *dirichlet_noise, float dirichlet_fraction,
                        const uint32_t key[2], void *stream);
/* slot_out [B]: the selected slot in [0, A + C); parent_is_decision_out [B]: 1 where the selected edge leaves a decision
 * node (the decision function's outputs will be used), 0 a chance node; parent_embedding_out [B, embed_dim] */
int mzs_select_stochastic(mzs_handle *h, int32_t sim, int32_t *slot_out, int32_t *parent_is_decision_out,
                          float *parent_embedding_out, void *stream);
/* Both functions' outputs for every root; per root the kernel takes the set of the selected edge's parent kind */
int mzs_expand_backup_stochastic(mzs_handle *h, int32_t sim, const mzs_stochastic_outputs *outputs, void *stream);
/* gumbel: [B, A] or NULL (drawn from the key given to mzs_root_stochastic); action_weights_out: [B, A] */
int mzs_finish_stochastic(mzs_handle *h, float temperature, const float *gumbel, int32_t *action_out,
                          float *action_weights_out, float *search_value_out, int32_t *depth_sum_out, void *stream);

/* ---- the default stochastic MLP family evaluated by the library: the decision and the chance function between
 * mzs_select_stochastic and mzs_expand_backup_stochastic in ONE launch (muax_amd/csrc/mz_stoch_mlp.cuh) ----
 * Every head is Linear(16)-elu-Linear, haiku layout w[in][out], float32 device pointers; E = embed_dim =
 * state_embed_dim = afterstate_embed_dim, A = num_actions, C = num_chance_outcomes, F = 2 * support_size + 1.
 *   decision function  as = min_max_normalize(ad([s, onehot(a, A)])); afterstate value = decode(av(as)); chance logits = ac(as)
 *   chance function    reward = decode(cr([as, onehot(c, C)])); s' = min_max_normalize(cn([as, onehot(c, C)]));
 *                      value = decode(pv(s')); action logits = pp(s'); discount = the constant below
 * decode = support_to_scalar(softmax(.)); the arithmetic is the "MZ-F32" spec of the default trio. */
typedef struct mzs_stochastic_mlp_weights {
  int32_t struct_size;        /* = sizeof(mzs_stochastic_mlp_weights) */
  int32_t support_size;       /* 8 .. 31 */
  float discount;
  float reserved0;
  const float *ad_w1, *ad_b1, *ad_w2, *ad_b2; /* afterstate dynamics [E+A,16] [16] [16,E] [E] */
  const float *av_w1, *av_b1, *av_w2, *av_b2; /* afterstate value    [E,16]   [16] [16,F] [F] */
  const float *ac_w1, *ac_b1, *ac_w2, *ac_b2; /* chance logits       [E,16]   [16] [16,C] [C] */
  const float *cr_w1, *cr_b1, *cr_w2, *cr_b2; /* chance reward       [E+C,16] [16] [16,F] [F] */
  const float *cn_w1, *cn_b1, *cn_w2, *cn_b2; /* chance next state   [E+C,16] [16] [16,E] [E] */
  const float *pv_w1, *pv_b1, *pv_w2, *pv_b2; /* prediction value    [E,16]   [16] [16,F] [F] */
  const float *pp_w1, *pp_b1, *pp_w2, *pp_b2; /* prediction policy   [E,16]   [16] [16,A] [A] */
} mzs_stochastic_mlp_weights;
/* Binds the weights to a stochastic handle (policy 2) whose two embeddings are both embed_dim wide.  Refused, with the
 * limit named: any other handle, num_actions + num_chance_outcomes > 64, support_size outside 8 .. 31, an LDS need
 * beyond a workgroup's.  The arrays stay the caller's and are read at every mzs_mlp_stochastic_recurrent. */
int mzs_mlp_set_stochastic_weights(mzs_handle *h, const mzs_stochastic_mlp_weights *w);
/* slot, parent_is_decision [B], parent_embedding [B, embed_dim]: what mzs_select_stochastic wrote.  Per root ONLY the
 * function of the parent's kind is evaluated -- decision parent: at action clamp(slot, 0, A - 1), chance parent: at
 * outcome clamp(slot - A, 0, C - 1) -- and only that function's rows of `outputs` (the arrays of mzs_stochastic_outputs,
 * WRITTEN here) are stored; the rows of the other kind are left untouched, mzs_expand_backup_stochastic does not read
 * them.  One launch on `stream`, nothing else: the loop stays capturable.  Needs no rooted tree. */
int mzs_mlp_stochastic_recurrent(mzs_handle *h, const int32_t *slot, const int32_t *parent_is_decision,
                                 const float *parent_embedding, const mzs_stochastic_outputs *outputs, void *stream);

/* ---- the WHOLE stochastic search of the bound family in ONE launch, the tree in LDS (muax_amd/csrc/mz_stoch_wide.cuh):
 * what mzs_root_stochastic, num_simulations x (mzs_select_stochastic, mzs_mlp_stochastic_recurrent,
 * mzs_expand_backup_stochastic) and mzs_finish_stochastic compute, bit for bit, one root per wavefront.
 * Limits (mzs_mlp_stochastic_plan): num_actions + num_chance_outcomes <= 64, embed_dim <= 64 = both embedding widths,
 * support_size 8..31, num_simulations <= 255, one root's tree within the 160 KiB of a CU's LDS. */
/* The kernel's LDS plan for a shape (host arithmetic, no device needed): out = {roots (wavefronts) per workgroup, LDS
 * bytes per workgroup, resident roots per CU, 1 when the embeddings are kept in LDS}; MZS_E_UNSUPPORTED when the kernel
 * declines the shape, MZS_E_INVALID for a null `out`. */
int mzs_mlp_stochastic_plan(int32_t num_actions, int32_t num_chance_outcomes, int32_t embed_dim, int32_t support_size,
                            int32_t num_simulations, int32_t out[4]);
typedef struct mzs_stochastic_search_args {
  int32_t struct_size;             /* = sizeof(mzs_stochastic_search_args) */
  int32_t export_tree;             /* 1: the finished tree into the handle's HBM tree arrays, for mzs_tree_export; 0: they
                                      are not touched */
  const float *prior_logits;       /* [B, A]  RootFnOutput, as mzs_root_stochastic takes it */
  const float *value;              /* [B] */
  const float *embedding;          /* [B, embed_dim] */
  const uint8_t *invalid_actions;  /* [B, A] or NULL */
  const float *dirichlet_noise;    /* [B, A] or NULL (then dirichlet_fraction must be 0) */
  const float *gumbel;             /* [B, A] or NULL: the categorical's Gumbel row drawn from `key` */
  uint32_t key[2];                 /* the act rng_key (HOST values) */
  float dirichlet_fraction;
  float temperature;
  /* NULL, or a DEVICE array of 4 + 2 num_simulations words that REPLACES key, temperature and dirichlet_fraction: a
   * captured launch freezes this struct's values, not the array's contents (mzs_stochastic_search_block fills a host copy;
   * mzs_mlp_stochastic_search_draw reads three words more: mzs_stochastic_search_block_draw) */
  const uint32_t *device_block;
  int32_t *action;                 /* out [B] */
  float *action_weights;           /* out [B, A] */
  float *search_value;             /* out [B] or NULL: the root's node value after the search */
  int32_t *depth_sum;              /* out [B] or NULL: sum over simulations of the selection depth, both kinds of level */
} mzs_stochastic_search_args;
/* One launch on `stream`, nothing else: capturable, no synchronisation, no copy to the host (the first call of a handle
 * that exports a tree, or whose plan keeps the embeddings in HBM, allocates).  Needs mzs_mlp_set_stochastic_weights.
 * Refused before any launch, the message (mzs_last_error) naming the limit: MZS_E_INVALID for a handle of another policy,
 * unbound weights, a null or mis-sized struct, a null required pointer (prior_logits, value, embedding, action,
 * action_weights); MZS_E_UNSUPPORTED for a shape the plan declines or embedding widths that differ. */
int mzs_mlp_stochastic_search(mzs_handle *h, const mzs_stochastic_search_args *args, void *stream);
/* HOST arithmetic: the 4 + 2 num_simulations words of `device_block` for (key, temperature, dirichlet_fraction) into
 * out_words -- k_sample[2], the two floats' bits, every simulation's key.  key NULL: zero. */
int mzs_stochastic_search_block(const uint32_t key[2], int32_t num_simulations, float temperature, float dirichlet_fraction,
                                uint32_t *out_words);

/* ---- root inference of the bound family evaluated by the library (muax_amd/csrc/mz_stoch_wide.cuh): the default
 * Representation, s = min_max_normalize(obs @ repr_w + repr_b), then value = decode(pv(s)), prior logits = pp(s) with the
 * heads bound by mzs_mlp_set_stochastic_weights -- RootFnOutput without a torch module.  Arithmetic "MZ-F32": the fma chain
 * over the observation in index order from 0, the bias last; one root per wavefront, embed_dim <= 64. ----
 * Binds the representation's weights, float32 device pointers repr_w [obs_dim, embed_dim] and repr_b [embed_dim], haiku
 * layout; any obs_dim >= 1.  They take no LDS (read from global memory once per root): mzs_mlp_stochastic_plan does not
 * change.  The arrays stay the caller's and are read at every launch.  MZS_E_INVALID for a handle of another policy,
 * obs_dim < 1, a null array. */
int mzs_mlp_set_stochastic_representation(mzs_handle *h, int32_t obs_dim, const float *repr_w, const float *repr_b);
/* obs [B, obs_dim] -> prior_logits_out [B, A], value_out [B], embedding_out [B, embed_dim], what mzs_root_stochastic takes.
 * One launch on `stream`, no LDS tree, capturable.  Refused before the launch, the message naming the cause: MZS_E_INVALID
 * for a handle of another policy, weights or representation not bound, a null obs or output; MZS_E_UNSUPPORTED for
 * embed_dim > 64 (and what mzs_mlp_set_stochastic_weights refuses). */
int mzs_mlp_stochastic_root(mzs_handle *h, const float *obs, float *prior_logits_out, float *value_out,
                            float *embedding_out, void *stream);
/* mzs_mlp_stochastic_search with the root inference inside the launch: obs [B, obs_dim] replaces the RootFnOutput arrays
 * of `args`, whose prior_logits, value and embedding must be NULL; root_value_out [B] receives the root's network value,
 * node 0's embedding is exported with export_tree.  Bit for bit mzs_mlp_stochastic_root followed by
 * mzs_mlp_stochastic_search.  Everything else as there: one launch, capturable, device_block honoured, the same plan.
 * Refused before any launch: MZS_E_INVALID for a handle of another policy, weights or representation not bound, a null or
 * mis-sized struct, a null obs, root_value_out, action or action_weights, a non-null root array in `args`;
 * MZS_E_UNSUPPORTED for a shape the plan declines. */
int mzs_mlp_stochastic_search_obs(mzs_handle *h, const mzs_stochastic_search_args *args, const float *obs,
                                  float *root_value_out, void *stream);

/* ---- the root exploration noise drawn INSIDE the one launch: each root's wavefront draws its own row of
 *   jax.random.dirichlet(split(args->key, 3)[1], full([num_actions], dirichlet_alpha), (global_batch,))
 * in front of its search, bit for bit the row mzs_dirichlet writes (rows indexed by the GLOBAL root: shards draw their
 * own), mixes it in with args->dirichlet_fraction and, when noise_out [B, A] (device) is not NULL, stores it there.  No
 * separate launch, no [B, A] input array: args->dirichlet_noise must be NULL.
 * obs == NULL: the root comes from the RootFnOutput arrays of `args`, as in mzs_mlp_stochastic_search.  obs != NULL: as
 * mzs_mlp_stochastic_search_obs, the root arrays must be NULL and root_value_out is required.
 * args->device_block, when not NULL, is read in the longer layout of mzs_stochastic_search_block_draw: a captured launch
 * then freezes none of key, temperature, dirichlet_fraction or dirichlet_alpha.  One launch, capturable, the same plan.
 * Refused before any launch, the message naming the cause: MZS_E_INVALID for a non-null dirichlet_noise, dirichlet_alpha
 * <= 0 or not finite, and what the two entries above refuse (another policy, unbound weights or representation, a null
 * or mis-sized struct, a null required pointer, a root array beside obs); MZS_E_UNSUPPORTED for a shape the plan
 * declines. */
int mzs_mlp_stochastic_search_draw(mzs_handle *h, const mzs_stochastic_search_args *args, const float *obs,
                                   float *root_value_out, float dirichlet_alpha, float *noise_out, void *stream);
/* HOST arithmetic: the 7 + 2 num_simulations words of that device_block -- the 4 + 2 num_simulations words of
 * mzs_stochastic_search_block for the same arguments, then the Dirichlet key split(key, 3)[1] (two words) and the bits of
 * dirichlet_alpha.  key NULL: zero. */
int mzs_stochastic_search_block_draw(const uint32_t key[2], int32_t num_simulations, float temperature,
                                     float dirichlet_fraction, float dirichlet_alpha, uint32_t *out_words);

/* ---- recurrent_fn of the EfficientZero-style nets ----
 * mzs_ez_recurrent evaluates, for a batch of 6x6xC hidden states (NHWC, C = 32 or 64) and actions, the whole
 * MuZero._recurrent_inference (muax/model.py:265-282) of EZDynamic + EZPrediction with use_v2 = True
 * (muax/nn.py:221-309, pre-activation blocks muax/nn.py:151-178) in ONE launch: next state, reward and value as
 * support_to_scalar(softmax(logits)), prior logits.  Weights, caller-owned device arrays:
 *   LayerNorm       [2][channels]                  scale row, offset row
 *   3x3 convolution [9][Cin / 16][4][C][4]         Wp[tap][c][g][co][i] = W[tap][16 c + 4 g + i][co] from haiku's
 *                                                  HWIO w[kh][kw][in][out] (the layout of mzs_resnet_tower); the
 *                                                  dynamics' first convolution has C + 1 inputs (last: the action
 *                                                  plane), zero-padded to Cin = C + 16
 *   head            ln_in [2][C], c1 [C][16] (1x1 conv), ln_mid [2][16], fc [576][32] (no bias), ln_vec [2][32],
 *                   out_w [32][n], out_b [n] with n = 2 support_size + 1 (reward, value) or num_actions (policy) */
typedef struct mzs_ez_head {
  const float *ln_in, *c1, *ln_mid, *fc, *ln_vec, *out_w, *out_b;
} mzs_ez_head;
typedef struct mzs_ez_args {
  int32_t struct_size;     /* = sizeof(mzs_ez_args) */
  int32_t device;
  int32_t batch;
  int32_t channels;        /* C: 32 or 64 */
  int32_t num_actions;     /* <= 64 */
  int32_t support_size;    /* 2 support_size + 1 <= 64 */
  const float *x;          /* [B, 6, 6, C] */
  const int32_t *action;   /* [B]; the plane holds the raw index (muax/nn.py:291-296) */
  float *y;                /* [B, 6, 6, C] next state out */
  float *reward;           /* [B] out */
  float *value;            /* [B] out */
  float *prior_logits;     /* [B, A] out */
  const float *d_ln_in, *d_conv;                       /* EZDynamic: LN before the action conv, the conv */
  const float *d_ln0, *d_conv0, *d_ln1, *d_conv1;      /* ... its residual block */
  const float *p_ln0, *p_conv0, *p_ln1, *p_conv1;      /* EZPrediction's residual block */
  mzs_ez_head r, v, p;                                 /* reward / value / policy heads */
} mzs_ez_args;
int mzs_ez_recurrent(const mzs_ez_args *a, void *stream);

/* ---- fused LayerNorm of the convolutional plugin nets ----
 * y = [relu]( LN(x) [+ LN2(x2)] [+ residual] ) with LN(x) = (x - mean) * rsqrt(var + eps) * scale[c] + offset[c],
 * statistics over ALL n elements of a sample (biased variance), scale / offset indexed by (element % channels):
 * hk.LayerNorm(axis=(-3,-2,-1), create_scale=True, create_offset=True) of NHWC tensors followed by the shortcut
 * addition and relu of ResidualConvBlockV1/V2 and of the EZ heads (muax/nn.py:118-178, 232-288) -- the chains between
 * the convolutions of the plugin nets' root inference, two launches instead of ~10 framework kernels each.
 * Inference only (no gradients).  All tensors fp32, contiguous, caller-owned; `workspace` >=
 * mzs_layernorm_workspace_bytes(batch, n) bytes of device memory, overwritten. */
typedef struct mzs_layernorm_args {
  int32_t struct_size;   /* = sizeof(mzs_layernorm_args) */
  int32_t device;
  int32_t batch;         /* samples */
  int32_t n;             /* elements per sample (H*W*C), multiple of 4 and of channels */
  int32_t channels;      /* C, multiple of 4 */
  int32_t relu;          /* 1: relu at the end */
  float eps;             /* haiku: 1e-5 */
  const float *x, *scale, *offset;      /* [batch, n], [C], [C] */
  const float *x2, *scale2, *offset2;   /* optional second normalised tensor (projected shortcut), or NULL */
  const float *residual;                /* optional plain tensor added (identity shortcut), or NULL */
  float *y;                             /* [batch, n]; may alias x, x2 or residual */
  void *workspace;
  int64_t workspace_bytes;
} mzs_layernorm_args;
int mzs_layernorm_act(const mzs_layernorm_args *a, void *stream);
int64_t mzs_layernorm_workspace_bytes(int32_t batch, int32_t n);

/* ---- device self-test ----
 * Three places of the kernels replace a library sequence by a shorter one that is only valid for this hardware's
 * v_sqrt_f32 / v_rcp_f32 / fma: sqrt on arguments that need no range scaling, division by 2 eps = 0.002f
 * (muax/utils.py:70-76), and the support decode's e_i / sum with one refined reciprocal per sum.  mzs_selftest compares
 * them with the IEEE operations on the device -- exhaustively over [1, 4) resp. 2^-9 .. 2^-2, over 2^24
 * denominators in [1, 64) with twelve numerators each, and over 2^24 denominators in 2^-27 .. 2^41 with eight -- and
 * returns the mismatch counts (all must be 0) in mismatches[0..3].  Synchronous.  errors: mzs_last_error(NULL) */
int mzs_selftest(int32_t device, int64_t *mismatches);

/* ---- root exploration noise ----
 * rows [root_offset, root_offset + batch) of what mctx.muzero_policy draws for a `global_batch`-root act:
 *   jax.random.dirichlet(split(rng_key, 3)[1], alpha = full([num_actions], dirichlet_alpha), shape = (global_batch,))
 * (policy call site muax/policy.py:18-30, defaults muax/model.py:92-93), into out [batch, num_actions] on the
 * device.  `key` is the DIRICHLET sub-key (host values).  Restated from jax's published sampler on the exact
 * threefry key walk; float bits are spec-to-confirm against a real jax (oracle/mz_oracle.c): inject an array
 * through mzs_act_args.dirichlet_noise / mzs_root for bit-pinned noise.  errors: mzs_last_error(NULL) */
int mzs_dirichlet(int32_t device, const uint32_t key[2], float alpha, int32_t batch, int32_t num_actions,
                  int64_t global_batch, int64_t root_offset, float *out, void *stream);

/* ---- training step of the default MLP trio ----
 * mzs_mlp_loss_grad replaces jax.value_and_grad(loss_fn) at muax/model.py:245-249 with the default
 * loss (muax/loss.py:10-88): for a batch of k-step trajectories it returns the scalar loss and the
 * gradient of every one of the 18 weight arrays, concatenated in the member order of mzs_mlp_weights
 * (repr_w, repr_b, pv_w1, ... dn_b2), each in its own haiku layout.  One fused forward+backward kernel
 * and a fixed-order reduction: bit-reproducible run to run.  The optimiser (muax/optimizers.py) and the
 * optional data-parallel gradient mean (one flat all-reduce over `grads`) stay with the caller.
 * Limits: obs_dim 1..128 (MZS_E_UNSUPPORTED above, the limit named); the (num_actions, embed_dim, 2 support_size + 1)
 * triple must have a kernel instance, a listed one (num_actions <= 16) or one registered through
 * mzs_register_train_dispatch (num_actions <= 64), else MZS_E_UNSUPPORTED "no kernel instance for this (A, E, F)";
 * unroll_steps beyond what the instance's LDS keeps is refused on the host, before any launch, the limit named. */
typedef struct mzs_train_args {
  int32_t struct_size;      /* = sizeof(mzs_train_args) */
  int32_t device;
  int32_t batch;            /* B trajectories */
  int32_t unroll_steps;     /* L = k_steps (muax/replay_buffer.py:192-240 batch layout [B, L, ...]) */
  int32_t num_actions;
  int32_t embed_dim;
  const float *obs;         /* [B, obs_dim]  batch.obs[:, 0] */
  const int32_t *actions;   /* [B, L] */
  const float *rewards;     /* [B, L]   batch.r  */
  const float *returns;     /* [B, L]   batch.Rn */
  const float *policy;      /* [B, L, A] batch.pi */
  float loss_scale;         /* 1/B (muax/loss.py) or 1/(B L) (frameworks/coax/loss.py:70-71) */
  float l2_coeff;           /* 1e-4 (muax/loss.py:84-87) */
  float *loss;              /* [1] out */
  float *grads;             /* [mzs_mlp_num_params] out */
  void *workspace;          /* >= mzs_mlp_train_workspace_bytes(...) */
  int64_t workspace_bytes;
} mzs_train_args;
int64_t mzs_mlp_num_params(int32_t obs_dim, int32_t embed_dim, int32_t num_actions, int32_t support_size);
int64_t mzs_mlp_train_workspace_bytes(int32_t batch, int32_t obs_dim, int32_t embed_dim,
                                      int32_t num_actions, int32_t support_size);
/* errors: mzs_last_error(NULL) */
int mzs_mlp_loss_grad(const mzs_mlp_weights *w, const mzs_train_args *a, void *stream);
/* The same step with a weight per batch row (importance sampling of prioritised replay):
 * sample_weight [B] float32 on the device multiplies the three cross entropies of row j at EVERY unroll step --
 *   loss = sum_j loss_scale * sample_weight[j] * sum_i (CE_r + CE_v + CE_pi)(j, i)  +  l2_coeff * 0.5 * sum ||w||^2
 * -- and with them the row's whole gradient; the L2 term is not weighted.  Same kernels, same instances (listed or
 * registered), same workspace, same limits and errors as the unweighted entry, reported under its name; weights of 1
 * give its bits.  The values are not inspected: a weight of 0 makes the row contribute exact zeros while its data is
 * finite.  A null sample_weight is MZS_E_INVALID.  errors: mzs_last_error(NULL) */
int mzs_mlp_loss_grad_weighted(const mzs_mlp_weights *w, const mzs_train_args *a, const float *sample_weight,
                               void *stream);

/* ---- training step of the default stochastic MLP family (muax_amd/csrc/mz_stoch_train.cuh) ----
 * Loss and gradients of muax_amd/loss.py::stochastic_loss_fn for the six modules of
 * nn.create_stochastic_muzero_network: step 0 contributes CE(v_0, Rn_0) + CE(pi_0, pi_0); transition i = 1 .. L-1, with
 * action a_{i-1} and the chance code c_i = argmax encoder(obs_i) (the lowest index among equal maxima),
 *   CE(r, r_{i-1}) + CE(v_i, Rn_i) + CE(pi_i, pi_i) + CE(chance logits, onehot(c_i)) + CE(afterstate value, Rn_{i-1})
 *   + vqvae_beta * mean_C (encoder(obs_i) - onehot(c_i))^2,
 * every term times loss_scale (times sample_weight[row] when given), plus l2_coeff * 0.5 * sum ||w||^2 over all 34
 * arrays.  The gradient is one flat vector in the member order of mzs_stochastic_train_weights.  Two launches on
 * `stream` that only enqueue (capturable), a fixed-order reduction: bit-reproducible run to run.
 * The chance dynamics read the exact one-hot of c_i where the torch formula computes e + (onehot - e) in floating
 * point (an ulp of the input apart).
 * Refusals, all before any launch: a null pointer or a struct size mismatch, a workspace below
 * mzs_stochastic_mlp_train_workspace_bytes (MZS_E_INVALID); obs_dim beyond 32, support_size outside 8 .. 31, an
 * (A, C, E, F) without a listed kernel instance ("no kernel instance"), unroll_steps beyond what the instance keeps in
 * LDS ("too large for the LDS", the limit named) (MZS_E_UNSUPPORTED).  An instance registered with
 * mzs_register_stochastic_train_dispatch serves its own (A, C, E, F) up to its own observation cap (at most 128); the
 * lookup comes before the obs_dim refusal, and with nothing registered every answer is the one above. */
typedef struct mzs_stochastic_train_weights {
  int32_t struct_size;        /* = sizeof(mzs_stochastic_train_weights) */
  int32_t obs_dim;            /* 1 .. 32 (the training entry's listed instances; on-demand ones and mzs_stochastic_mlp_unroll_values: 1 .. 128) */
  int32_t support_size;       /* 8 .. 31 */
  int32_t reserved0;
  const float *repr_w, *repr_b;               /* representation      [obs_dim,E] [E] */
  const float *ad_w1, *ad_b1, *ad_w2, *ad_b2; /* the 28 arrays of mzs_stochastic_mlp_weights, in its order */
  const float *av_w1, *av_b1, *av_w2, *av_b2;
  const float *ac_w1, *ac_b1, *ac_w2, *ac_b2;
  const float *cr_w1, *cr_b1, *cr_w2, *cr_b2;
  const float *cn_w1, *cn_b1, *cn_w2, *cn_b2;
  const float *pv_w1, *pv_b1, *pv_w2, *pv_b2;
  const float *pp_w1, *pp_b1, *pp_w2, *pp_b2;
  const float *en_w1, *en_b1, *en_w2, *en_b2; /* chance encoder      [obs_dim,16] [16] [16,C] [C] */
} mzs_stochastic_train_weights;
typedef struct mzs_stochastic_train_args {
  int32_t struct_size;          /* = sizeof(mzs_stochastic_train_args) */
  int32_t device;
  int32_t batch;                /* B */
  int32_t unroll_steps;         /* L */
  int32_t num_actions;          /* A */
  int32_t num_chance_outcomes;  /* C */
  int32_t embed_dim;            /* E */
  int32_t reserved0;
  const float *obs;             /* [B, L, obs_dim]: an observation for every step */
  const int32_t *actions;       /* [B, L] */
  const float *rewards;         /* [B, L] */
  const float *returns;         /* [B, L] */
  const float *policy;          /* [B, L, A] */
  const float *sample_weight;   /* [B] or NULL (all 1) */
  float loss_scale;             /* 1/B or 1/(B L) */
  float l2_coeff;               /* 1e-4 */
  float vqvae_beta;             /* 0.25 */
  float reserved1;
  float *loss;                  /* [1] out */
  float *grads;                 /* [mzs_stochastic_mlp_num_params] out */
  void *workspace;              /* >= mzs_stochastic_mlp_train_workspace_bytes(...) */
  int64_t workspace_bytes;
} mzs_stochastic_train_args;
int64_t mzs_stochastic_mlp_num_params(int32_t obs_dim, int32_t embed_dim, int32_t num_actions,
                                      int32_t num_chance_outcomes, int32_t support_size);
int64_t mzs_stochastic_mlp_train_workspace_bytes(int32_t batch, int32_t obs_dim, int32_t embed_dim, int32_t num_actions,
                                                 int32_t num_chance_outcomes, int32_t support_size);
/* errors: mzs_last_error(NULL) */
int mzs_stochastic_mlp_loss_grad(const mzs_stochastic_train_weights *w, const mzs_stochastic_train_args *a, void *stream);

/* ---- next-state tower of the ResNet dynamics net ----
 * mzs_resnet_tower evaluates, for a batch of 6x6x64 hidden states (NHWC, the reference's embedding
 * layout), what muax/nn.py:344-378 calls ns_func followed by min_max_normalize2d: conv1x1 on
 * [s, a / num_actions] + relu, `blocks` x ResidualConvBlockV1(64, stride 1, projection)
 * (muax/nn.py:118-148: 3 x conv3x3 + LayerNorm over (H, W, C)), per-channel min-max normalisation -- one
 * kernel, one workgroup per root, fp32 MFMA.  Weights stay in haiku's layouts:
 *   stem_w  [65][64]                 (hk.Conv2D 1x1, HWIO)  or NULL to skip the stem
 *   conv_w  [blocks][3] convolutions (projection conv, conv_0, conv_1), each haiku HWIO w[3][3][64][64]
 *           re-ordered once by the caller to Wp[tap 9][c 4][g 4][co 64][i 4] = w[tap][16 c + 4 g + i][co]
 *           (one 16-byte load per lane and 4 k-steps)
 *   ln      [blocks][3][2][64]        (scale, offset) of the projection's, ln_0's, ln_1's LayerNorm */
typedef struct mzs_tower_args {
  int32_t struct_size;     /* = sizeof(mzs_tower_args) */
  int32_t device;
  int32_t batch;
  int32_t blocks;
  int32_t normalize;       /* != 0: apply min_max_normalize2d at the end */
  int32_t num_actions;     /* the action plane is a / num_actions */
  const float *x;          /* [B, 6, 6, 64] */
  const int32_t *action;   /* [B] (needed with stem_w) */
  const float *stem_w;
  const float *conv_w;
  const float *ln;
  float *y;                /* [B, 6, 6, 64] out */
  /* Optional heads, fused into the same launch when r_c1 != NULL (then all of them must be given): the
   * whole recurrent_fn of muax/model.py:265-282 for the ResNet nets -- reward head r_func on
   * [s, a / num_actions] (muax/nn.py:347-357) and ResNetPrediction on the normalised next state
   * (muax/nn.py:313-341); reward / value come out as support_to_scalar(softmax(logits)).  haiku layouts:
   * conv1x1 w[in][out], Linear w[in][out] on the NHWC-flattened map, biases [out]. */
  const float *r_c1, *r_c2, *r_l1, *r_b1, *r_l2, *r_b2;   /* [65,64] [64,64] [2304,64] [64] [64,F] [F] */
  const float *v_c1, *v_c2, *v_l1, *v_b1, *v_l2, *v_b2;   /* [64,16] [16,16] [576,16] [16] [16,F] [F] */
  const float *p_c1, *p_l1, *p_b1, *p_l2, *p_b2;          /* [64,16] [576,16] [16] [16,A] [A]        */
  float *reward;           /* [B] out */
  float *value;            /* [B] out */
  float *prior_logits;     /* [B, A] out */
  int32_t support_size;    /* F = 2 * support_size + 1 <= 64 */
  int32_t reserved0;
  /* Optional pair mode for small batches (2 * batch workgroups must be resident at once: batch <= 128):
   * two workgroups per root split the pixels of its map and swap boundary pixels + LayerNorm moments
   * through `pair_scratch` (caller-owned device memory of mzs_tower_pair_scratch_bytes(batch) bytes,
   * ZEROED once when allocated and then left to the library; one scratch per stream).  NULL: one
   * workgroup per root.  Word 4 r + 3 of the trailing uint32 region turns non-zero if root r's halves ever
   * lost each other (bounded spin ran out): results of that launch are then invalid. */
  void *pair_scratch;
  int64_t pair_scratch_bytes;
} mzs_tower_args;
int mzs_resnet_tower(const mzs_tower_args *a, void *stream);
/* bytes of pair_scratch for `batch` roots (0 if pair mode cannot run that batch) */
int64_t mzs_tower_pair_scratch_bytes(int32_t batch);

/* The tail of root inference with those nets (muax/model.py:251-263), one launch: the last hk.AvgPool(3, 2, 'SAME') of
 * ResNetRepresentation (muax/nn.py:308; the mean of the VALID elements under each window) on its [B, H, W, 64] map with
 * H, W in {11, 12} -> 6 x 6, min_max_normalize2d (:47-56, :310; normalize != 0), ResNetPrediction on that embedding
 * (:313-341; weights as in mzs_tower_args) and support_to_scalar(softmax(value logits)) (muax/model.py:254). */
typedef struct mzs_root_tail_args {
  int32_t struct_size;     /* = sizeof(mzs_root_tail_args) */
  int32_t device;
  int32_t batch, height, width;
  int32_t num_actions, support_size, normalize;
  const float *x;          /* [B, H, W, 64] */
  const float *v_c1, *v_c2, *v_l1, *v_b1, *v_l2, *v_b2, *p_c1, *p_l1, *p_b1, *p_l2, *p_b2;
  float *embedding;        /* [B, 6, 6, 64] out */
  float *value;            /* [B] out */
  float *prior_logits;     /* [B, num_actions] out */
} mzs_root_tail_args;
int mzs_resnet_root_tail(const mzs_root_tail_args *a, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * hk.Conv2D(C, kernel_shape=3, stride=1, padding='SAME', with_bias=False) on NHWC maps with C -> C channels, C = 16, 32
 * or 64: the convolutions inside the residual blocks of the representation nets at their 21 x 21 / 11 x 11 / 6 x 6 stages
 * (muax/nn.py:118-178 inside ResNetRepresentation :291-310 and EZStateEncoder :180-207; root inference,
 * muax/model.py:251-263).  fp32 MFMA implicit GEMM (mz_repr.cuh); any height / width whose rows fit a CU's LDS.
 *   w_packed: the HWIO kernel w[3][3][C][C] re-ordered once by the caller to Wp[tap][c][g][co][i] = w[tap][16 c + 4 g + i][co]
 *   (the layout of mzs_resnet_tower's conv_w).  relu != 0: max(., 0) on the way out. */
typedef struct mzs_conv3x3_args {
  int32_t struct_size;     /* = sizeof(mzs_conv3x3_args) */
  int32_t device;
  int32_t batch, height, width, channels;
  int32_t relu, reserved0;
  const float *x;          /* [B, H, W, C] */
  const float *w_packed;   /* 9 * C * C floats */
  float *y;                /* [B, H, W, C] out */
} mzs_conv3x3_args;
int mzs_conv3x3_nhwc(const mzs_conv3x3_args *a, void *stream);

/* The stems of those nets: hk.Conv2D(out, kernel_shape=3, stride=2, padding='SAME', with_bias=False) with (in, out)
 * channels (4, 32) / (4, 16) -- raw frame stacks, muax/nn.py:299 / :189 -- or (32, 64) / (16, 32) (muax/nn.py:303, and
 * the strided convolutions of the EZ encoder's projection block, :151-178 inside :180-207); output
 * [B, ceil(H / 2), ceil(W / 2), out].  w_packed: Wp[tap][c][g][co][i] = w[tap][16 c + 4 g + i][co] with the 4 frame
 * channels padded to 16 by zero rows (9 * 16 * 32 floats).  in_div != 0: the input is divided by it on the way in (the
 * reference's observations / 255); relu != 0: max(., 0) on the way out. */
typedef struct mzs_conv3x3s_args {
  int32_t struct_size;     /* = sizeof(mzs_conv3x3s_args) */
  int32_t device;
  int32_t batch, height, width;   /* of the input */
  int32_t in_channels, out_channels;
  int32_t relu;
  float in_div;
  int32_t reserved0;
  const float *x;          /* [B, H, W, in] */
  const float *w_packed;
  float *y;                /* [B, ceil(H/2), ceil(W/2), out] */
} mzs_conv3x3s_args;
int mzs_conv3x3_stride2_nhwc(const mzs_conv3x3s_args *a, void *stream);

/* A whole ResidualConvBlockV1 (muax/nn.py:118-148: conv_0 - LN - relu - conv_1 - LN, + LN(projection conv) or + x,
 * relu) of those nets, stride 1, C -> C with C = 32 or 64, inference, in three launches: the projection and conv_0
 * share one pass over the input and leave the moments of their outputs, conv_1 normalises its input on the way into
 * LDS, one streaming pass applies the last LayerNorm(s), the shortcut and the relu (mz_repr.cuh, mz_norm.cuh).
 *   w_proj / w0 / w1: packed kernels as for mzs_conv3x3_nhwc; w_proj NULL = identity shortcut (y = relu(LN1(.) + x)).
 *   workspace >= mzs_resblock_workspace_bytes(...) bytes of device memory, overwritten; y must not alias x. */
typedef struct mzs_resblock_args {
  int32_t struct_size;     /* = sizeof(mzs_resblock_args) */
  int32_t device;
  int32_t batch, height, width, channels;
  float eps;               /* haiku: 1e-5 */
  int32_t reserved0;
  const float *x;          /* [B, H, W, C] */
  const float *w_proj, *w0, *w1;
  const float *proj_scale, *proj_offset;   /* [C] each; NULL with w_proj NULL */
  const float *ln0_scale, *ln0_offset, *ln1_scale, *ln1_offset;
  float *y;                /* [B, H, W, C] out */
  void *workspace;
  int64_t workspace_bytes;
} mzs_resblock_args;
int mzs_resblock_v1(const mzs_resblock_args *a, void *stream);
int64_t mzs_resblock_workspace_bytes(int32_t batch, int32_t height, int32_t width, int32_t channels);

/* A whole ResidualConvBlockV2 (muax/nn.py:151-178: the pre-activation block of the EfficientZero-style encoder,
 * muax/nn.py:180-207) with the identity shortcut, stride 1, C -> C with C = 16, 32 or 64, inference, in three launches:
 *     y = x + conv_1(relu(LN_1(conv_0(relu(LN_0(x))))))
 * fp64 moments of x; conv_0 normalising x on its way into LDS and leaving the moments of its outputs; conv_1
 * normalising those on the way in and adding x in its epilogue.  Same argument block as mzs_resblock_v1 with
 * w_proj / proj_scale / proj_offset NULL (the reference's projection block of this kind is strided: single calls);
 * workspace >= mzs_resblock_v2_workspace_bytes(...); y must not alias x. */
int mzs_resblock_v2(const mzs_resblock_args *a, void *stream);
int64_t mzs_resblock_v2_workspace_bytes(int32_t batch, int32_t height, int32_t width, int32_t channels);

/* ------------------------------------------------------------------------------------------------------------
 * Fused-kernel instances built on demand.
 *
 * mzs_act_mlp serves the (num_actions, embedding_dim, support_size, num_simulations) shapes compiled into the library
 * (muax_amd/csrc/mz_instances.def) and returns MZS_E_UNSUPPORTED for others, although the reference's act() takes any
 * (muax/model.py:82-96).  A host that has hipcc can close the gap at run time: compile muax_amd/csrc/mz_fused_jit.hip for
 * the missing shape into a side library (muax_amd/_jit.py does), dlopen it and pass its
 * two entry points (the values of `mzs_jit_dispatch` and `mzs_jit_abi`) here; later mzs_act_mlp calls (any handle) try the registered instances after the
 * built-in ones.  `jit_abi` must equal mzs_fused_jit_abi() (same kernel-argument layout). */
int mzs_register_fused_dispatch(void *dispatch, int32_t jit_abi);
/* Round 6: an instance compiled with -DMZ_FUSED_MUZERO_ONLY=1 serves the MuZero policy's modes alone (its record has four
 * words per child instead of the Gumbel modes' five: more roots per workgroup, muax_amd/_jit.py::plan(gumbel=False)) and
 * declines a Gumbel handle.  Registered here it is tried BEFORE the instances registered with the call above, so that a
 * MuZero-policy handle takes it even when an all-modes instance of the same shape is present. */
int mzs_register_fused_dispatch_muzero(void *dispatch, int32_t jit_abi);
int mzs_fused_jit_abi(void);
/* The same for the training step (round 5): mzs_mlp_loss_grad carries mz_train_kernel for a list of (num_actions,
 * embedding_dim, 2 support_size + 1) triples and returns MZS_E_UNSUPPORTED for others, although the reference's
 * update() takes whatever widths its nets have (muax/model.py:181-201).  muax_amd/csrc/mz_train_jit.hip compiled for
 * the missing triple gives a side library whose `mzs_jit_train_launch` is passed here together with its
 * `mzs_jit_train_shape` values and the value of its `mzs_jit_train_abi` (must equal mzs_train_jit_abi(): same argument
 * layout); later
 * mzs_mlp_loss_grad calls of that triple take it.  The kernel's own limits bound what can be built: embed_dim 1..64,
 * 2 support_size + 1 in 17..63, num_actions 1..16, or 17..64 when the translation unit is compiled with
 * -DMZ_TRAIN_WIDE=1 (policy head over ceil(num_actions / 16) lane slots; muax_amd/_jit.py::ensure_wide_train_instance).
 * Wide shapes exist as on-demand instances only: the library lists none. */
int mzs_register_train_dispatch(void *launch, int32_t num_actions, int32_t embed_dim, int32_t full_support_size, int32_t jit_abi);
int mzs_train_jit_abi(void);
/* ... and for the training step of the default stochastic MLP family: mzs_stochastic_mlp_loss_grad lists four
 * (A, C, E, F = 2 support_size + 1) tuples at an observation cap of 32.  muax_amd/csrc/mz_stoch_train_jit.hip compiled
 * for another tuple and an observation cap of 32, 64, 96 or 128 gives a side library whose `mzs_jit_stoch_train_launch`
 * is passed here with its `mzs_jit_stoch_train_shape` values and the value of its `mzs_jit_stoch_train_abi` (must equal
 * mzs_stochastic_train_jit_abi(): the argument block over 34 arrays).  Later mzs_stochastic_mlp_loss_grad calls of that
 * tuple with obs_dim <= obs_cap take it (the smallest sufficient cap when several are registered), after the listed
 * instances; an unroll beyond the instance's own LDS plan is still refused ("too large for the LDS", its limit named).
 * The kernel's limits bound what can be built: num_actions 1..16, num_actions + num_chance_outcomes <= 64,
 * embed_dim 1..64, F in 17..63 (muax_amd/_jit.py::stochastic_train_plan).  MZS_E_INVALID for a null launcher, another
 * ABI word or an obs_cap that is none of the four. */
int mzs_register_stochastic_train_dispatch(void *launch, int32_t num_actions, int32_t num_chance_outcomes, int32_t embed_dim,
                                           int32_t full_support_size, int32_t obs_cap, int32_t jit_abi);
int mzs_stochastic_train_jit_abi(void);
/* Shapes the fused kernel cannot be instantiated for at all (more than 16 actions, more than 255 simulations, embeddings
 * wider than 64): allow != 0 lets mzs_act_mlp / mzs_act_mlp_host serve them through the generic route instead of
 * returning MZS_E_UNSUPPORTED -- the trio with run-time shapes (num_actions <= 64, support_size 8..31), tree in HBM with
 * cached decisions, ONE launch for all simulations plus root / select / finish launches (mz_mlp_generic.cuh).  Same
 * arithmetic spec, same results bit for bit as an instance would give; several times slower per simulation than a
 * tuned instance, an order of magnitude faster than per-simulation launches with the caller's own nets. */
int mzs_mlp_allow_generic(mzs_handle *h, int32_t allow);
/* 17..64 actions under the MuZero policy: allow != 0 lets mzs_act_mlp / mzs_act_mlp_host serve them with the wide-action
 * kernel (mz_wide.cuh) -- the whole act() in ONE launch like a fused instance, one root per wavefront, one lane per action,
 * the root's tree in LDS, shapes at run time (embed_dim <= 64, support_size 8..31, num_simulations <= 255).  It is tried
 * after the fused instances and before the generic route, and DECLINES (the call goes on as if it were not allowed: the
 * generic route when that is allowed, else MZS_E_UNSUPPORTED) a Gumbel handle (see mzs_mlp_allow_wide_gumbel),
 * num_actions <= 16, support_size outside 8..31, num_simulations > 255 and a shape whose single root does not fit a CU's
 * LDS.  Same results bit for bit as the generic route.  Off by default: a handle that never calls this behaves as before. */
int mzs_mlp_allow_wide(mzs_handle *h, int32_t allow);
/* The same for a handle of the Gumbel policy (both qtransforms, any max_num_considered_actions, root Gumbel noise given or
 * drawn from the key): allow != 0 lets the wide-action kernel serve its 17..64-action shapes -- sequential halving at the
 * root, the deterministic interior selection and the completed-Q transform one lane per action.  A separate switch:
 * mzs_mlp_allow_wide alone leaves a Gumbel handle where it was (generic route or MZS_E_UNSUPPORTED), and this one has no
 * effect on a handle of the MuZero policy.  The record holds the prior logits as well (5 fields per action), so the plan
 * is mzs_mlp_wide_plan_policy(..., 1, ...): fewer resident roots, a smaller largest num_simulations. */
int mzs_mlp_allow_wide_gumbel(mzs_handle *h, int32_t allow);
/* The wide kernel's LDS plan for a shape (host arithmetic, no device): out = {roots (wavefronts) per workgroup, LDS
 * bytes per workgroup, resident roots per CU, 1 when the embeddings are kept in LDS}; MZS_E_UNSUPPORTED when the kernel
 * declines the shape.  Per root (num_simulations + 1) x (4 + 4 num_actions [+ embed_dim] + 1) words, per workgroup the
 * four nets' weights and num_simulations + 2 words; the workgroup size 1..4 that keeps most roots within 160 KiB. */
int mzs_mlp_wide_plan(int32_t num_actions, int32_t embed_dim, int32_t support_size, int32_t num_simulations, int32_t out[4]);
/* ... for a policy: 0 MuZero (what mzs_mlp_wide_plan answers), 1 Gumbel (4 + 5 num_actions words per record);
 * MZS_E_INVALID for another policy or a null `out`. */
int mzs_mlp_wide_plan_policy(int32_t num_actions, int32_t embed_dim, int32_t support_size, int32_t num_simulations,
                             int32_t policy, int32_t out[4]);

/* ------------------------------------------------------------------------------------------------------------
 * The simulation loop of a search with the ResNet nets in ONE launch (mz_search_conv.hip).
 *
 * Replaces, for simulations [sim_begin, sim_end) of a search on handle `h` (rooted with mzs_root / mzs_root_gumbel and
 * with simulate() of `sim_begin` already run: mzs_select(h, sim_begin, ...), or the tail of a previous call), the loop
 *     recurrent_fn (mzs_resnet_tower with heads)  ->  mzs_expand_backup_select                (2 launches per simulation)
 * that mirrors mctx's search loop calling muax's recurrent_fn (muax/model.py:265-282 through muax/policy.py:13-30).
 * Every root is advanced by its own workgroup(s) through all the simulations: the next state is written into the tree's
 * embedding row of the new node, the next pass reads the parent's row in place, reward / value / prior logits stay on
 * the CU.  Same device code as the step-wise entry points, same results bit for bit.
 *
 * `a`: the weights, `num_actions`, `support_size`, `blocks`, `normalize` (must be set), all 17 head arrays and the three
 * per-root output arrays `reward` [B], `value` [B], `prior_logits` [B, A] (used as scratch; they hold the last
 * simulation's values afterwards) of mzs_tower_args; `x`, `y`, `action` are ignored.  `pair_scratch` != NULL: two
 * workgroups per root (batch <= 128), as for mzs_resnet_tower -- check the status words afterwards and repeat the
 * search without it if any is set.  `discount`: the constant muax's recurrent_fn returns (muax/model.py:274).
 * Discount contract: every edge already expanded on the handle must carry the same `discount` as the argument.  The LDS
 * tree build does not store per-edge discounts and applies the argument to existing edges; a tree continued from
 * mzs_expand_backup[_select] calls with other discounts gives results that depend on MZS_SEARCH_LDS_TREE.
 * The handle's embed_dim must be 2304 (6 x 6 x 64) and its tree must use cached decisions (the default whenever
 * batch * (num_simulations + 1)^2 words fit 1 GiB).  Errors: mzs_last_error(h). */
int mzs_resnet_search(mzs_handle *h, const mzs_tower_args *a, float discount, int32_t sim_begin, int32_t sim_end,
                      void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Device-resident trajectory replay (mz_replay.cuh): the buffer of muax/replay_buffer.py:161-262 with
 * its storage on the GPU and a k-step batch sampled in ONE launch, in the layout mzs_mlp_loss_grad reads.
 *
 * Whole episodes lie contiguous in per-field arenas of `max_steps` transitions (caller-owned device memory, as are the
 * two episode tables of `capacity` rows); WHERE an episode goes and which ones are evicted is the caller's bookkeeping
 * (muax_amd/replay_device.py).  No entry point synchronises or copies to the host; errors: mzs_last_error(NULL). */
typedef struct mzs_replay_arena {
  int32_t struct_size;     /* = sizeof(mzs_replay_arena) */
  int32_t device;
  int64_t max_steps;       /* transitions per arena, < 2^31 */
  int32_t capacity;        /* episode table rows */
  int32_t obs_dim, num_actions, reserved0;
  float *obs;              /* [max_steps, obs_dim] */
  int32_t *a;              /* [max_steps] */
  float *r, *Rn, *v;       /* [max_steps] */
  uint8_t *done;           /* [max_steps] */
  float *pi;               /* [max_steps, num_actions] */
  double *w, *cw;          /* [max_steps]: priority weight; its inclusive prefix sum inside the episode */
  int32_t *t_start, *t_len; double *t_w; int64_t *t_serial;   /* [capacity] by table slot: written by the store */
  int32_t *c_start, *c_len; double *c_CW; int64_t *c_serial;  /* [capacity] oldest first: written by the refresh */
} mzs_replay_arena;

/* One add: `episodes` complete episodes, given as one flat stream of `stream_steps` transitions, are copied to their
 * places, the prefix sums `cw` and the table rows written -- one launch, one wavefront per episode.
 *   desc[e] = {first transition in the stream, first transition in the arena, length, table slot}; the HOST copy is
 *   checked here (ranges inside the stream / the arena, slot < capacity), the DEVICE copy is what the kernel reads.
 *   The caller keeps the episodes of one call disjoint in the arena and in the table.
 * raw == 0: r, v are float[stream_steps]; Rn, done, w are given; the episode weights are ep_w (weight_mode 0).
 * raw == 1: r, v are DOUBLE[stream_steps]; Rn, done and w are computed as muax_amd/vector.py:25-52 defines them, in
 *   fp64 and in its operation order: Rn = sum_{i < n_step} gpow[i] * r[t + i] (i ascending, 0 past the end), then
 *   + v[t + n_step] * gpow[n_step] where that step exists (else done = 1); w = |v - Rn| ** alpha, or 1 with
 *   has_alpha == 0; with alpha == 1.0 no pow is executed, so w is exactly |v - Rn| (as in
 *   mzs_replay_update_priorities).  gpow: device table of the n_step + 1 powers gamma ** i the host computed.
 *   weight_mode 1 / 2: the episode weight is the mean / the sum of its w (0: ep_w, as with raw == 0). */
typedef struct mzs_replay_store_args {
  int32_t struct_size;     /* = sizeof(mzs_replay_store_args) */
  int32_t episodes;
  int64_t stream_steps;
  int32_t raw, n_step, weight_mode, has_alpha;
  double alpha;
  const int32_t *desc_host;  /* HOST [episodes][4] */
  const int32_t *desc;       /* [episodes][4] */
  const int64_t *serial;     /* [episodes]: running number of the add that stores the episode */
  const double *ep_w;        /* [episodes], or NULL with weight_mode != 0 */
  const double *gpow;        /* [n_step + 1] (raw) */
  const float *obs;          /* [stream_steps, obs_dim] */
  const int32_t *a;          /* [stream_steps] */
  const float *pi;           /* [stream_steps, num_actions] */
  const void *r, *v;         /* [stream_steps] float (raw == 0) or double (raw == 1) */
  const float *Rn; const uint8_t *done; const double *w;   /* [stream_steps] (raw == 0) */
} mzs_replay_store_args;
int mzs_replay_store(const mzs_replay_arena *arena, const mzs_replay_store_args *a, void *stream);

/* The `count` live episodes from table slot `head` on (slots wrap at capacity), oldest first, into the compact table,
 * with CW = the inclusive fp64 prefix sum, in that order, of the weights of the episodes LONGER than k_steps (the others
 * carry no probability).  One launch; needed after adds / evictions and when k_steps changes. */
int mzs_replay_refresh(const mzs_replay_arena *arena, int32_t head, int32_t count, int32_t k_steps, void *stream);

/* A batch of `batch` k-step windows in one launch, one wavefront per row.  Row j:
 *   u(x0, x1) = ((y0 << 32 | y1) >> 11) * 2^-53 in fp64 with (y0, y1) = threefry2x32(key, x0, x1);
 *   u0 = u(j / sample_per_trajectory, 0), u1 = u(j, 1);
 *   episode e = the first with CW[e] > u0 * CW[count - 1];   m = length(e) - k_steps;
 *   start i = the first i < m with cw[i] > u1 * cw[m - 1], or floor(u1 * m) when cw[m - 1] == 0;
 *   the outputs are transitions i .. i + k_steps - 1 of that episode (obs: transition i alone).
 *   obs_steps == k_steps: obs is [batch, k_steps, obs_dim] and row j holds the observations of transitions
 *   i .. i + k_steps - 1, one contiguous run of the arena copied in the same launch from the same draw and searches
 *   (the layout mzs_stochastic_mlp_loss_grad reads); every other output, and obs[j][0], has the bits of obs_steps == 0.
 *   obs_steps == 0: obs is [batch, obs_dim] as above.  Any other value is MZS_E_INVALID before any launch, as is
 *   k_steps * obs_dim >= 2^31 with obs_steps set.
 * With every weight zero (CW[count - 1] == 0: the caller's error) the draw lands on the newest episode; a row whose
 * episode is no longer than k_steps is zero-filled (all k_steps * obs_dim floats of obs with obs_steps), serial and
 * start -1.
 * obs_steps takes the place of a reserved field that was never read and that callers zero-fill: the struct's size and
 * layout, and MZS_ABI_VERSION, are unchanged. */
typedef struct mzs_replay_sample_args {
  int32_t struct_size;     /* = sizeof(mzs_replay_sample_args) */
  int32_t count;           /* rows of the compact table */
  int32_t batch, k_steps, sample_per_trajectory;
  uint32_t key[2];         /* HOST values */
  int32_t obs_steps;       /* 0, or k_steps (was reserved0, which every caller zero-filled) */
  float *obs;              /* out [batch, obs_dim], or [batch, k_steps, obs_dim] with obs_steps == k_steps */
  int32_t *a;              /* out [batch, k_steps] */
  float *r, *Rn, *v;       /* out [batch, k_steps] */
  uint8_t *done;           /* out [batch, k_steps], 0 / 1 */
  float *pi;               /* out [batch, k_steps, num_actions] */
  float *w;                /* out [batch, k_steps] */
  int64_t *serial;         /* out [batch] */
  int32_t *start;          /* out [batch] */
} mzs_replay_sample_args;
int mzs_replay_sample(const mzs_replay_arena *arena, const mzs_replay_sample_args *a, void *stream);

/* The same batch -- every output of mzs_replay_sample for the same key, bit for bit -- and the importance-sampling
 * weight of every row (Schaul et al. 2016, 3.4; MuZero Appendix G is beta = 1), in fp64, in this operation order:
 *   p_e = (CW[e] - CW[e - 1]) / CW[count - 1]   (CW[-1] = 0; 1 when CW[count - 1] == 0: the draw is deterministic)
 *   p_s = (cw[i] - cw[i - 1]) / cw[m - 1]       (cw[-1] = 0; 1 / (double)m when cw[m - 1] == 0: the uniform start)
 *   q   = p_e * p_s        the probability that a row is window (e, i), whatever rows share its episode
 *   raw = 1.0 / (num_windows * q) with beta == 1.0, pow(num_windows * q, -beta) otherwise (exactly 1 with beta == 0);
 *         0 for a zero-filled row (serial -1), which therefore does not train
 *   isw = (float)raw, or with normalize != 0 (float)(raw / the largest raw of the batch), the maximum taken in fp64;
 *         a batch of zero-filled rows alone gives zeros.
 * num_windows is the caller's count of eligible windows: the sum of length - k_steps over the live episodes longer than
 * k_steps.  One launch, and with normalize a second one of a single workgroup over `scratch`; deterministic; neither
 * synchronises or copies to the host.  MZS_E_INVALID before any launch for what mzs_replay_sample refuses, a struct
 * size, beta outside 0..1 or not finite, num_windows below 1 or not finite, a null isw, normalize with a null scratch. */
typedef struct mzs_replay_is_args {
  int32_t struct_size;     /* = sizeof(mzs_replay_is_args) */
  int32_t normalize;       /* != 0: divide by the batch maximum */
  double beta;             /* 0..1 */
  double num_windows;      /* N >= 1 */
  float *isw;              /* out [batch] */
  double *scratch;         /* [batch], or NULL with normalize == 0 */
} mzs_replay_is_args;
int mzs_replay_sample_is(const mzs_replay_arena *arena, const mzs_replay_sample_args *a, const mzs_replay_is_args *w,
                         void *stream);

/* Reanalysis: fresh search results for episodes the arenas already hold, without the host.  Between
 * the two calls the caller runs its searches on the gathered observations.  Both take the descriptors of
 * mzs_replay_store -- desc[e] = {first row in the dense stream, first row in the arena, length, table slot}, the HOST
 * copy checked here (every range inside the stream, the arena and the table, else MZS_E_INVALID), the DEVICE copy read
 * by the kernel -- one wavefront per episode, one launch each; neither synchronises or copies to the host.  The caller
 * keeps the episodes of one call disjoint and back to back in the stream (rows [0, stream_rows) all covered).
 *
 * mzs_replay_gather_obs: obs[src + t] = arena.obs[dst + t] for every selected episode; rows stream_rows ..
 *   rows_padded - 1 of `obs` are written as zeros (whole chunks for a fixed-batch search). */
typedef struct mzs_replay_gather_args {
  int32_t struct_size;     /* = sizeof(mzs_replay_gather_args) */
  int32_t episodes;
  int64_t stream_rows;     /* sum of the lengths */
  int64_t rows_padded;     /* >= stream_rows, < 2^31 */
  const int32_t *desc;       /* [episodes][4] */
  const int32_t *desc_host;  /* HOST [episodes][4] */
  float *obs;                /* out [rows_padded, obs_dim] */
} mzs_replay_gather_args;
int mzs_replay_gather_obs(const mzs_replay_arena *arena, const mzs_replay_gather_args *a, void *stream);

/* mzs_replay_reanalyse: for an episode of length T at stream row src, arena row dst:
 *   arena.pi[dst + t] = pi[src + t], arena.v[dst + t] = v[src + t];
 *   Rn, done, w by the arithmetic of mzs_replay_store's raw == 1, in fp64 and in its operation order, on
 *   r[t] = (double)arena.r[dst + t] (the STORED float reward) and v[t] = (double)v[src + t] (the bootstrap value is
 *   read from the stream as well); cw = the sequential inclusive prefix sum of w; the episode's table weight t_w =
 *   the mean (weight_mode 1) or the sum (weight_mode 2) of its w.
 * obs, a, r and the table's start / length / serial are not written.  The compact table is stale afterwards
 * (mzs_replay_refresh).  pi / v may have rows_padded rows; rows from stream_rows on are not read. */
typedef struct mzs_replay_reanalyse_args {
  int32_t struct_size;     /* = sizeof(mzs_replay_reanalyse_args) */
  int32_t episodes;
  int64_t stream_rows, rows_padded;
  const int32_t *desc;       /* [episodes][4] */
  const int32_t *desc_host;  /* HOST [episodes][4] */
  int32_t n_step;          /* >= 1 */
  int32_t weight_mode;     /* 1: mean, 2: sum */
  int32_t has_alpha, reserved0;
  double alpha;
  const double *gpow;        /* [n_step + 1]: gamma ** i */
  const float *pi;           /* [stream_rows, num_actions] */
  const float *v;            /* [stream_rows] */
} mzs_replay_reanalyse_args;
int mzs_replay_reanalyse(const mzs_replay_arena *arena, const mzs_replay_reanalyse_args *a, void *stream);

/* Priorities from training written back (prioritised replay): `batch` rows (serial[j], start[j]) as mzs_replay_sample
 * returns them, each with k_prio priorities; row j addresses transitions start[j] + i, i < k_prio, of the live episode
 * whose t_serial equals serial[j].  Two launches (one wavefront per row, then one per live episode); no synchronisation,
 * no copy to the host.
 * PRECONDITION (mzs_replay_refresh's): the live episodes are the `count` table slots from `head` on, wrapping at
 *   capacity, and their serials ascend along that ring -- the store's running number guarantees it.  The episode is
 *   found by binary search over t_serial on the ring; t_start / t_len give its rows.
 * Skipped silently, writing nothing: a row whose serial is not live (evicted since the sample, or the -1 of a
 *   zero-filled sample row); a row with start < 0; an element with start + i >= the episode's length; an element whose
 *   priority is NaN or +-inf.
 * New weight: w = (|p| + eps) ** alpha in fp64 on the widened float; with alpha == 1.0 no pow is executed, so w is
 *   exactly (double)|p| + eps.  Where several rows address one transition, the HIGHEST row index whose element is valid
 *   wins (NumPy's last assignment among the valid ones): deterministic; a skipped element never shadows a valid one.
 * Of every episode with at least one valid element: the new w, cw = the sequential inclusive prefix sum of the whole
 *   episode's w, t_w = the mean (weight_mode 1) or the sum (weight_mode 2) of its w.  Of every other episode not one
 *   byte is written (an ep_w given to the store survives until one of the episode's transitions is updated).  obs, a,
 *   r, Rn, v, done, pi, t_start, t_len, t_serial and the compact table are never written; the compact table is stale
 *   afterwards (mzs_replay_refresh).
 * Scratch (caller-owned): owner all -1 and touched all 0 on entry; both are left that way on exit.
 * batch == 0 or count == 0: MZS_OK without a launch.  MZS_E_INVALID, the message naming the field, before any launch
 *   for: struct sizes; head outside 0..capacity - 1; count outside 0..capacity; batch < 0; k_prio < 1 (or batch * k_prio
 *   >= 2^31); weight_mode other than 1 / 2; alpha outside 0..1; eps negative or not finite; a null pointer with
 *   batch > 0. */
typedef struct mzs_replay_update_args {
  int32_t struct_size;     /* = sizeof(mzs_replay_update_args) */
  int32_t head, count;     /* the live ring of the episode table */
  int32_t batch, k_prio;
  int32_t weight_mode;     /* 1: mean, 2: sum */
  double alpha, eps;
  const int64_t *serial;   /* [batch] */
  const int32_t *start;    /* [batch] */
  const float *prio;       /* [batch, k_prio] */
  int32_t *owner;          /* scratch [max_steps] */
  int32_t *touched;        /* scratch [capacity] */
} mzs_replay_update_args;
int mzs_replay_update_priorities(const mzs_replay_arena *arena, const mzs_replay_update_args *a, void *stream);

/* ---- collection on the device: a vector environment's steps staged in a ring, episodes cut in the store launch ----
 * The ring is caller-owned device memory, STEP-major: row s holds step s of all `num_envs` environments, so the
 * transitions of one episode lie num_envs rows apart and wrap at the ring's end.  r is double because the
 * environments' rewards are and mzs_replay_store's raw route reads double; v is act()'s float, widened (exactly)
 * inside the kernel.  The caller writes r itself (one or two copies per collection). */
typedef struct mzs_replay_ring {
  int32_t struct_size;     /* = sizeof(mzs_replay_ring) */
  int32_t device;
  int32_t ring_steps;      /* rows; ring_steps * max(obs_dim, num_actions) < 2^31 */
  int32_t num_envs;        /* N */
  int32_t obs_dim, num_actions;
  float *obs;              /* [ring_steps, N, obs_dim] */
  int32_t *a;              /* [ring_steps, N] */
  double *r;               /* [ring_steps, N] */
  float *v;                /* [ring_steps, N] */
  float *pi;               /* [ring_steps, N, num_actions] */
} mzs_replay_ring;

/* One step: obs [N, obs_dim], a [N], v [N], pi [N, num_actions] (device memory) into ring row `row`, in one launch;
 * r is not touched.  No copy to the host, no synchronisation.  MZS_E_INVALID before any launch for a struct size, a
 * null pointer, non-positive ring dimensions, or a row outside 0 .. ring_steps - 1. */
typedef struct mzs_replay_stage_args {
  int32_t struct_size;     /* = sizeof(mzs_replay_stage_args) */
  int32_t row;
  const float *obs;
  const int32_t *a;
  const float *v;
  const float *pi;
} mzs_replay_stage_args;
int mzs_replay_stage(const mzs_replay_ring *ring, const mzs_replay_stage_args *a, void *stream);

/* The finished episodes of a collection from the ring into the arenas: mzs_replay_store with raw == 1 reading a
 * strided, wrapping source -- one launch, one wavefront per episode.
 *   desc[e] = {environment, first ring row, length, first transition in the arena, table slot}; the HOST copy is
 *   checked here, the DEVICE copy is what the kernel reads.  Transition t of the episode is ring row
 *   (first + t) % ring_steps, column `environment`.
 * Written: obs, a, r (rounded to float), v, pi copied; Rn, done, w by the raw store's arithmetic in its operation
 * order; cw the sequential prefix sum; the table row with the mean (weight_mode 1) or the sum (2) of w -- bit for bit
 * what mzs_replay_store (raw == 1) writes for the same episodes given as a dense stream with v widened to double.
 * The cost of the strided reads against the dense store's has not been measured.
 * MZS_E_INVALID before any launch for: struct sizes; a null pointer; ring and arena that disagree in obs_dim,
 * num_actions or device; episodes outside 1..capacity; environment outside 0..num_envs - 1; length < 1 or
 * > ring_steps; a first row outside the ring; an arena range or a slot out of bounds; n_step < 1; weight_mode other
 * than 1 / 2. */
typedef struct mzs_replay_store_steps_args {
  int32_t struct_size;     /* = sizeof(mzs_replay_store_steps_args) */
  int32_t episodes;
  int32_t n_step, weight_mode, has_alpha, reserved0;
  double alpha;
  const int32_t *desc_host;  /* HOST [episodes][5] */
  const int32_t *desc;       /* [episodes][5] */
  const int64_t *serial;     /* [episodes] */
  const double *gpow;        /* [n_step + 1]: gamma ** i */
} mzs_replay_store_steps_args;
int mzs_replay_store_steps(const mzs_replay_arena *arena, const mzs_replay_ring *ring,
                           const mzs_replay_store_steps_args *a, void *stream);

/* The episodes a collection call finishes, cut and summed on the device: what the host otherwise works out from the
 * downloaded [steps, N] rewards and flags.  The rewards are ring->r; `done` is a uint8 [ring_steps, N] plane beside the
 * ring (the flags mzs_env_cartpole_step wrote); step t of the call is ring row (row0 + t) % ring_steps.
 * Environment e walks t = 0 .. steps - 1 in time order with len = open_len[e], g = open_ret[e]: every step does
 * len += 1 and g = g + r (a plain fp64 add in time order: no fused multiply-add, no reassociation -- NOT a pairwise
 * sum); where done != 0 the episode (e, first, len, g) ends, first = ((row0 - open_len[e] % ring_steps) + ring_steps) %
 * ring_steps for the environment's first episode of the call and the row after the previous end (modulo ring_steps)
 * for later ones, and len = 0, g = 0.0 start the next.  At the end len and g go back to open_len[e], open_ret[e].
 * Output: dense, environment-major then time: episode i of that order is ep[i] = {environment, first ring row, length,
 * stored = (length >= min_length)} and ret[i] = g.  counts = {episodes, stored episodes, max open_len afterwards, 0}.
 * Rows at or beyond counts[0] are not written; rows at or beyond max_out are never written and counts[0], counts[1]
 * still report the true totals (the caller compares counts[0] with max_out).
 * scratch: num_envs + (num_envs + 255) / 256 int32 of device memory, the call's to overwrite; nothing is kept in it
 * between calls.
 * Two launches on the caller's stream (a count, then a scan-and-emit that walks again; one thread per environment);
 * deterministic; no allocation, no copy to the host, no synchronisation.  counts[1] and counts[2] are integer atomics.
 * MZS_E_INVALID before any launch, the field named, for: struct sizes; a null pointer; non-positive ring dimensions;
 * row0 outside 0 .. ring_steps - 1; steps outside 1 .. ring_steps; num_envs * steps >= 2^31; min_length < 1;
 * max_out < 1. */
typedef struct mzs_replay_plan_args {
  int32_t struct_size;     /* = sizeof(mzs_replay_plan_args) */
  int32_t row0;            /* ring row of the call's first step */
  int32_t steps;           /* T */
  int32_t min_length;
  int32_t max_out;         /* rows of ep / ret */
  int32_t reserved0;
  const uint8_t *done;     /* [ring_steps, N] */
  int32_t *open_len;       /* [N] in/out: steps of each environment's open episode */
  double *open_ret;        /* [N] in/out: sum of that open episode's rewards so far */
  int32_t *ep;             /* out [max_out][4] */
  double *ret;             /* out [max_out] */
  int32_t *counts;         /* out [4] */
  int32_t *scratch;        /* [num_envs + (num_envs + 255) / 256] */
} mzs_replay_plan_args;
int mzs_replay_plan_steps(const mzs_replay_ring *ring, const mzs_replay_plan_args *a, void *stream);

/* ---- vector environments stepped on the device: the cart-pole ----
 * N cart-poles (Barto, Sutton, Anderson 1983: explicit Euler at 50 Hz, force +-10 N, reward 1 per step; an episode ends
 * when |x| > 2.4, |theta| > 12 * 2 * pi / 360 or after max_episode_steps steps) with auto-reset.  The descriptor and
 * its three arrays are the caller's (device memory, state 16-byte aligned); zeroed arrays are a valid start.
 * The start state of environment e, its d-th draw (d = draws[e]), component c:
 *   state[c] = -0.05 + 0.1 * u53(key, e, 4 d + c),  u53 = ((y0 << 32 | y1) >> 11) * 2^-53 of threefry2x32(key, x0, x1)
 * (the uniform of mzs_replay_sample), after which draws[e] grows by one: no math-library call, so the same bits as the
 * host's restatement.  4 d + c is taken modulo 2^32.
 * Both entries: one launch, one thread per environment, on the caller's stream; no allocation, no copy to the host, no
 * synchronisation.  MZS_E_INVALID before any launch for a struct size, a null pointer, num_envs < 1,
 * max_episode_steps < 1, or a state / obs_out that is not 16-byte aligned.  errors: mzs_last_error(NULL) */
typedef struct mzs_env_cartpole {
  int32_t struct_size;       /* = sizeof(mzs_env_cartpole) */
  int32_t device;
  int32_t num_envs;          /* N */
  int32_t max_episode_steps;
  uint32_t key[2];
  double *state;             /* [N, 4]: x, x_dot, theta, theta_dot */
  int32_t *t;                /* [N] steps of the open episode */
  int32_t *draws;            /* [N] start states drawn so far */
} mzs_env_cartpole;

/* Every environment draws a fresh start state; t = 0; obs_out [N, 4] = (float)state. */
int mzs_env_cartpole_reset(const mzs_env_cartpole *env, float *obs_out, void *stream);

/* One step of every environment in fp64, in the operation order of the host's VectorCartPole.step (no fused
 * multiply-add): force +10 where a == 1, -10 for any other value; r_out = 1.0; done_out = 1 where the NEW state has
 * |x| > 2.4 or |theta| > the angle limit, or t + 1 >= max_episode_steps, else 0.  A finished environment draws its next
 * start state and sets t = 0 in the same launch, so obs_out = (float)state is already the first observation of its
 * next episode.  sin and cos are the device library's: the new state equals a host libm's to a few units in the last
 * place, not bit for bit.  r_out and done_out are plain [N] pointers (a row of a larger array will do). */
typedef struct mzs_env_step_args {
  int32_t struct_size;       /* = sizeof(mzs_env_step_args) */
  int32_t reserved0;
  const int32_t *a;          /* [N] */
  float *obs_out;            /* [N, 4] */
  double *r_out;             /* [N] */
  uint8_t *done_out;         /* [N] */
} mzs_env_step_args;
int mzs_env_cartpole_step(const mzs_env_cartpole *env, const mzs_env_step_args *a, void *stream);

/* ---- vector environments stepped on the device: Acrobot and MountainCar ----
 * The two other discrete classic-control tasks behind one descriptor; `kind` selects the dynamics and with them the
 * widths:            kind                  state [N, .] f64             obs_out [N, .] f32                     actions
 *   MZS_ENV_ACROBOT      (1)   4: th1, th2, dth1, dth2     6: cos th1, sin th1, cos th2, sin th2, dth1, dth2    3
 *   MZS_ENV_MOUNTAINCAR  (2)   2: x, v                     2: (float)x, (float)v                                3
 * Conventions, arrays, auto-reset and the draw rule are the cart-pole's: with C drawn components, component c of
 * environment e's d-th draw (d = draws[e], which then grows by one) is lo_c + width_c * u53(key, e, C d + c) --
 *   Acrobot: all four components -0.1 + 0.2 u (C = 4);   MountainCar: x = -0.6 + 0.2 u, v = 0 (C = 1)
 * -- no math-library call, so the same bits as the host's restatement.  C d + c is taken modulo 2^32.
 * Acrobot (Sutton & Barto's "book" equations as in Gym's Acrobot-v1): action <= 0 is torque -1, 1 is 0, >= 2 is +1; one
 *   classical Runge-Kutta step of dt = 0.2 of (state, torque) with m1 = m2 = 1, l1 = 1, lc1 = lc2 = 0.5, I1 = I2 = 1,
 *   g = 9.8; then th1 and th2 are brought into [-pi, pi] by repeated -+2 pi (each way at most 64 times: far more than
 *   any step from a wrapped state needs, and an infinite or absurdly large uploaded angle cannot keep the launch
 *   running), dth1 is clamped to +-4 pi and dth2 to +-9 pi.  terminated = -cos th1 - cos(th1 + th2) > 1 on the NEW
 *   state; r_out = -1.0, and 0.0 on a terminating step.
 * MountainCar (Gym's MountainCar-v0 in fp64): the action is clamped to 0..2; v += (a - 1) 0.001 + cos(3 x) (-0.0025),
 *   v clamped to +-0.07, x += v, x clamped to [-1.2, 0.6], v = 0 where x == -1.2 and v < 0; terminated = x >= 0.5 and
 *   v >= 0; r_out = -1.0 on every step.
 * Both: done_out = terminated or t + 1 >= max_episode_steps; a finished environment draws its next start state and sets
 * t = 0 in the same launch, so obs_out already shows the next episode's first observation.  fp64, operation by
 * operation, no fused multiply-add; sin and cos are the device library's, so a stepped state equals a host libm's to
 * the last bits only (measured: profiles/env_device.txt).  mzs_env_step_args is the cart-pole's, obs_out [N, 6] or
 * [N, 2].  One launch per call, one thread per environment, on the caller's stream; no allocation, no copy to the
 * host, no synchronisation.  MZS_E_INVALID before any launch, nothing written, for a struct size, an unknown kind, a
 * null pointer, num_envs < 1, max_episode_steps < 1, a state that is not 16-byte aligned or an obs_out that is not
 * 8-BYTE aligned (obs is stored two floats at a time for both kinds).  errors: mzs_last_error(NULL) */
#define MZS_ENV_ACROBOT 1
#define MZS_ENV_MOUNTAINCAR 2
typedef struct mzs_env_classic {
  int32_t struct_size;       /* = sizeof(mzs_env_classic) */
  int32_t device;
  int32_t kind;              /* MZS_ENV_ACROBOT or MZS_ENV_MOUNTAINCAR */
  int32_t num_envs;          /* N */
  int32_t max_episode_steps;
  uint32_t key[2];
  double *state;             /* [N, 4] or [N, 2] */
  int32_t *t;                /* [N] steps of the open episode */
  int32_t *draws;            /* [N] start states drawn so far */
} mzs_env_classic;
int mzs_env_classic_reset(const mzs_env_classic *env, float *obs_out, void *stream);
int mzs_env_classic_step(const mzs_env_classic *env, const mzs_env_step_args *a, void *stream);

/* ---- vector environments stepped on the device: 2048, with the legal-move mask of every returned observation ----
 * Board: one uint64 per environment; nibble i (bits 4 i .. 4 i + 3) is the exponent of cell i, row-major, cell 0
 *   top-left.  Exponent 0 is empty, exponent k is tile 2^k.
 * Moves: actions 0 up, 1 right, 2 down, 3 left; any other value is treated as illegal.  A move slides every line toward
 *   its edge and merges equal neighbours once per tile, starting from that edge: 2 2 2 2 -> 4 4 . . and
 *   2 2 4 . -> 4 4 . .  Two tiles of exponent 15 do not merge.
 * Reward: the sum of the tiles created by merging, as fp64, times 2^-reward_shift (reward_shift 0..11): a power of two
 *   keeps every reward and every partial sum exact, so sequential and pairwise sums of an episode have the same bits.
 * Illegal moves: a move that would leave the board unchanged is illegal.  Taking it is a no-op: reward 0, no spawn, no
 *   draw consumed; t still advances.
 * Spawns: after a legal move one tile spawns.  With d = draws[e] and (x0, x1) = threefry2x32(key, (e, d)) -- the block
 *   and counter convention of the other environments' u53 -- and n the number of empty cells, enumerated in ascending
 *   cell index, the cell chosen is number k = (uint64(x0) * n) >> 32 of them and the spawned exponent is 2 if
 *   x1 < 0x1999999A, else 1; then draws[e] grows by one.  A reset spawns twice on an empty board.
 * Termination: terminated = the board after the step has no legal move (no move changes it; evaluated after a no-op as
 *   well, so an uploaded dead board -- an empty one included -- ends on its next step); done_out = terminated or
 *   t + 1 >= max_episode_steps.  A finished environment resets in the same launch and sets t = 0: obs_out and the mask
 *   are already the next episode's.
 * Observation: obs_out float32 [N, 16], obs[i] = exponent_i / 16 (exact).
 * Mask: invalid uint8 [N, 4], 1 where the move is illegal for the returned observation.  A board with no tile at all
 *   reports every move as legal (zero-padded reanalysis rows: an all-invalid root must never reach a search).
 * The descriptor and its four arrays are the caller's device memory; the mask lies in the descriptor, beside the state
 * the launch already owns, and mzs_env_step_args is the other environments'.  Zeroed t and draws are a valid start; the
 * board is whatever mzs_env_2048_reset or the caller put there.
 * reset, step: one launch, one thread per environment, integer work in registers (no table in memory), on the caller's
 * stream; no allocation, no copy to the host, no synchronisation.  MZS_E_INVALID before any launch, nothing written,
 * for a struct size, a null pointer, num_envs < 1, max_episode_steps < 1, reward_shift outside 0..11, a board that is
 * not 8-byte aligned, an invalid that is not 4-byte aligned (the mask is one 32-bit store) or an obs_out that is not
 * 16-byte aligned (four float4 stores).  errors: mzs_last_error(NULL) */
typedef struct mzs_env_2048 {
  int32_t struct_size;       /* = sizeof(mzs_env_2048) */
  int32_t device;
  int32_t num_envs;          /* N */
  int32_t max_episode_steps;
  uint32_t key[2];
  int32_t reward_shift;      /* 0..11: rewards are scaled by 2^-reward_shift */
  int32_t reserved0;
  uint64_t *board;           /* [N] */
  int32_t *t;                /* [N] steps of the open episode */
  int32_t *draws;            /* [N] spawns drawn so far */
  uint8_t *invalid;          /* [N, 4] out: 1 where the move is illegal for the returned observation */
} mzs_env_2048;
int mzs_env_2048_reset(const mzs_env_2048 *env, float *obs_out, void *stream);
int mzs_env_2048_step(const mzs_env_2048 *env, const mzs_env_step_args *a, void *stream);

/* The same legality rule from observations: invalid_out [B, 4] = the mask of the boards obs [B, 16] encodes, decoded as
 * exponent = lrintf(obs * 16) clamped to 0..15 (an all-zero row: mask 0).  One launch, one thread per row, on the
 * caller's stream.  MZS_E_INVALID before any launch for a null pointer, B < 1, an obs that is not 16-byte aligned or an
 * invalid_out that is not 4-byte aligned. */
int mzs_env_2048_mask(int32_t device, const float *obs, uint8_t *invalid_out, int32_t B, void *stream);

/* ---- forward value unroll of the default MLP trio: the priorities mzs_replay_update_priorities takes ----
 * For every window j < batch and step i < k_prio, with s_0 = Representation(obs[j]) and s_{i+1} = the next state of
 * Dynamic(s_i, actions[j][i]) (muax/nn.py:59-115):
 *   values[j][i] = support_to_scalar(softmax(value head(s_i)))     prio[j][i] = |values[j][i] - returns[j][i]|
 * One launch, one wavefront per window; the policy head and the reward head are not evaluated.  The arithmetic is the
 * spec's ("MZ-F32"): values has the bits of the oracle's root_inference / recurrent_inference chain for any widths, prio
 * is one fp32 subtraction with the sign cleared (a NaN or infinite return gives a NaN or infinite priority, which
 * mzs_replay_update_priorities skips).  No atomics: the same bits on every run.  No allocation, no synchronisation, no
 * copy to the host.  `actions` and `returns` are read with the row stride row_steps, of which the first k_prio columns
 * are used; an action outside 0..num_actions - 1 is the all-zero one-hot (nothing is indexed by it).
 * Limits, checked before any launch, the message naming the limit: MZS_E_UNSUPPORTED for obs_dim outside 1..128,
 * embed_dim outside 1..64, num_actions outside 1..64, support_size outside 8..31; MZS_E_INVALID for struct sizes, a
 * null weight / input pointer, batch < 1, k_prio outside 1..row_steps, values and prio both NULL.
 * errors: mzs_last_error(NULL) */
typedef struct mzs_unroll_args {
  int32_t struct_size;      /* = sizeof(mzs_unroll_args) */
  int32_t device;
  int32_t batch;            /* B windows */
  int32_t row_steps;        /* L: row stride of actions and returns */
  int32_t k_prio;           /* kp <= L steps evaluated */
  int32_t num_actions;
  int32_t embed_dim;
  int32_t reserved0;
  const float *obs;         /* [B, obs_dim] */
  const int32_t *actions;   /* [B, L] */
  const float *returns;     /* [B, L] */
  float *values;            /* out [B, kp] or NULL */
  float *prio;              /* out [B, kp] or NULL */
} mzs_unroll_args;
int mzs_mlp_unroll_values(const mzs_mlp_weights *w, const mzs_unroll_args *a, void *stream);

/* ---- the same unroll of the default stochastic MLP family (mz_stoch_unroll_kernel, muax_amd/csrc/mz_unroll.cuh) ----
 * For every window j < batch and step i < k_prio, with s_0 = Representation(obs[j][0]):
 *   values[j][i] = support_to_scalar(softmax(value head pv(s_i)))     prio[j][i] = |values[j][i] - returns[j][i]|
 * and, while i + 1 < k_prio,
 *   after_i = min_max(ad([s_i | onehot(actions[j][i], A)]))           the afterstate dynamics
 *   c_{i+1} = argmax_k en(obs[j][i+1])[k]                             the chance encoder on the raw observation row,
 *                                                                     the lowest index among equal maxima
 *   s_{i+1} = min_max(cn([after_i | onehot(c_{i+1}, C)]))             the chance dynamics' next state, an exact one-hot
 * -- the chain and the code rule of mzs_stochastic_mlp_loss_grad.  codes[j][0] = -1 (step 0 has no transition),
 * codes[j][i] = c_i behind it.  One launch, one wavefront per window; the afterstate value, the chance logits, the
 * policy head and the reward head are not evaluated.  The arithmetic is the spec's ("MZ-F32"): values has the bits of the
 * oracle's inference chain for any widths, prio is one fp32 subtraction with the sign cleared.  No atomics: the same
 * bits on every run.  No allocation, no synchronisation, no copy to the host; capturable.  obs rows, `actions` and
 * `returns` are read with the row stride row_steps, of which the first k_prio are used; an action outside
 * 0..num_actions - 1 is the all-zero one-hot (nothing is indexed by it).
 * The weights are the 34 arrays of mzs_stochastic_train_weights; of its scalar fields this entry reads obs_dim, here
 * 1..128 (the 1..32 of that struct's comment is the training entry's own limit), and support_size.
 * Limits, checked before the device is selected, the message naming the entry and the limit: MZS_E_UNSUPPORTED for
 * obs_dim outside 1..128, embed_dim outside 1..64, num_actions < 1, num_chance_outcomes < 1,
 * num_actions + num_chance_outcomes > 64, support_size outside 8..31; MZS_E_INVALID for struct sizes, a null weight /
 * input pointer, batch < 1, k_prio outside 1..row_steps, values, prio and codes all NULL.
 * errors: mzs_last_error(NULL) */
typedef struct mzs_stochastic_unroll_args {
  int32_t struct_size;          /* = sizeof(mzs_stochastic_unroll_args) */
  int32_t device;
  int32_t batch;                /* B windows */
  int32_t row_steps;            /* L: row stride of obs rows, actions and returns */
  int32_t k_prio;               /* kp <= L steps evaluated */
  int32_t num_actions;          /* A */
  int32_t num_chance_outcomes;  /* C */
  int32_t embed_dim;            /* E */
  const float *obs;             /* [B, L, obs_dim] */
  const int32_t *actions;       /* [B, L] */
  const float *returns;         /* [B, L] */
  float *values;                /* out [B, kp] or NULL */
  float *prio;                  /* out [B, kp] or NULL */
  int32_t *codes;               /* out [B, kp] or NULL */
} mzs_stochastic_unroll_args;
int mzs_stochastic_mlp_unroll_values(const mzs_stochastic_train_weights *w, const mzs_stochastic_unroll_args *a,
                                     void *stream);

#ifdef __cplusplus
}
#endif
#endif
