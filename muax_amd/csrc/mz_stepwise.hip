// mz_stepwise.hip -- the routes on the HBM tree of mz_step.cuh, whose kernels (mz_step_kernels.cuh) THIS unit emits: the
// step-wise entry points for plugin nets (mzs_root .. mzs_finish, mzs_tree_export), the generic one-launch act()
// (mz_mlp_generic.cuh) and the default stochastic MLP family's one-launch recurrent step (mz_stoch_mlp.cuh).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "mz_handle.h"
#include "mz_mlp_generic.cuh"
#include "mz_step_kernels.cuh"
#include "mz_stoch_mlp.cuh"
#include "mz_stoch_wide_launch.h"

using mzh::fail;

// Small batches run one wavefront (4 roots) per workgroup: the tree of a root is then always walked from the
// same XCD, all 8 L2s share the trees, and the dependent per-level loads hit L2 instead of HBM.
static int step_block(int batch) { return batch >= 4096 ? 256 : 64; }
static int step_grid(int batch) { const int per = step_block(batch) / 16; return (batch + per - 1) / per; }

static void emb_xfer(const mz::StepArgs& sa, float* rows, int dir, hipStream_t stream) {
  hipLaunchKernelGGL(mz::emb_xfer_kernel, dim3(sa.B, (sa.E + 1023) / 1024), dim3(256), 0, stream, sa, rows, dir);
}

// What roots a tree: the root inference's outputs and, by policy, the Dirichlet noise (MuZero, stochastic) or the Gumbel
// noise -- null: drawn from the key gk -- (Gumbel); the other policies' members are null / 0
struct RootInputs {
  const float *prior_logits, *value, *embedding;
  const uint8_t* invalid_actions;
  const float* dirichlet_noise;
  float dirichlet_fraction;
  const float* gumbel;
  uint32_t gk[2];
};
// roots the trees of sa's rows by the handle's policy; `jump`: ... and their cached decisions (the slab holds these rows)
static void launch_root(mzs_handle* h, const mz::StepArgs& sa, const RootInputs& in, bool jump, hipStream_t stream) {
  const dim3 grid(step_grid(sa.B)), blk(step_block(sa.B));
  const int gumbel = h->cfg.policy == 1;
  if (h->cfg.policy == 2)
    hipLaunchKernelGGL(mz::step_root_stochastic_kernel, grid, blk, 0, stream, sa, in.prior_logits, in.value, in.embedding,
                       h->cfg.state_embed_dim, in.invalid_actions, in.dirichlet_noise, in.dirichlet_fraction);
  else
    hipLaunchKernelGGL(mz::step_root_kernel, grid, blk, 0, stream, sa, in.prior_logits, in.value, in.embedding, in.invalid_actions,
                       in.dirichlet_noise, in.dirichlet_fraction, gumbel, in.gumbel, in.gk[0], in.gk[1]);
  if (jump && gumbel) hipLaunchKernelGGL(mz::jump_root_kernel<true>, grid, blk, 0, stream, sa, h->jump);
  else if (jump) hipLaunchKernelGGL(mz::jump_root_kernel<false>, grid, blk, 0, stream, sa, h->jump);
}
// the policy's action choice over sa's rows (gumbel: the MuZero and the stochastic policy's optional sampling noise;
// k_sample from the key walk)
static void launch_finish(mzs_handle* h, const mz::StepArgs& sa, float temperature, const float* gumbel, int32_t* action_out,
                          float* action_weights_out, float* search_value_out, int32_t* depth_sum_out, hipStream_t stream) {
  const dim3 grid(step_grid(sa.B)), blk(step_block(sa.B));
  if (h->cfg.policy == 1)
    hipLaunchKernelGGL(mz::step_finish_gumbel_kernel, grid, blk, 0, stream, sa, action_out, action_weights_out,
                       search_value_out, depth_sum_out);
  else if (h->cfg.policy == 2)
    hipLaunchKernelGGL(mz::step_finish_stochastic_kernel, grid, blk, 0, stream, sa, temperature, gumbel, h->k_sample[0],
                       h->k_sample[1], action_out, action_weights_out, search_value_out, depth_sum_out);
  else
    hipLaunchKernelGGL(mz::step_finish_kernel, grid, blk, 0, stream, sa, temperature, gumbel, h->k_sample[0], h->k_sample[1],
                       action_out, action_weights_out, search_value_out, depth_sum_out);
}

static int ensure_step_state(mzs_handle* h) {
  const mzs_config& c = h->cfg;
  if (h->step.allocated) return MZS_OK;
  const int rows = c.policy == 1 ? c.max_num_considered_actions + 1 : 0;
  const int table_words = rows * c.num_simulations;
  hipError_t e = h->step.allocate(c.batch, c.num_simulations + 1, mz::slots_per_node(c), c.embed_dim, table_words);
  if (e != hipSuccess) return fail(h, MZS_E_RUNTIME, "tree allocation: %s", hipGetErrorString(e));
  // cached-decision kernels (mz_step_jump.cuh): bounded tree, B N^2 path words within the slab budget (8 GiB of the
  // 288 GB: 4096 roots x 300 simulations are 1.5 GB; MZS_JUMP_BUDGET_MB overrides); MZS_STEP_WALK=1 keeps the
  // level-by-level kernels (A/B testing).  A tree beyond the budget gets a slab for a CHUNK of roots: the step-wise
  // entry points then walk level by level (they address the whole batch), the generic one-launch search of mzs_act_mlp
  // runs the batch chunk by chunk (roots never interact; muax/model.py:222-243 takes any num_simulations).
  const size_t B = (size_t)c.batch, N = (size_t)c.num_simulations + 1;
  const char* walk = getenv("MZS_STEP_WALK");
  const char* mb = getenv("MZS_JUMP_BUDGET_MB");
  const size_t budget = mb && atoll(mb) > 0 ? (size_t)atoll(mb) << 20 : (size_t)8 << 30;
  const size_t per_root = (3 * N + N * N) * 4;
  if (N <= (size_t)mz::kJumpMaxNodes && !(walk && walk[0] == '1') && c.policy != 2) {  // (chance nodes: walked only)
    const bool whole = B * per_root <= budget;
    size_t roots = whole ? B : budget / per_root;
    if (roots > B) roots = B;
    if (roots >= 1 && hipMalloc(&h->jump_slab, roots * per_root) == hipSuccess) {
      int32_t* w = static_cast<int32_t*>(h->jump_slab);
      h->jump.jump_pa = w; h->jump.jump_lv = w + roots * N; h->jump.node_depth = w + 2 * roots * N;
      h->jump.node_path = reinterpret_cast<uint32_t*>(w + 3 * roots * N);
      h->use_jump = whole;
      h->jump_roots = (int)roots;
    }
  }
  if (table_words) {
    const std::vector<int32_t> table = mzh::visit_table(c.max_num_considered_actions, c.num_simulations);
    MZS_HIP(h, hipMemcpy(h->step.visit_table, table.data(), sizeof(int32_t) * table.size(), hipMemcpyHostToDevice));
  }
  return MZS_OK;
}

int mzh::step_view(mzs_handle* h, mz::StepArgs* sa, mz::JumpArgs* ja, int* policy, const char* who, int* device) {
  if (!h) return MZS_E_INVALID;
  if (!h->step.rooted) return fail(h, MZS_E_INVALID, "%s: call mzs_root first", who);
  if (!h->use_jump) return fail(h, MZS_E_UNSUPPORTED, "%s: this handle's tree has no cached decisions (too large, or MZS_STEP_WALK=1)", who);
  *sa = h->step.args(h->cfg);
  *ja = h->jump;
  *policy = h->cfg.policy;
  if (device) *device = h->cfg.device;
  return MZS_OK;
}

// What a step-wise entry works with once its call passed: the stream, the tree and the one-row-per-root geometry
struct StepCall { hipStream_t stream; mz::StepArgs sa; dim3 grid, blk; };
constexpr int kMuZero = 1, kGumbel = 2, kDeterministic = kMuZero | kGumbel, kStochastic = 4;  // policies an entry serves (bits)
constexpr int32_t kNoSim = 0;  // (what an entry without a simulation index passes)
// How every step-wise entry opens: the refusals in the order its family reports them -- the stochastic entries: policy,
// root, sim, arguments; every other: root, sim, arguments, policy -- in the entry's own words (bad_args: null when the
// arguments are in order), then the device, the tree (`rooted`: the entry needs one; a root entry allocates it) and the call.
static int step_begin(mzs_handle* h, const char* who, int serves, const char* other_policy, bool rooted, int32_t sim,
                      const char* bad_args, void* stream_, StepCall* call) {
  if (!h) return MZS_E_INVALID;
  const mzs_config& c = h->cfg;
  const bool stochastic = serves == kStochastic, served = (serves >> c.policy) & 1;
  auto refuse = [&](const char* what) { return fail(h, MZS_E_INVALID, "%s", (std::string(who) + ": " + what).c_str()); };
  if (stochastic && !served) return refuse(other_policy);
  if (rooted && !h->step.rooted) return refuse(stochastic ? "call mzs_root_stochastic first" : "call mzs_root first");
  if (sim < 0 || sim >= c.num_simulations) return refuse("sim out of range");
  if (bad_args) return refuse(bad_args);
  if (!served) return refuse(other_policy);
  MZS_HIP(h, hipSetDevice(c.device));
  if (int rc = rooted ? MZS_OK : ensure_step_state(h)) return rc;
  *call = {static_cast<hipStream_t>(stream_), h->step.args(c), dim3(step_grid(c.batch)), dim3(step_block(c.batch))};
  return MZS_OK;
}
static int launched(mzs_handle* h) {
  MZS_HIP(h, hipGetLastError());
  return MZS_OK;
}
static const char* root_bad_args(const RootInputs& in) {
  if (!in.prior_logits || !in.value || !in.embedding) return "null input";
  if (!in.dirichlet_noise && in.dirichlet_fraction != 0.0f) return "dirichlet_fraction != 0 needs dirichlet_noise";
  return nullptr;
}

// the keys of a MuZero or stochastic tree from the act's key (null: zero): k_sample, and with tie-break noise every
// simulation's key on the device
static int seed_tree_keys(mzs_handle* h, const uint32_t key[2], hipStream_t stream) {
  const mzs_config& c = h->cfg;
  const uint32_t zero[2] = {0, 0};
  mzh::derive_keys(key ? key : zero, c.num_simulations, h->k_sample, h->sim_keys.data());
  if (c.tiebreak) {
    // pageable source: the runtime stages it before the call returns, so the next act() may rewrite sim_keys
    MZS_HIP(h, hipMemcpyAsync(h->step.sim_keys, h->sim_keys.data(), sizeof(uint32_t) * 2 * (size_t)c.num_simulations,
                              hipMemcpyHostToDevice, stream));
  }
  return MZS_OK;
}
// the whole batch rooted: the root launch and, for wide embeddings, the rows zeroed before and the root's row scattered after
static int root_batch(mzs_handle* h, const StepCall& call, const RootInputs& in) {
  const mz::StepArgs& sa = call.sa;
  hipStream_t stream = call.stream;
  if (sa.wide) MZS_HIP(h, hipMemsetAsync(sa.embeddings, 0, sizeof(float) * (size_t)sa.B * sa.N * sa.E, stream));
  launch_root(h, sa, in, h->use_jump, stream);
  if (sa.wide) emb_xfer(sa, const_cast<float*>(in.embedding), 1, stream);
  h->step.rooted = true;
  return launched(h);
}
// mzs_root and mzs_root_stochastic: the roots of the MuZero prelude (Dirichlet noise, the tree's keys)
static int root_dirichlet(mzs_handle* h, const char* who, int serves, const char* other_policy, const RootInputs& in,
                          const uint32_t key[2], void* stream_) {
  StepCall c;
  if (int rc = step_begin(h, who, serves, other_policy, false, kNoSim, root_bad_args(in), stream_, &c)) return rc;
  if (int rc = seed_tree_keys(h, key, c.stream)) return rc;
  return root_batch(h, c, in);
}
static int finish_impl(mzs_handle* h, const char* who, int serves, const char* other_policy, float temperature, const float* gumbel,
                       int32_t* action_out, float* action_weights_out, float* search_value_out, int32_t* depth_sum_out,
                       void* stream_) {
  StepCall c;
  if (int rc = step_begin(h, who, serves, other_policy, true, kNoSim, !action_out || !action_weights_out ? "null output" : nullptr,
                          stream_, &c))
    return rc;
  launch_finish(h, c.sa, temperature, gumbel, action_out, action_weights_out, search_value_out, depth_sum_out, c.stream);
  return launched(h);
}

extern "C" {

int mzs_root(mzs_handle* h, const float* prior_logits, const float* value, const float* embedding, const uint8_t* invalid_actions,
             const float* dirichlet_noise, float dirichlet_fraction, const uint32_t key[2], void* stream_) {
  return root_dirichlet(h, "mzs_root", kMuZero,
                        h && h->cfg.policy == 2 ? "this handle runs the stochastic policy; use mzs_root_stochastic"
                                                : "this handle runs the gumbel policy; use mzs_root_gumbel",
                        {prior_logits, value, embedding, invalid_actions, dirichlet_noise, dirichlet_fraction, nullptr, {0, 0}}, key,
                        stream_);
}

int mzs_root_gumbel(mzs_handle* h, const float* prior_logits, const float* value, const float* embedding,
                    const uint8_t* invalid_actions, const float* gumbel, const uint32_t key[2], void* stream_) {
  RootInputs in = {prior_logits, value, embedding, invalid_actions, nullptr, 0.0f, gumbel, {0, 0}};
  StepCall c;
  if (int rc = step_begin(h, "mzs_root_gumbel", kGumbel, "this handle does not run the gumbel policy (policy 1)", false, kNoSim,
                          root_bad_args(in), stream_, &c))
    return rc;
  // mctx gumbel_muzero_policy: rng_key, gumbel_rng = jax.random.split(rng_key)
  const uint32_t zero[2] = {0, 0};
  mzh::h_split(key ? key : zero, 2, 1, in.gk);
  return root_batch(h, c, in);
}

int mzs_select(mzs_handle* h, int32_t sim, int32_t* action_out, float* parent_embedding_out, void* stream_) {
  StepCall call;
  if (int rc = step_begin(h, "mzs_select", kDeterministic, "this handle runs the stochastic policy; use mzs_select_stochastic", true,
                          sim, !action_out || !parent_embedding_out ? "null output" : nullptr, stream_, &call))
    return rc;
  const mzs_config& c = h->cfg;
  const mz::StepArgs& sa = call.sa;
  hipStream_t stream = call.stream;
  const bool gathers = h->use_jump && sa.wide;  // one workgroup per root: selection + the gather of the wide embedding row
  if (gathers)
    hipLaunchKernelGGL(mz::jump_select_kernel<true>, dim3(c.batch), dim3(256), 0, stream, sa, h->jump, sim, action_out,
                       parent_embedding_out);
  else if (h->use_jump)
    hipLaunchKernelGGL(mz::jump_select_kernel<false>, call.grid, call.blk, 0, stream, sa, h->jump, sim, action_out,
                       parent_embedding_out);
  else if (c.policy == 1)
    hipLaunchKernelGGL(mz::step_select_gumbel_kernel, call.grid, call.blk, 0, stream, sa, sim, action_out, parent_embedding_out);
  else
    hipLaunchKernelGGL(mz::step_select_kernel, call.grid, call.blk, 0, stream, sa, sim, action_out, parent_embedding_out);
  if (sa.wide && !gathers) emb_xfer(sa, parent_embedding_out, 0, stream);
  return launched(h);
}

static int expand_backup_impl(mzs_handle* h, int32_t sim, const float* reward, const float* discount, const float* prior_logits,
                              const float* value, const float* next_embedding, int32_t* next_action_out,
                              float* next_parent_embedding_out, void* stream_, const char* who) {
  StepCall call;
  if (int rc = step_begin(h, who, kDeterministic, "this handle runs the stochastic policy; use mzs_expand_backup_stochastic", true,
                          sim, !reward || !discount || !prior_logits || !value || !next_embedding ? "null input" : nullptr,
                          stream_, &call))
    return rc;
  const mzs_config& c = h->cfg;
  const mz::StepArgs& sa = call.sa;
  hipStream_t stream = call.stream;
  const bool want_next = next_action_out != nullptr && sim + 1 < c.num_simulations;
  if (h->use_jump) {
    // small batches: 16 levels in flight per root; large ones: one wavefront per root keeps the launch small;
    // few roots and long searches (deep paths): 64 levels in flight
    const dim3 blk(c.batch <= 256 && c.num_simulations >= 64 ? 1024 : (c.batch <= 1024 ? 256 : 64));
    const size_t lds = sizeof(int32_t) * 15 * ((size_t)c.num_simulations + 2);
    if (c.policy == 1)
      hipLaunchKernelGGL(mz::jump_expand_backup_kernel<true>, dim3(c.batch), blk, lds, stream, sa, h->jump, sim, reward,
                         discount, prior_logits, value, next_embedding, next_action_out, next_parent_embedding_out);
    else
      hipLaunchKernelGGL(mz::jump_expand_backup_kernel<false>, dim3(c.batch), blk, lds, stream, sa, h->jump, sim, reward,
                         discount, prior_logits, value, next_embedding, next_action_out, next_parent_embedding_out);
  } else
    hipLaunchKernelGGL(mz::step_expand_backup_kernel, call.grid, call.blk, 0, stream, sa, sim, reward, discount, prior_logits,
                       value, next_embedding);
  if (sa.wide && !h->use_jump) emb_xfer(sa, const_cast<float*>(next_embedding), 1, stream);
  MZS_HIP(h, hipGetLastError());
  // the walking kernels (trees beyond the cached-decision budget, MZS_STEP_WALK=1) select in a launch of their own
  if (want_next && !h->use_jump) return mzs_select(h, sim + 1, next_action_out, next_parent_embedding_out, stream_);
  return MZS_OK;
}

int mzs_expand_backup(mzs_handle* h, int32_t sim, const float* reward, const float* discount, const float* prior_logits,
                      const float* value, const float* next_embedding, void* stream_) {
  return expand_backup_impl(h, sim, reward, discount, prior_logits, value, next_embedding, nullptr, nullptr, stream_,
                            "mzs_expand_backup");
}

int mzs_expand_backup_select(mzs_handle* h, int32_t sim, const float* reward, const float* discount, const float* prior_logits,
                             const float* value, const float* next_embedding, int32_t* next_action_out,
                             float* next_parent_embedding_out, void* stream_) {
  if (h && (!next_action_out || !next_parent_embedding_out))
    return fail(h, MZS_E_INVALID, "mzs_expand_backup_select: null output");
  return expand_backup_impl(h, sim, reward, discount, prior_logits, value, next_embedding, next_action_out,
                            next_parent_embedding_out, stream_, "mzs_expand_backup_select");
}

int mzs_finish(mzs_handle* h, float temperature, const float* gumbel, int32_t* action_out,
               float* action_weights_out, float* search_value_out, int32_t* depth_sum_out, void* stream_) {
  return finish_impl(h, "mzs_finish", kDeterministic, "this handle runs the stochastic policy; use mzs_finish_stochastic",
                     temperature, gumbel, action_out, action_weights_out, search_value_out, depth_sum_out, stream_);
}

// ---- stochastic policy (policy == 2): the walking kernels with chance nodes at odd depth ----
static const char* const kNotStochastic = "this handle does not run the stochastic policy (policy 2)";

int mzs_root_stochastic(mzs_handle* h, const float* prior_logits, const float* value, const float* embedding,
                        const uint8_t* invalid_actions, const float* dirichlet_noise, float dirichlet_fraction,
                        const uint32_t key[2], void* stream_) {
  return root_dirichlet(h, "mzs_root_stochastic", kStochastic, kNotStochastic,
                        {prior_logits, value, embedding, invalid_actions, dirichlet_noise, dirichlet_fraction, nullptr, {0, 0}}, key,
                        stream_);
}

int mzs_select_stochastic(mzs_handle* h, int32_t sim, int32_t* slot_out, int32_t* parent_is_decision_out,
                          float* parent_embedding_out, void* stream_) {
  StepCall c;
  if (int rc = step_begin(h, "mzs_select_stochastic", kStochastic, kNotStochastic, true, sim,
                          !slot_out || !parent_is_decision_out || !parent_embedding_out ? "null output" : nullptr, stream_, &c))
    return rc;
  hipLaunchKernelGGL(mz::step_select_stochastic_kernel, c.grid, c.blk, 0, c.stream, c.sa, sim, slot_out, parent_is_decision_out,
                     parent_embedding_out);
  return launched(h);
}

int mzs_expand_backup_stochastic(mzs_handle* h, int32_t sim, const mzs_stochastic_outputs* o, void* stream_) {
  const char* bad = !o || o->struct_size != (int32_t)sizeof(mzs_stochastic_outputs) ? "null or size mismatch (ABI)"
                    : !o->chance_logits || !o->afterstate_value || !o->afterstate_embedding || !o->action_logits || !o->value ||
                          !o->reward || !o->discount || !o->state_embedding ? "null input" : nullptr;
  StepCall c;
  if (int rc = step_begin(h, "mzs_expand_backup_stochastic", kStochastic, kNotStochastic, true, sim, bad, stream_, &c)) return rc;
  const mz::StochasticOutputs k = {o->chance_logits, o->afterstate_value, o->afterstate_embedding, o->action_logits, o->value,
                                   o->reward, o->discount, o->state_embedding, h->cfg.afterstate_embed_dim, h->cfg.state_embed_dim};
  hipLaunchKernelGGL(mz::step_expand_backup_stochastic_kernel, c.grid, c.blk, 0, c.stream, c.sa, sim, k);
  return launched(h);
}

int mzs_finish_stochastic(mzs_handle* h, float temperature, const float* gumbel, int32_t* action_out, float* action_weights_out,
                          float* search_value_out, int32_t* depth_sum_out, void* stream_) {
  return finish_impl(h, "mzs_finish_stochastic", kStochastic, kNotStochastic, temperature, gumbel, action_out, action_weights_out,
                     search_value_out, depth_sum_out, stream_);
}

// ---- the default stochastic MLP family between the select and the expansion (mz_stoch_mlp.cuh) ----
// what keeps a handle (and, `w`, a weight set) off the one-launch recurrent step: null when it is served
static int stoch_mlp_refusal(mzs_handle* h, const char* who, int support_size) {
  const mzs_config& c = h->cfg;
  auto refuse = [&](int code, const char* what) { return fail(h, code, "%s", (std::string(who) + ": " + what).c_str()); };
  if (c.policy != 2) return refuse(MZS_E_INVALID, kNotStochastic);
  if (c.state_embed_dim != c.embed_dim || c.afterstate_embed_dim != c.embed_dim)
    return refuse(MZS_E_UNSUPPORTED, "state_embed_dim and afterstate_embed_dim must both equal embed_dim");
  if (c.num_actions + c.num_chance_outcomes > 64) return refuse(MZS_E_UNSUPPORTED, "num_actions + num_chance_outcomes > 64");
  if (support_size < 8 || support_size > 31) return refuse(MZS_E_UNSUPPORTED, "support_size must be 8..31");
  if (sizeof(float) * (size_t)mz::stoch_scratch_words(c.embed_dim, c.num_actions, c.num_chance_outcomes) > 64 * 1024)
    return refuse(MZS_E_UNSUPPORTED, "embedding too large for the LDS of a workgroup (64 KiB)");
  return MZS_OK;
}

int mzs_mlp_set_stochastic_weights(mzs_handle* h, const mzs_stochastic_mlp_weights* w) {
  if (!h) return MZS_E_INVALID;
  const char* who = "mzs_mlp_set_stochastic_weights";
  if (!w || w->struct_size != (int32_t)sizeof(mzs_stochastic_mlp_weights))
    return fail(h, MZS_E_INVALID, "%s: null or size mismatch (ABI)", who);
  if (int rc = stoch_mlp_refusal(h, who, w->support_size)) return rc;
  const float* const* wp = &w->ad_w1;
  for (int i = 0; i < 28; ++i)
    if (!wp[i]) return fail(h, MZS_E_INVALID, "%s: null weight array", who);
  h->sw = *w;
  h->have_stochastic_weights = true;
  return MZS_OK;
}

int mzs_mlp_stochastic_recurrent(mzs_handle* h, const int32_t* slot, const int32_t* parent_is_decision,
                                 const float* parent_embedding, const mzs_stochastic_outputs* o, void* stream_) {
  if (!h) return MZS_E_INVALID;
  const char* who = "mzs_mlp_stochastic_recurrent";
  const mzs_config& c = h->cfg;
  // (the weights' own limits are looked at once there are weights: a handle of another policy is told so first)
  if (c.policy == 2 && !h->have_stochastic_weights) return fail(h, MZS_E_INVALID, "%s: call mzs_mlp_set_stochastic_weights first", who);
  if (int rc = stoch_mlp_refusal(h, who, h->sw.support_size)) return rc;
  if (!o || o->struct_size != (int32_t)sizeof(mzs_stochastic_outputs)) return fail(h, MZS_E_INVALID, "%s: null or size mismatch (ABI)", who);
  if (!slot || !parent_is_decision || !parent_embedding) return fail(h, MZS_E_INVALID, "%s: null input", who);
  if (!o->chance_logits || !o->afterstate_value || !o->afterstate_embedding || !o->action_logits || !o->value || !o->reward ||
      !o->discount || !o->state_embedding)
    return fail(h, MZS_E_INVALID, "%s: null output", who);
  MZS_HIP(h, hipSetDevice(c.device));
  const mzs_stochastic_mlp_weights& s = h->sw;
  mz::StochMlp w;
  w.ad = {s.ad_w1, s.ad_b1, s.ad_w2, s.ad_b2}; w.av = {s.av_w1, s.av_b1, s.av_w2, s.av_b2};
  w.ac = {s.ac_w1, s.ac_b1, s.ac_w2, s.ac_b2}; w.cr = {s.cr_w1, s.cr_b1, s.cr_w2, s.cr_b2};
  w.cn = {s.cn_w1, s.cn_b1, s.cn_w2, s.cn_b2}; w.pv = {s.pv_w1, s.pv_b1, s.pv_w2, s.pv_b2};
  w.pp = {s.pp_w1, s.pp_b1, s.pp_w2, s.pp_b2};
  w.E = c.embed_dim; w.A = c.num_actions; w.C = c.num_chance_outcomes; w.F = 2 * s.support_size + 1;
  w.support = s.support_size; w.discount = s.discount;
  // (the struct's arrays are const for the expansion, which reads them; this entry is their writer)
  auto out = [](const float* p) { return const_cast<float*>(p); };
  const mz::StochRecurrentArgs a = {c.batch, slot, parent_is_decision, parent_embedding, out(o->chance_logits),
                                    out(o->afterstate_value), out(o->afterstate_embedding), out(o->action_logits), out(o->value),
                                    out(o->reward), out(o->discount), out(o->state_embedding)};
  const size_t lds = sizeof(float) * (size_t)mz::stoch_scratch_words(w.E, w.A, w.C);
  hipLaunchKernelGGL(mz::mz_stoch_mlp_recurrent_kernel, dim3(c.batch), dim3(64), lds, static_cast<hipStream_t>(stream_), w, a);
  return launched(h);
}

// ---- root inference of the bound family in the library (mz_stoch_wide.cuh: wave_root_state + the prediction heads) ----
int mzs_mlp_set_stochastic_representation(mzs_handle* h, int32_t obs_dim, const float* repr_w, const float* repr_b) {
  if (!h) return MZS_E_INVALID;
  const char* who = "mzs_mlp_set_stochastic_representation";
  if (h->cfg.policy != 2) return fail(h, MZS_E_INVALID, "%s", (std::string(who) + ": " + kNotStochastic).c_str());
  if (obs_dim < 1) return fail(h, MZS_E_INVALID, "%s: obs_dim must be at least 1", who);
  if (!repr_w || !repr_b) return fail(h, MZS_E_INVALID, "%s: null weight array", who);
  h->stoch_obs_dim = obs_dim;
  h->stoch_repr_w = repr_w;
  h->stoch_repr_b = repr_b;
  return MZS_OK;
}

// what the two entries that run root inference open with: the policy and the family's limits, weights and representation bound
static int stoch_root_refusal(mzs_handle* h, const char* who) {
  const mzs_config& c = h->cfg;
  if (c.policy == 2 && !h->have_stochastic_weights) return fail(h, MZS_E_INVALID, "%s: call mzs_mlp_set_stochastic_weights first", who);
  if (int rc = stoch_mlp_refusal(h, who, h->sw.support_size)) return rc;
  if (h->stoch_obs_dim < 1) return fail(h, MZS_E_INVALID, "%s: call mzs_mlp_set_stochastic_representation first", who);
  return MZS_OK;
}

int mzs_mlp_stochastic_root(mzs_handle* h, const float* obs, float* prior_logits_out, float* value_out, float* embedding_out,
                            void* stream_) {
  if (!h) return MZS_E_INVALID;
  const char* who = "mzs_mlp_stochastic_root";
  const mzs_config& c = h->cfg;
  if (int rc = stoch_root_refusal(h, who)) return rc;
  if (!obs) return fail(h, MZS_E_INVALID, "%s: null obs", who);
  if (!prior_logits_out || !value_out || !embedding_out) return fail(h, MZS_E_INVALID, "%s: null output", who);
  if (c.embed_dim > 64) return fail(h, MZS_E_UNSUPPORTED, "%s: embed_dim must be 1..64", who);
  MZS_HIP(h, hipSetDevice(c.device));
  const mzs_stochastic_mlp_weights& s = h->sw;
  mz::StochRootParams p = {};
  p.obs = obs; p.repr_w = h->stoch_repr_w; p.repr_b = h->stoch_repr_b;
  p.pv = {s.pv_w1, s.pv_b1, s.pv_w2, s.pv_b2}; p.pp = {s.pp_w1, s.pp_b1, s.pp_w2, s.pp_b2};
  p.prior_logits = prior_logits_out; p.value = value_out; p.embedding = embedding_out;
  p.B = c.batch; p.obs_dim = h->stoch_obs_dim; p.E = c.embed_dim; p.A = c.num_actions; p.F = 2 * s.support_size + 1;
  p.support = s.support_size;
  std::string err;
  if (int rc = mz::stoch_root_launch(p, static_cast<hipStream_t>(stream_), &err))
    return fail(h, rc, "%s", (std::string(who) + ": " + err).c_str());
  return MZS_OK;
}

// ---- the whole stochastic search of the bound family in ONE launch, the tree in LDS (mz_stoch_wide.cuh) ----
// with_obs: root inference inside the launch on `obs`, else the RootFnOutput arrays of `a`; draw_alpha: null, or the root
// noise drawn inside the launch with this alpha (mzs_mlp_stochastic_search_draw), its rows into noise_out when set
static int stoch_search(mzs_handle* h, const char* who, const mzs_stochastic_search_args* a, const float* obs,
                        float* root_value_out, bool with_obs, const float* draw_alpha, float* noise_out, void* stream_) {
  const mzs_config& c = h->cfg;
  if (with_obs) {
    if (int rc = stoch_root_refusal(h, who)) return rc;
  } else {
    if (c.policy == 2 && !h->have_stochastic_weights) return fail(h, MZS_E_INVALID, "%s: call mzs_mlp_set_stochastic_weights first", who);
    if (int rc = stoch_mlp_refusal(h, who, h->sw.support_size)) return rc;
  }
  if (!a || a->struct_size != (int32_t)sizeof(mzs_stochastic_search_args)) return fail(h, MZS_E_INVALID, "%s: null or size mismatch (ABI)", who);
  if (with_obs) {
    if (!obs) return fail(h, MZS_E_INVALID, "%s: null obs", who);
    if (!root_value_out) return fail(h, MZS_E_INVALID, "%s: null root_value_out", who);
    if (a->prior_logits || a->value || a->embedding)
      return fail(h, MZS_E_INVALID, "%s: prior_logits, value and embedding must be NULL (the kernel computes them from obs)", who);
  } else if (!a->prior_logits || !a->value || !a->embedding) {
    return fail(h, MZS_E_INVALID, "%s: null input", who);
  }
  if (!a->action || !a->action_weights) return fail(h, MZS_E_INVALID, "%s: null output", who);
  if (draw_alpha) {
    if (a->dirichlet_noise) return fail(h, MZS_E_INVALID, "%s: dirichlet_noise must be NULL (the kernel draws the noise)", who);
    if (!(*draw_alpha > 0.0f) || std::isinf(*draw_alpha))
      return fail(h, MZS_E_INVALID, "%s: dirichlet_alpha must be positive and finite", who);
  } else if (!a->dirichlet_noise && a->dirichlet_fraction != 0.0f && !a->device_block) {
    return fail(h, MZS_E_INVALID, "%s: dirichlet_fraction != 0 needs dirichlet_noise", who);
  }
  const mzs_stochastic_mlp_weights& s = h->sw;
  mz::WidePlan pl;
  if (const char* limit = mz::stoch_wide_plan(c.num_actions, c.num_chance_outcomes, c.embed_dim, 2 * s.support_size + 1,
                                              c.num_simulations, &pl))
    return fail(h, MZS_E_UNSUPPORTED, "%s", (std::string(who) + ": " + limit).c_str());
  MZS_HIP(h, hipSetDevice(c.device));
  const bool ex = a->export_tree != 0;
  if (ex)
    if (int rc = ensure_step_state(h)) return rc;
  const size_t BN = (size_t)c.batch * (c.num_simulations + 1);
  if (!pl.emb_lds && !ex && !h->fused_emb)
    MZS_HIP(h, hipMalloc(reinterpret_cast<void**>(&h->fused_emb), BN * c.embed_dim * sizeof(float)));
  mz::StochWideParams p = {};
  p.prior_logits = a->prior_logits; p.value = a->value; p.embedding = a->embedding;
  if (with_obs) {
    p.obs = obs; p.repr_w = h->stoch_repr_w; p.repr_b = h->stoch_repr_b; p.obs_dim = h->stoch_obs_dim;
    p.root_value_out = root_value_out;
  }
  p.invalid = a->invalid_actions; p.dirichlet_noise = a->dirichlet_noise; p.gumbel = a->gumbel;
  memcpy(p.w, &s.ad_w1, sizeof p.w);
  p.action = a->action; p.action_weights = a->action_weights; p.search_value = a->search_value; p.depth_sum = a->depth_sum;
  if (ex) {
    const mz::StepState& t = h->step;
    p.t_node_visits = t.node_visits; p.t_raw_values = t.raw_values; p.t_node_values = t.node_values;
    p.t_parents = t.parents; p.t_action_from_parent = t.action_from_parent;
    p.t_children_index = t.children_index; p.t_children_prior_logits = t.children_prior_logits;
    p.t_children_prior_probs = t.children_prior_probs; p.t_children_values = t.children_values;
    p.t_children_visits = t.children_visits; p.t_children_rewards = t.children_rewards;
    p.t_children_discounts = t.children_discounts; p.t_embeddings = t.embeddings;
    p.t_root_invalid = t.root_invalid; p.t_depth_sum = t.depth_sum;
  }
  p.emb_scratch = h->fused_emb;
  p.dyn = a->device_block;
  p.B = c.batch; p.A = c.num_actions; p.C = c.num_chance_outcomes; p.E = c.embed_dim; p.F = 2 * s.support_size + 1;
  p.support = s.support_size; p.S = c.num_simulations; p.max_depth = c.max_depth; p.export_tree = ex;
  p.pb_c_init = c.pb_c_init; p.pb_c_base = c.pb_c_base; p.dirichlet_fraction = a->dirichlet_fraction;
  p.discount = s.discount; p.temperature = a->temperature;
  p.global_batch = (uint64_t)c.global_batch; p.root_offset = (uint64_t)c.root_offset;
  mzh::derive_keys(a->key, c.num_simulations, p.k_sample, &p.sim_keys[0][0]);  // num_simulations <= 255 (the plan)
  if (draw_alpha) {
    mzh::h_split(a->key, 3, 1, p.k_dirichlet);  // mctx: rng_key, dirichlet_rng_key, search_rng_key = split(rng_key, 3)
    p.dirichlet_alpha = *draw_alpha;
    p.noise_out = noise_out;
  }
  std::string err;
  if (int rc = mz::stoch_wide_launch(c.tiebreak != 0, with_obs, draw_alpha != nullptr, c.device, p, pl,
                                     static_cast<hipStream_t>(stream_), &err))
    return fail(h, rc, "%s", (std::string(who) + ": " + err).c_str());
  if (ex) h->step.rooted = true;  // the HBM tree is that of a finished step-wise search: mzs_tree_export serves it
  return MZS_OK;
}

int mzs_mlp_stochastic_search(mzs_handle* h, const mzs_stochastic_search_args* a, void* stream_) {
  if (!h) return MZS_E_INVALID;
  return stoch_search(h, "mzs_mlp_stochastic_search", a, nullptr, nullptr, false, nullptr, nullptr, stream_);
}

int mzs_mlp_stochastic_search_obs(mzs_handle* h, const mzs_stochastic_search_args* a, const float* obs, float* root_value_out,
                                  void* stream_) {
  if (!h) return MZS_E_INVALID;
  return stoch_search(h, "mzs_mlp_stochastic_search_obs", a, obs, root_value_out, true, nullptr, nullptr, stream_);
}

int mzs_mlp_stochastic_search_draw(mzs_handle* h, const mzs_stochastic_search_args* a, const float* obs, float* root_value_out,
                                   float dirichlet_alpha, float* noise_out, void* stream_) {
  if (!h) return MZS_E_INVALID;
  return stoch_search(h, "mzs_mlp_stochastic_search_draw", a, obs, root_value_out, obs != nullptr, &dirichlet_alpha, noise_out,
                      stream_);
}

int mzs_tree_export(mzs_handle* h, const mzs_tree_view* out, void* stream_) {
  if (!h) return MZS_E_INVALID;
  if (!h->step.rooted) return fail(h, MZS_E_INVALID, "mzs_tree_export: no step-wise tree (call mzs_root first)");
  if (!out) return fail(h, MZS_E_INVALID, "mzs_tree_export: null view");
  const void* const* tp = reinterpret_cast<const void* const*>(out);
  for (int i = 0; i < 12; ++i)
    if (!tp[i]) return fail(h, MZS_E_INVALID, "mzs_tree_export: tree view has a null array");
  const mzs_config& c = h->cfg;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  MZS_HIP(h, hipSetDevice(c.device));
  const size_t BN = (size_t)c.batch * (c.num_simulations + 1);
  const size_t A = (size_t)mz::slots_per_node(c);
  const mz::StepState& s = h->step;
#define CP(dst, src, n) MZS_HIP(h, hipMemcpyAsync(dst, src, (n) * 4, hipMemcpyDeviceToDevice, stream))
  CP(out->node_visits, s.node_visits, BN); CP(out->raw_values, s.raw_values, BN);
  CP(out->node_values, s.node_values, BN); CP(out->parents, s.parents, BN);
  CP(out->action_from_parent, s.action_from_parent, BN);
  CP(out->children_index, s.children_index, BN * A);
  CP(out->children_prior_logits, s.children_prior_logits, BN * A);
  CP(out->children_values, s.children_values, BN * A);
  CP(out->children_visits, s.children_visits, BN * A);
  CP(out->children_rewards, s.children_rewards, BN * A);
  CP(out->children_discounts, s.children_discounts, BN * A);
  CP(out->embeddings, s.embeddings, BN * c.embed_dim);
#undef CP
  return MZS_OK;
}

}  // extern "C"

// the generic route's ONE search launch over `n` roots (round 6: MuZero-policy instances specialised on the 16-lane slots
// the action count fills, with the pUCT table in LDS while it fits the workgroup's 64 KB)
static void launch_mlp_search(const mzs_config& c, const mz::StepArgs& sa, const mz::JumpArgs& ja, const mz::MlpGen& g, int n,
                              size_t lds_search, hipStream_t stream) {
  const size_t lds_tbl = lds_search + sizeof(float) * 2 * ((size_t)sa.S + 2);
  const bool tbl = sa.S + 2 <= 1030 && lds_tbl <= 64 * 1024;  // (Markstein's sequence is checked for every divisor up to 1030)
  // the 128-register build (four wavefronts per SIMD, mz_mlp_generic.cuh) where it puts MORE roots on the chip: more roots
  // than two wavefronts per SIMD hold, and workgroups small enough that sixteen share a CU's LDS
  const size_t lds = (c.policy != 1 && tbl && sa.A <= 32) ? lds_tbl : lds_search;
  const bool occ4 = n > 2 * 4 * 256 && 16 * lds <= 160 * 1024;
#define MZ_GEN_LAUNCH(...)                                                                                            \
  do {                                                                                                                \
    if (occ4) hipLaunchKernelGGL((mz::mz_mlp_search_kernel_occ4<__VA_ARGS__>), dim3(n), dim3(64), lds, stream, sa, ja, g, 0, sa.S); \
    else hipLaunchKernelGGL((mz::mz_mlp_search_kernel<__VA_ARGS__>), dim3(n), dim3(64), lds, stream, sa, ja, g, 0, sa.S);           \
  } while (0)
  if (c.policy == 1) MZ_GEN_LAUNCH(true);
  else if (tbl && sa.A <= 16) MZ_GEN_LAUNCH(false, 1, true);
  else if (tbl && sa.A <= 32) MZ_GEN_LAUNCH(false, 2, true);
  else MZ_GEN_LAUNCH(false);
#undef MZ_GEN_LAUNCH
}
// rows [rb, rb + n) of the step-wise tree as a batch of their own: every per-root array starts at row rb, the PRNG streams
// stay those of the global root index (root_offset + rb)
static mz::StepArgs slice_rows(mz::StepArgs s, size_t rb, int n) {
  const size_t N = (size_t)s.N, A = (size_t)s.A, E = (size_t)s.E;
  s.B = n;
  s.root_offset += rb;
  s.node_visits += rb * N; s.raw_values += rb * N; s.node_values += rb * N; s.parents += rb * N;
  s.action_from_parent += rb * N; s.path += rb * N;
  s.children_index += rb * N * A; s.children_prior_logits += rb * N * A; s.children_prior_probs += rb * N * A;
  s.children_values += rb * N * A; s.children_visits += rb * N * A; s.children_rewards += rb * N * A;
  s.children_discounts += rb * N * A; s.embeddings += rb * N * E;
  s.root_invalid += rb * A; s.root_gumbel += rb * A;
  s.sel_parent += rb; s.sel_action += rb; s.sel_depth += rb; s.depth_sum += rb; s.xfer_node += rb;
  return s;
}
// The generic route for a tree whose B N^2 cached path words exceed the slab budget (4096 roots x 1000 simulations would
// be 16 GB): the handle's slab holds `jump_roots` roots and the batch is searched in chunks of that many -- root /
// select(0) / ONE search launch / finish per chunk on the caller's stream, the slab reused chunk after chunk (stream order),
// the tree arrays those of the whole batch (an export copies them as ever).  Same kernels, same per-root PRNG streams
// (root_offset + row), hence the same bits as the undivided launch.
static int act_mlp_generic_chunks(mzs_handle* h, const mzs_act_args* a, const mz::MlpGen& g, float* pl, float* emb,
                                  int32_t* act0, size_t lds_search, hipStream_t stream) {
  const mzs_config& c = h->cfg;
  const size_t A = (size_t)c.num_actions, E = (size_t)c.embed_dim;
  uint32_t gk[2] = {0, 0};
  if (c.policy == 1) {
    mzh::h_split(a->key, 2, 1, gk);  // mctx gumbel_muzero_policy: rng_key, gumbel_rng = split(rng_key)
  } else {
    if (int rc = seed_tree_keys(h, a->key, stream)) return rc;
  }
  const mz::StepArgs whole = h->step.args(c);
  const bool gum = c.policy == 1;
  for (size_t rb = 0; rb < (size_t)c.batch; rb += (size_t)h->jump_roots) {
    const int n = (int)std::min((size_t)h->jump_roots, (size_t)c.batch - rb);
    const mz::StepArgs sa = slice_rows(whole, rb, n);
    auto rows = [&](auto* p, size_t stride) { return p ? p + rb * stride : nullptr; };  // row rb of an optional [B, stride] array
    launch_root(h, sa, {pl + rb * A, a->root_value + rb, emb + rb * E, rows(a->invalid_actions, A),
                        gum ? nullptr : rows(a->dirichlet_noise, A), gum ? 0.0f : a->dirichlet_fraction,
                        gum ? rows(a->gumbel, A) : nullptr, {gk[0], gk[1]}}, true, stream);
    hipLaunchKernelGGL(mz::jump_select_kernel<false>, dim3(step_grid(n)), dim3(step_block(n)), 0, stream, sa, h->jump, 0,
                       act0 + rb, emb + rb * E);
    launch_mlp_search(c, sa, h->jump, g, n, lds_search, stream);
    launch_finish(h, sa, a->temperature, rows(a->gumbel, A), a->action + rb, a->action_weights + rb * A,
                  rows(a->search_value, 1), rows(a->depth_sum, 1), stream);
    MZS_HIP(h, hipGetLastError());
  }
  h->step.rooted = true;
  if (a->tree) return mzs_tree_export(h, a->tree, stream);
  return MZS_OK;
}
// act() of the default MLP trio for shapes the fused kernel has no instance for (mz_mlp_generic.cuh): root inference,
// mzs_root, mzs_select(0), ONE launch for all simulations, mzs_finish -- five launches per act instead of two per
// simulation, the nets evaluated by the library to the project's arithmetic spec (== the oracle for any shape).
int mzh::act_mlp_generic(mzs_handle* h, const mzs_act_args* a, void* stream_) {
  const mzs_config& c = h->cfg;
  const mzs_mlp_weights& w = h->w;
  const int A = c.num_actions, E = c.embed_dim, F = 2 * w.support_size + 1, S = c.num_simulations;
  if (F < 17 || F > 64 || A > 64)
    return fail(h, MZS_E_UNSUPPORTED, "mzs_act_mlp (generic route): support_size must be 8..31 and num_actions <= 64");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  MZS_HIP(h, hipSetDevice(c.device));  // (reached before mzs_act_mlp's own hipSetDevice when num_simulations > kMaxSims)
  if (int rc = ensure_step_state(h)) return rc;
  if (h->jump_roots < 1 || (!h->use_jump && E >= mz::kWideEmb))
    return fail(h, MZS_E_UNSUPPORTED, "mzs_act_mlp (generic route): no cached-decision slab for this tree (more than 1023 "
                                      "simulations, MZS_STEP_WALK=1, or out of device memory); use the step-wise path");
  const size_t B = (size_t)c.batch;
  if (!h->gen_scratch) MZS_HIP(h, hipMalloc(reinterpret_cast<void**>(&h->gen_scratch), (B * A + B * E + B) * sizeof(float)));
  float* pl = h->gen_scratch;
  float* emb = pl + B * A;
  int32_t* act0 = reinterpret_cast<int32_t*>(emb + B * E);
  mz::MlpGen g;
  mzh::copy_weights(w, g);
  g.obs_dim = w.obs_dim; g.E = E; g.A = A; g.F = F; g.support = w.support_size; g.pred_on_parent = w.recurrent_pred_on;
  g.discount = w.discount;
  const size_t lds_root = sizeof(float) * (size_t)mz::gen_scratch_words(mz::gen_obs_width(E, w.obs_dim), A);
  const size_t lds_search = sizeof(int32_t) * 15 * ((size_t)S + 2) + sizeof(float) * (size_t)mz::gen_scratch_words(E, A);
  if (lds_root > 64 * 1024 || lds_search > 64 * 1024)
    return fail(h, MZS_E_UNSUPPORTED, "mzs_act_mlp (generic route): num_simulations / embedding too large for the LDS of a workgroup");
  hipLaunchKernelGGL(mz::mz_mlp_root_kernel, dim3(c.batch), dim3(64), lds_root, stream, g, c.batch, a->obs, pl, a->root_value, emb);
  MZS_HIP(h, hipGetLastError());
  if (!h->use_jump) return act_mlp_generic_chunks(h, a, g, pl, emb, act0, lds_search, stream);
  int rc = c.policy == 1 ? mzs_root_gumbel(h, pl, a->root_value, emb, a->invalid_actions, a->gumbel, a->key, stream_)
                         : mzs_root(h, pl, a->root_value, emb, a->invalid_actions, a->dirichlet_noise, a->dirichlet_fraction,
                                    a->key, stream_);
  if (rc) return rc;
  if ((rc = mzs_select(h, 0, act0, emb, stream_))) return rc;  // simulate() of simulation 0 (emb: consumed by mzs_root, reused)
  mz::StepArgs sa = h->step.args(c);
  launch_mlp_search(c, sa, h->jump, g, c.batch, lds_search, stream);
  MZS_HIP(h, hipGetLastError());
  if ((rc = mzs_finish(h, a->temperature, c.policy == 1 ? nullptr : a->gumbel, a->action, a->action_weights, a->search_value,
                       a->depth_sum, stream_)))
    return rc;
  if (a->tree) return mzs_tree_export(h, a->tree, stream_);
  return MZS_OK;
}

#ifdef MZ_PROFILE
// tools-only entry point (not part of the ABI): the tree-step phase counters of THIS translation unit's kernels (the
// generic one-launch search, the step-wise launches): read and clear (tools/profile_generic.py)
extern "C" int mzs_debug_generic_jump_profile(uint64_t* host_out, int32_t words) {
  static unsigned long long zero[1024 * 8];
  if (words > 1024 * 8) words = 1024 * 8;
  if (hipMemcpyFromSymbol(host_out, HIP_SYMBOL(mz::g_jump_prof), sizeof(uint64_t) * (size_t)words) != hipSuccess) return MZS_E_RUNTIME;
  if (hipMemcpyToSymbol(HIP_SYMBOL(mz::g_jump_prof), zero, sizeof(zero)) != hipSuccess) return MZS_E_RUNTIME;
  return MZS_OK;
}
#endif
