// mz_stoch_wide_launch.h -- host interface of the one-launch stochastic search (mz_stoch_wide.cuh, compiled in
// mz_stoch_wide.hip): its argument block, its LDS plan and its launch.
#pragma once
#include <string>

#include "mz_wide_launch.h"

namespace mz {

// LDS budget of the stochastic kernel, in 4-byte words (wide_fit: all blocks rounded to 16 bytes):
//   workgroup: the seven heads' weights + the pUCT table [S + 2]
//   root:      (S + 1) records of 4 header words + 4 child fields x (A + C) slots, the path [S + 1], and -- when it costs
//              no resident root -- the embeddings [S + 1][E]
inline int stoch_weight_words(int A, int C, int E, int F) {
  const int H = kHidden;
  auto head = [&](int n_in, int n_out) { return n_in * H + H + H * n_out + n_out; };
  return head(E + A, E) + head(E, F) + head(E, C) + head(E + C, F) + head(E + C, E) + head(E, F) + head(E, A);
}
// What keeps a shape off the kernel, in the caller's words (null: the plan admits it and *out is set)
inline const char* stoch_wide_plan(int A, int C, int E, int F, int S, WidePlan* out) {
  if (A < 1 || C < 1) return "num_actions and num_chance_outcomes must be at least 1";
  if (A + C > 64) return "num_actions + num_chance_outcomes > 64";
  if (E < 1 || E > 64) return "embed_dim must be 1..64";
  if (F < 17 || F > 63) return "support_size must be 8..31";
  if (S < 1 || S > 255) return "num_simulations must be 1..255";
  if (!wide_fit(wide_round4(stoch_weight_words(A, C, E, F)), 4 + 4 * (A + C), E, S, out))
    return "one root's tree is too large for the LDS of a CU (160 KiB)";
  return nullptr;
}

// Per-call values a captured launch must not freeze, as a DEVICE block of 4 + 2 S words (mzs_stochastic_search_block
// fills the host copy): k_sample[2], the bits of temperature and dirichlet_fraction, every simulation's key.  The DRAW
// instantiations read kStochBlockDrawTail more words behind them (mzs_stochastic_search_block_draw): the Dirichlet key's
// two words and the bits of dirichlet_alpha
constexpr int kStochBlockHead = 4, kStochBlockDrawTail = 3;

struct StochWideParams {
  // RootFnOutput and the root's options ([B, A]; invalid, dirichlet_noise, gumbel may be null)
  const float *prior_logits, *value, *embedding;
  const uint8_t* invalid;
  const float *dirichlet_noise, *gumbel;
  const float* w[28];  // the seven heads, w1 b1 w2 b2 each, in the order of mzs_stochastic_mlp_weights
  // outputs (search_value, depth_sum may be null)
  int32_t* action;
  float* action_weights;  // [B, A]
  float* search_value;
  int32_t* depth_sum;
  // the handle's HBM tree (StepState), written with export_tree: [B, N], [B, N, A + C], [B, N, E], root_invalid [B, A + C]
  int32_t* t_node_visits; float* t_raw_values; float* t_node_values;
  int32_t* t_parents; int32_t* t_action_from_parent;
  int32_t* t_children_index; float* t_children_prior_logits; float* t_children_prior_probs; float* t_children_values;
  int32_t* t_children_visits; float* t_children_rewards; float* t_children_discounts;
  float* t_embeddings;
  uint8_t* t_root_invalid;
  int32_t* t_depth_sum;
  float* emb_scratch;   // [B][S + 1][E]: embeddings out of LDS and no export
  const uint32_t* dyn;  // device block (above) or null: k_sample, temperature, dirichlet_fraction, sim_keys below
  int32_t B, A, C, E, F, support, S, max_depth, export_tree;
  float pb_c_init, pb_c_base, dirichlet_fraction, discount, temperature;
  uint64_t global_batch, root_offset;
  uint32_t k_sample[2];
  uint32_t sim_keys[kMaxSims][2];
  // root inference inside the launch (the kernel's ROOT instantiations; prior_logits, value, embedding are then null):
  // obs [B, obs_dim], the representation's repr_w [obs_dim, E] and repr_b [E] in HBM, the root's network value out [B]
  const float *obs, *repr_w, *repr_b;
  float* root_value_out;
  int32_t obs_dim;
  // the root noise drawn inside the launch (the kernel's DRAW instantiations; dirichlet_noise is then null): the call's
  // Dirichlet key split(key, 3)[1] and alpha -- both from the device block's tail when there is one --, the drawn rows
  // out [B, A] or null
  float dirichlet_alpha;
  uint32_t k_dirichlet[2];
  float* noise_out;
};

// tiebreak: the handle's (the kernel's mode 1); root: p.obs set, root inference inside the launch; draw: the root noise
// drawn inside the launch.  MZS_OK after the launch, or a negative MZS_E_* with *err set.
int stoch_wide_launch(bool tiebreak, bool root, bool draw, int device, const StochWideParams& p, const WidePlan& pl,
                      hipStream_t stream, std::string* err);

// Root inference of the family on its own (mz_stoch_root_kernel): one wavefront per root, no LDS.  E, A <= 64, F <= 63.
struct StochRootParams {
  const float *obs, *repr_w, *repr_b;  // [B, obs_dim], [obs_dim, E], [E]
  Mlp2 pv, pp;                         // the prediction heads in HBM
  float *prior_logits, *value, *embedding;  // out [B, A], [B], [B, E]
  int32_t B, obs_dim, E, A, F, support;
};
int stoch_root_launch(const StochRootParams& p, hipStream_t stream, std::string* err);

}  // namespace mz
