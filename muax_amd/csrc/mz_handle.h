// mz_handle.h -- the handle behind the C-ABI and the host helpers its routes share (not part of the ABI): mz_api.hip,
// mz_act.hip, mz_stepwise.hip.  (Types and device functions of the step-wise path only: its kernels are in
// mz_step_kernels.cuh, which mz_stepwise.hip alone includes.)
#pragma once
#include <string>
#include <vector>

#include "mz_host.h"
#include "mz_keys.h"
#include "mz_step_jump.cuh"

struct mzs_handle {
  mzs_config cfg;
  std::string err;
  bool have_weights = false;
  mzs_mlp_weights w;
  mz::StepState step;  // device buffers of the step-wise path (lazily allocated)
  uint32_t k_sample[2] = {0, 0};
  std::vector<uint32_t> sim_keys;  // [num_simulations][2], sized at create: simulate_key of every simulation
  uint64_t* prof = nullptr;        // MZ_PROFILE builds only
  int32_t* fused_table = nullptr;  // gumbel policy, fused path: seq_halving table on the device
  float* fused_emb = nullptr;      // fused path, embed_dim > 16, and the one-launch stochastic search: [B][S+1][E] embeddings in HBM
  int32_t* fused_path = nullptr;   // fused path, instances with the root paths in HBM: [B][S+1][fused_path_words]
  int fused_path_words = 0;
  int cu_count = 0;
  // mzs_act_mlp_host: pinned staging (in: obs | noise | invalid, out: action | weights | value) and their device twins
  void* host_in = nullptr; void* host_out = nullptr; void* dev_noise = nullptr;  // dev_noise: [B, A] drawn root noise
  size_t host_in_bytes = 0;
  mz::JumpArgs jump = {nullptr, nullptr, nullptr, nullptr};  // step-wise path with cached decisions
  void* jump_slab = nullptr;
  bool use_jump = false;
  int jump_roots = 0;              // roots the cached-decision slab holds: the batch (use_jump), or -- generic route of trees whose
                                   // B N^2 path words exceed the budget -- the chunk of roots act() searches at a time
  bool allow_generic = false;      // mzs_mlp_allow_generic: shapes without a fused instance take the generic one-launch search
  float* gen_scratch = nullptr;    // generic route: prior logits [B, A] | embeddings [B, E] | actions [B]
  bool allow_wide = false;         // mzs_mlp_allow_wide: 17..64 actions under the MuZero policy take the wide one-launch kernel
  bool allow_wide_gumbel = false;  // mzs_mlp_allow_wide_gumbel: ... and under the Gumbel policy (a handle opts in separately)
  bool have_stochastic_weights = false;  // mzs_mlp_set_stochastic_weights: the default stochastic MLP family (policy 2)
  mzs_stochastic_mlp_weights sw = {};
  int32_t stoch_obs_dim = 0;  // mzs_mlp_set_stochastic_representation (0: not bound): the family's root inference in the library
  const float *stoch_repr_w = nullptr, *stoch_repr_b = nullptr;
};

namespace mzh {

// act() of the default MLP trio on the step-wise tree with ONE search launch (mz_stepwise.hip): what mzs_act_mlp falls
// back to, with mzs_mlp_allow_generic, for shapes no fused or wide instance serves
int act_mlp_generic(mzs_handle* h, const mzs_act_args* a, void* stream);

}  // namespace mzh
