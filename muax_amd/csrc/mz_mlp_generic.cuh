// mz_mlp_generic.cuh -- the default MLP trio (muax/nn.py:59-115) with RUN-TIME shapes, and a whole search on it in one
// launch, for the shapes the fused kernel (mz_fused.cuh: tree in LDS, weights in registers, templates over every
// width) has no instance for and cannot be instantiated for: more than 8 actions, more than 127 simulations,
// embeddings wider than 64.  The reference's act() takes any of them (muax/model.py:82-96).
//
//   root:    obs -> Representation -> Prediction -> (prior_logits, value, embedding) arrays  (muax/model.py:251-263);
//            the tree kernels of the step-wise path take it from there (mzs_root / mzs_select);
//   search:  ONE launch for all simulations, one wavefront per root:  gather the parent's embedding row from the tree ->
//            Dynamic + Prediction (muax/model.py:265-282) -> next state written into the new node's row -> mctx's expand
//            / backward / next simulate with the cached decisions of mz_step_jump.cuh (tree in HBM / L2, A <= 64,
//            num_simulations <= 1023).  4096 roots are 4 wavefronts per SIMD: the memory round trips of one root's tree
//            step hide behind the other roots'.
//
// The nets are the run-time-shape blocks and stages of mz_mlp_blocks.cuh (the project's one arithmetic spec, "MZ-F32").
#pragma once
#include "mz_mlp_blocks.cuh"
#include "mz_step_jump.cuh"

#pragma clang fp contract(off)

namespace mz {

// muax/model.py:251-263 for every root: one wavefront per root
__global__ __launch_bounds__(64) void mz_mlp_root_kernel(const MlpGen w, int B, const float* obs, float* prior_logits, float* value,
                                                         float* embedding) {
  extern __shared__ float gen_f[];
  const int r = blockIdx.x, tid = threadIdx.x;
  if (r >= B) return;
  const GenLds G = gen_lds(gen_f, gen_obs_width(w.E, w.obs_dim), w.A);
  gen_embed(w.repr_w, w.repr_b, obs + (size_t)r * w.obs_dim, w.obs_dim, w.E, G, tid);
  const Mlp2 pv = w.pv(), pp = w.pp();
  gen_prediction(pv, pp, true, w.A, w.E, w.F, w.support, G, G.ns, tid);
  for (int e = tid; e < w.E; e += 64) embedding[(size_t)r * w.E + e] = G.ns[e];
  for (int j = tid; j < w.A; j += 64) prior_logits[(size_t)r * w.A + j] = G.pl[j];
  if (tid == 0) value[r] = G.scal[1];
}

// all simulations [sim_begin, sim_end) of every root (simulate() of sim_begin has run: mzs_select)
// AS (round 6, MuZero policy): the 16-lane slots the action count fills (1: A <= 16, 2: A <= 32; 0: any A <= 64) -- the tree
// step's decision refresh without the run-time tests of the general code's four slots (mz_step_jump.cuh, level_load); TBL:
// the {sqrt(n) pb_c(n), RN(1 / n)} table behind the trio's scratch (visit counts up to 1030: Markstein's checked range)
template <bool GUMBEL, int AS, bool TBL, bool U32>
MZ_DEV void mlp_search_body(const StepArgs& s, const JumpArgs& g, const MlpGen& w, int sim_begin, int sim_end) {
  extern __shared__ int gen_i[];
  const int r = blockIdx.x, tid = threadIdx.x;
  if (r >= s.B) return;
  const int N = s.N, A = s.A, E = s.E;
  const size_t rb = (size_t)r * N;
  int* tree_lds = gen_i;
  const GenLds G = gen_lds(reinterpret_cast<float*>(gen_i + 15 * (N + 1)), E, A);
  float* score_tbl = nullptr;
  if constexpr (TBL) {
    score_tbl = reinterpret_cast<float*>(gen_i + 15 * (N + 1)) + gen_scratch_words(E, A);
    for (int n = tid; n < N + 1; n += 64) {
      score_tbl[2 * n] = puct_scale(n, s.pb_c_init, s.pb_c_base);
      score_tbl[2 * n + 1] = n > 0 ? 1.0f / (float)n : 0.0f;
    }
    __syncthreads();
  }
  const Mlp2 pv = w.pv(), pp = w.pp();
  TreeView T = tree_view_global(s, g, rb);
  if constexpr (AS != 0) {  // the root's invalid-action mask once per launch, not a load in front of level 0's scores every time
    T.inv_bits = 0;
#pragma unroll
    for (int t = 0; t < AS; ++t) {
      const int a = (tid & 15) + 16 * t;
      if (a < A && s.root_invalid[(size_t)r * A + a]) T.inv_bits |= 1 << t;
    }
  }
  int parent = s.sel_parent[r], action = s.sel_action[r], depth = s.sel_depth[r];
  int newn;
  {
    const int next = s.children_index[(rb + parent) * A + action];
    newn = next == -1 ? sim_begin + 1 : next;
  }
  for (int sim = sim_begin; sim < sim_end; ++sim) {
    // recurrent_fn: Dynamic on [s, onehot(a)], Prediction on the next state (or the parent's, pip-release quirk)
    gen_stage_input(G, s.embeddings + (rb + parent) * E, E, A, action, tid);
    // gen_next_state, written out: through the shared stage the 128-register build at A <= 16 measured 2.6 % slower
    // (profiles/mlp_blocks_refactor.txt); like this both builds keep the instruction stream they had
    if (tid < 32) {
      const int u = tid & 15;
      const float a = (tid < 16) ? gen_linear<U32>(G.sa, E + A, w.dr_w1, w.dr_b1, kHidden, u)
                                 : gen_linear<U32>(G.sa, E + A, w.dn_w1, w.dn_b1, kHidden, u);
      G.hid[tid] = elu(a);
    }
    __syncthreads();
    for (int j = tid; j < w.F; j += 64) G.rl[j] = gen_linear<U32>(G.hid, kHidden, w.dr_w2, w.dr_b2, w.F, j);
    for (int e = tid; e < E; e += 64) G.ns[e] = gen_linear<U32>(G.hid + 16, kHidden, w.dn_w2, w.dn_b2, E, e);
    __syncthreads();
    gen_min_max_normalize(G.ns, E, tid);
    __syncthreads();
    float* nrow = s.embeddings + (rb + newn) * E;
    for (int e = tid; e < E; e += 64) nrow[e] = G.ns[e];
    gen_reward_decode(G, w.F, w.support, tid);
    gen_prediction<U32>(pv, pp, true, w.A, w.E, w.F, w.support, G, w.pred_on_parent ? G.sa : G.ns, tid);
    const float rew = G.scal[0], val = G.scal[1];
    const int known[4] = {parent, action, depth, newn};
    int sel[3] = {0, 0, 0};
    jump_expand_backup_body<GUMBEL, kLevelsInFlight, AS, TBL>(s, g, T, sim, r, tree_lds, rew, w.discount, G.pl, val, nullptr, true, nullptr,
                                                              nullptr, sel, known, 0, score_tbl);
    if (sim + 1 < sim_end && sim + 1 < s.S) {
      parent = sel[0];
      action = sel[1];
      depth = sel[2];
      const int next = s.children_index[(rb + parent) * A + action];
      newn = next == -1 ? sim + 2 : next;
    }
    __syncthreads();
  }
}
// As compiled the search needs 168 .. 181 VGPRs = TWO wavefronts per SIMD: 2048 roots resident, 4096 roots two rounds (per
// simulation 18.6 us at 1024 roots, 21.7 at 2048, 41.9 at 4096).  _occ4: the same body held to 128 registers (four
// wavefronts per SIMD; ~25 loop invariants spilled to scratch) for launches of more roots than two wavefronts per SIMD
// hold whose workgroups fit sixteen to a CU's LDS -- 1.2 - 1.3x there, slower everywhere else (the host chooses:
// mz_stepwise.hip, launch_mlp_search; both measured in profiles/r06_generic_notes.txt).
template <bool GUMBEL, int AS = 0, bool TBL = false>
__global__ __launch_bounds__(64) void mz_mlp_search_kernel(const StepArgs s, const JumpArgs g, const MlpGen w, int sim_begin,
                                                           int sim_end) {
  mlp_search_body<GUMBEL, AS, TBL, false>(s, g, w, sim_begin, sim_end);
}
template <bool GUMBEL, int AS = 0, bool TBL = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void mz_mlp_search_kernel_occ4(
    const StepArgs s, const JumpArgs g, const MlpGen w, int sim_begin, int sim_end) {
  mlp_search_body<GUMBEL, AS, TBL, true>(s, g, w, sim_begin, sim_end);
}

}  // namespace mz
