// mz_mlp_blocks.cuh -- the default MLP nets (muax/nn.py:59-115; the stochastic family of muax_amd/nn.py) with RUN-TIME
// shapes, evaluated by one wavefront with the activations in LDS: the layer, the normalise and the decode, and on top of
// them every stage of a net pass stated once -- observation -> embedding, [s | one-hot], next state (+ reward logits),
// reward decode, prediction.  The kernels built from them: the generic route's root and one-launch search
// (mz_mlp_generic.cuh), the stochastic family's recurrent step (mz_stoch_mlp.cuh), the forward value unroll
// (mz_unroll.cuh).  Device and host-device functions only, no kernel.
//
// Arithmetic: the project's one spec ("MZ-F32") exactly as the oracle states it (oracle/mz_oracle.c:300-398):
// a linear layer is a k-ordered fma chain from 0 with the bias added last, ELU / exp / log / inv_scaling from mz_spec.cuh,
// every float sum 16 partials + xor butterfly (row_softmax_rt, row_sum) -- the same bits as the fused kernel and the
// oracle for any shape, which is what the tests check.
#pragma once
#include "mz_step.cuh"  // row_softmax_rt, kMaxAS

#pragma clang fp contract(off)

namespace mz {

// the trio's kernel argument block: the member names of mzs_mlp_weights (mzh::copy_weights), the heads as Mlp2 views
struct MlpGen {
  const float *repr_w, *repr_b;
  const float *pv_w1, *pv_b1, *pv_w2, *pv_b2, *pp_w1, *pp_b1, *pp_w2, *pp_b2;
  const float *dr_w1, *dr_b1, *dr_w2, *dr_b2, *dn_w1, *dn_b1, *dn_w2, *dn_b2;
  int obs_dim, E, A, F, support, pred_on_parent;
  float discount;
  MZ_DEV Mlp2 pv() const { return {pv_w1, pv_b1, pv_w2, pv_b2}; }
  MZ_DEV Mlp2 pp() const { return {pp_w1, pp_b1, pp_w2, pp_b2}; }
  MZ_DEV Mlp2 dr() const { return {dr_w1, dr_b1, dr_w2, dr_b2}; }
  MZ_DEV Mlp2 dn() const { return {dn_w1, dn_b1, dn_w2, dn_b2}; }
};

// haiku Linear, output j: dot (k-ordered fma chain from 0) then + bias; x in LDS (every lane reads the same word)
// U32: the weights indexed from the UNIFORM base with a 32-bit per-lane offset (global_load saddr + voffset) instead of
// through the per-lane pointer `w + j`.  That pointer is loop-invariant for the whole search and the compiler keeps one
// register pair per weight array alive across every simulation -- ~40 of the search kernel's VGPRs; the 32-bit form
// costs an address add per load (1 - 3 % at equal occupancy) and is what lets the four-wavefront build of the search
// kernel (mz_mlp_search_kernel_occ4) get by with two dozen spilled loop invariants instead of 66 registers
template <bool U32 = false>
MZ_DEV float gen_linear(const float* x, int n_in, const float* __restrict__ w, const float* __restrict__ b, int n_out, int j) {
  // the weights of eight links are requested before the first of their fmas issues (one link at a time is one L1 / L2
  // round trip per link: ~0.5 us each on a lone chain); the chain itself stays k-ordered
  float acc = 0.0f;
  const float* wj = w + j;
  auto wt = [&](int i) { return U32 ? w[(unsigned)(i * n_out + j)] : wj[(size_t)i * n_out]; };
  int i = 0;
  for (; i + 8 <= n_in; i += 8) {
    float wv[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) wv[k] = wt(i + k);
#pragma unroll
    for (int k = 0; k < 8; ++k) acc = __builtin_fmaf(x[i + k], wv[k], acc);
  }
  for (; i < n_in; ++i) acc = __builtin_fmaf(x[i], wt(i), acc);
  return acc + b[j];
}
// muax/nn.py:37-44 over a vector of n floats in LDS, by one wavefront (min / max do not depend on the order)
MZ_DEV void gen_min_max_normalize(float* v, int n, int tid) {
  float mn = INFINITY, mx = -INFINITY;
  for (int i = tid; i < n; i += 64) {
    mn = fminf(mn, v[i]);
    mx = fmaxf(mx, v[i]);
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, d));
    mx = fmaxf(mx, __shfl_xor(mx, d));
  }
  float scale = mx - mn;
  scale = scale < 1e-5f ? scale + 1e-5f : scale;
  __syncthreads();
  for (int i = tid; i < n; i += 64) v[i] = (v[i] - mn) / scale;
}
// support_to_scalar(softmax(logits[0..F))) (muax/utils.py:70-102) by the 16 lanes of one row; F in (16, 64]
MZ_DEV float gen_decode(const float* logits, int F, int support, int j) {
  float x[kMaxAS], p[kMaxAS];
#pragma unroll
  for (int t = 0; t < kMaxAS; ++t) x[t] = (j + 16 * t < F) ? logits[j + 16 * t] : 0.0f;
  row_softmax_rt(x, F, j, p);
  float part = 0.0f;
#pragma unroll
  for (int t = 0; t < kMaxAS; ++t) {
    const float term = (float)(j + 16 * t - support) * p[t];
    part = (t == 0) ? term : ((j + 16 * t < F) ? part + term : part);
  }
  return inv_scaling(row_sum(part));
}
// LDS scratch of the trio (floats): sa [E + A] | hid [32] | rl [64] | vl [64] | pl [64] | ns [E] | scal [4]
inline __host__ __device__ int gen_scratch_words(int E, int A) { return ((E + A + 3) / 4) * 4 + 32 + 3 * 64 + ((E + 3) / 4) * 4 + 4; }
// the `E` of that scratch for a kernel that starts from the observation: sa holds it before it holds [s | one-hot]
inline __host__ __device__ int gen_obs_width(int E, int obs_dim) { return E > obs_dim ? E : obs_dim; }
struct GenLds {
  float *sa, *hid, *rl, *vl, *pl, *ns, *scal;
};
MZ_DEV GenLds gen_lds(float* f, int E, int A) {
  GenLds G;
  G.sa = f; G.hid = G.sa + ((E + A + 3) / 4) * 4; G.rl = G.hid + 32; G.vl = G.rl + 64; G.pl = G.vl + 64;
  G.ns = G.pl + 64; G.scal = G.ns + ((E + 3) / 4) * 4;
  return G;
}

// ---- the stages of a net pass; each ends behind a barrier.  An optional head is a head and a flag (a pointer that may be
// null cost the stochastic kernel 256 bytes of scratch): with the flag false the head is never read, pass any ----
// Representation: the observation row -> G.sa -> the min-max normalised embedding in G.ns
MZ_DEV void gen_embed(const float* repr_w, const float* repr_b, const float* obs_row, int obs_dim, int E, const GenLds& G, int tid) {
  for (int i = tid; i < obs_dim; i += 64) G.sa[i] = obs_row[i];
  __syncthreads();
  for (int e = tid; e < E; e += 64) G.ns[e] = gen_linear(G.sa, obs_dim, repr_w, repr_b, E, e);
  __syncthreads();
  gen_min_max_normalize(G.ns, E, tid);
  __syncthreads();
}
// [s | onehot(hot, width)] -> G.sa; the one-hot by comparison: a `hot` outside 0..width-1 is all zeros
MZ_DEV void gen_stage_input(const GenLds& G, const float* s, int E, int width, int hot, int tid) {
  for (int i = tid; i < E; i += 64) G.sa[i] = s[i];
  for (int k = tid; k < width; k += 64) G.sa[E + k] = (k == hot) ? 1.0f : 0.0f;
  __syncthreads();
}
// Dynamic on the n_in inputs in G.sa: hidden rows 0 (the reward head `dr`, only with `reward`) and 1 (the next-state
// head `dn`), reward logits -> G.rl, the min-max normalised next state -> G.ns
template <bool U32 = false>
MZ_DEV void gen_next_state(const Mlp2& dn, const Mlp2& dr, bool reward, int n_in, int E, int F, const GenLds& G, int tid) {
  if (tid < 32 && (reward || tid >= 16)) {
    const int u = tid & 15;
    const float a = (tid < 16) ? gen_linear<U32>(G.sa, n_in, dr.w1, dr.b1, kHidden, u)
                               : gen_linear<U32>(G.sa, n_in, dn.w1, dn.b1, kHidden, u);
    G.hid[tid] = elu(a);
  }
  __syncthreads();
  if (reward)
    for (int j = tid; j < F; j += 64) G.rl[j] = gen_linear<U32>(G.hid, kHidden, dr.w2, dr.b2, F, j);
  for (int e = tid; e < E; e += 64) G.ns[e] = gen_linear<U32>(G.hid + 16, kHidden, dn.w2, dn.b2, E, e);
  __syncthreads();
  gen_min_max_normalize(G.ns, E, tid);
  __syncthreads();
}
// the reward decode of G.rl on the last row, -> G.scal[0], while rows 0 / 1 start the prediction net (no barrier here)
MZ_DEV void gen_reward_decode(const GenLds& G, int F, int support, int tid) {
  if (tid >= 48) {
    const float rw = gen_decode(G.rl, F, support, tid & 15);
    if (tid == 48) G.scal[0] = rw;
  }
}
// Prediction on the embedding `s` (LDS): value logits -> G.vl, the n_policy logits of `pp` (only with `policy`) -> G.pl,
// the decoded value -> G.scal[1] and returned in lanes 0..15
template <bool U32 = false>
MZ_DEV float gen_prediction(const Mlp2& pv, const Mlp2& pp, bool policy, int n_policy, int E, int F, int support, const GenLds& G,
                            const float* s, int tid) {
  if (tid < 32 && (policy || tid < 16)) {
    const int u = tid & 15;
    const float a = (tid < 16) ? gen_linear<U32>(s, E, pv.w1, pv.b1, kHidden, u) : gen_linear<U32>(s, E, pp.w1, pp.b1, kHidden, u);
    G.hid[tid] = elu(a);
  }
  __syncthreads();
  for (int j = tid; j < F; j += 64) G.vl[j] = gen_linear<U32>(G.hid, kHidden, pv.w2, pv.b2, F, j);
  if (policy)
    for (int j = tid; j < n_policy; j += 64) G.pl[j] = gen_linear<U32>(G.hid + 16, kHidden, pp.w2, pp.b2, n_policy, j);
  __syncthreads();
  float v = 0.0f;
  if (tid < 16) {
    v = gen_decode(G.vl, F, support, tid);
    if (tid == 0) G.scal[1] = v;
  }
  __syncthreads();
  return v;
}

}  // namespace mz
