// mz_unroll.cuh -- the forward unroll of the default MLP trio for the priority write-back of the device replay
// (DESIGN.md 4.7): for every sampled window j and every step i < kp
//
//     s_0 = Representation(obs[j]),   s_{i+1} = next state of Dynamic(s_i, a[j][i])        (muax/nn.py:59-115)
//     v_i = support_to_scalar(softmax(value head(s_i))),   prio[j][i] = |v_i - Rn[j][i]|
//
// in ONE launch, one wavefront per window.  Only what a value needs is evaluated: the value head of the prediction net
// (not the policy head) and the next-state branch of the dynamics net (not the reward head).  Everything is built from the
// run-time-shape blocks of mz_mlp_generic.cuh, so the arithmetic is the project's one spec ("MZ-F32") for any widths:
// v_i has the bits of the oracle's root_inference / recurrent_inference chain, and of act()'s root value for i = 0.
// No atomics, nothing that depends on the launch geometry: the same bits on every run.
#pragma once
// mz_mlp_generic.cuh defines the root kernel of the generic act() route, which mz_stepwise.hip emits; this unit takes the
// header's device functions only, so its copy of that kernel gets a name of its own (never launched)
#define mz_mlp_root_kernel mz_unroll_unused_root_kernel
#include "mz_mlp_generic.cuh"
#undef mz_mlp_root_kernel

#pragma clang fp contract(off)

namespace mz {

struct UnrollArgs {
  MlpGen w;
  int B, L, kp;      // windows; row stride of act / Rn; steps evaluated (kp <= L)
  const float* obs;  // [B, obs_dim]
  const int* act;    // [B, L]
  const float* Rn;   // [B, L]
  float* values;     // [B, kp] or null
  float* prio;       // [B, kp] or null
};

// gen_prediction without the policy head: value logits of the embedding `s` (LDS) -> G.vl, the decoded value returned in
// lanes 0..15 (G.hid[0..16) and G.vl are free again after the last barrier)
MZ_DEV float gen_value(const MlpGen& w, const GenLds& G, const float* s, int tid) {
  if (tid < 16) G.hid[tid] = elu(gen_linear(s, w.E, w.pv_w1, w.pv_b1, kGenHidden, tid));
  __syncthreads();
  for (int j = tid; j < w.F; j += 64) G.vl[j] = gen_linear(G.hid, kGenHidden, w.pv_w2, w.pv_b2, w.F, j);
  __syncthreads();
  float v = 0.0f;
  if (tid < 16) v = gen_decode(G.vl, w.F, w.support, tid);
  __syncthreads();
  return v;
}

__global__ __launch_bounds__(64) void mz_mlp_unroll_kernel(const UnrollArgs p) {
  extern __shared__ float unroll_f[];
  const MlpGen& w = p.w;
  const int r = blockIdx.x, tid = threadIdx.x;
  if (r >= p.B) return;
  const int E = w.E, A = w.A;
  const GenLds G = gen_lds(unroll_f, E > w.obs_dim ? E : w.obs_dim, A);  // sa holds the observation first
  for (int i = tid; i < w.obs_dim; i += 64) G.sa[i] = p.obs[(size_t)r * w.obs_dim + i];
  __syncthreads();
  for (int e = tid; e < E; e += 64) G.ns[e] = gen_linear(G.sa, w.obs_dim, w.repr_w, w.repr_b, E, e);
  __syncthreads();
  gen_min_max_normalize(G.ns, E, tid);
  __syncthreads();
  for (int i = 0; i < p.kp; ++i) {
    const float v = gen_value(w, G, G.ns, tid);
    if (tid == 0) {
      const size_t o = (size_t)r * p.kp + i;
      if (p.values) p.values[o] = v;
      // |v - Rn| on the bits: a NaN or infinite return stays one, whatever the unit's NaN flags let the compiler assume
      if (p.prio) p.prio[o] = u2f(f2u(v - p.Rn[(size_t)r * p.L + i]) & 0x7fffffffu);
    }
    if (i + 1 == p.kp) break;
    // Dynamic's next-state branch on [s, onehot(a)]; the one-hot by comparison: an action outside 0..A-1 is all zeros
    const int action = p.act[(size_t)r * p.L + i];
    for (int k = tid; k < E; k += 64) G.sa[k] = G.ns[k];
    for (int k = tid; k < A; k += 64) G.sa[E + k] = (k == action) ? 1.0f : 0.0f;
    __syncthreads();
    if (tid < 16) G.hid[16 + tid] = elu(gen_linear(G.sa, E + A, w.dn_w1, w.dn_b1, kGenHidden, tid));
    __syncthreads();
    for (int e = tid; e < E; e += 64) G.ns[e] = gen_linear(G.hid + 16, kGenHidden, w.dn_w2, w.dn_b2, E, e);
    __syncthreads();
    gen_min_max_normalize(G.ns, E, tid);
    __syncthreads();
  }
}

}  // namespace mz
