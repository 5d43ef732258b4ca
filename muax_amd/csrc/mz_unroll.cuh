// mz_unroll.cuh -- the forward unroll of the default MLP trio for the priority write-back of the device replay
// (DESIGN.md 4.7): for every sampled window j and every step i < kp
//
//     s_0 = Representation(obs[j]),   s_{i+1} = next state of Dynamic(s_i, a[j][i])        (muax/nn.py:59-115)
//     v_i = support_to_scalar(softmax(value head(s_i))),   prio[j][i] = |v_i - Rn[j][i]|
//
// in ONE launch, one wavefront per window.  Only what a value needs is evaluated: the value head of the prediction net
// (not the policy head) and the next-state branch of the dynamics net (not the reward head).  Everything is built from the
// run-time-shape blocks and stages of mz_mlp_blocks.cuh, so the arithmetic is the project's one spec ("MZ-F32") for any widths:
// v_i has the bits of the oracle's root_inference / recurrent_inference chain, and of act()'s root value for i = 0.
// No atomics, nothing that depends on the launch geometry: the same bits on every run.
// Below it, mz_stoch_unroll_kernel: the same unroll of the default stochastic MLP family, through the afterstate dynamics
// and the chance dynamics on the encoder's code of every next observation.
#pragma once
#include "mz_mlp_blocks.cuh"

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

__global__ __launch_bounds__(64) void mz_mlp_unroll_kernel(const UnrollArgs p) {
  extern __shared__ float unroll_f[];
  const MlpGen& w = p.w;
  const int r = blockIdx.x, tid = threadIdx.x;
  if (r >= p.B) return;
  const int E = w.E, A = w.A;
  const GenLds G = gen_lds(unroll_f, gen_obs_width(E, w.obs_dim), A);
  gen_embed(w.repr_w, w.repr_b, p.obs + (size_t)r * w.obs_dim, w.obs_dim, E, G, tid);
  const Mlp2 pv = w.pv(), pp = w.pp(), dr = w.dr(), dn = w.dn();  // (pp, dr: passed with their flags false, never read)
  for (int i = 0; i < p.kp; ++i) {
    const float v = gen_prediction(pv, pp, false, 0, E, w.F, w.support, G, G.ns, tid);
    if (tid == 0) {
      const size_t o = (size_t)r * p.kp + i;
      if (p.values) p.values[o] = v;
      // |v - Rn| on the bits: a NaN or infinite return stays one, whatever the unit's NaN flags let the compiler assume
      if (p.prio) p.prio[o] = u2f(f2u(v - p.Rn[(size_t)r * p.L + i]) & 0x7fffffffu);
    }
    if (i + 1 == p.kp) break;
    // Dynamic's next-state branch on [s, onehot(a)]; the one-hot by comparison: an action outside 0..A-1 is all zeros
    gen_stage_input(G, G.ns, E, A, p.act[(size_t)r * p.L + i], tid);
    gen_next_state(dn, dr, false, E + A, E, w.F, G, tid);
  }
}

// ---- the same unroll of the default stochastic MLP family (muax_amd/nn.py): between two values lie the
// afterstate dynamics on the action and the chance dynamics on the code the encoder gives the NEXT observation,
//
//     after_i = AfterstateDynamic(s_i, a[j][i]),   c_{i+1} = argmax encoder(obs[j][i+1]),   s_{i+1} = next state of
//     Dynamic(after_i, c_{i+1}),
//
// the code by the training kernel's rule (mz_stoch_train.cuh: the lowest index among equal maxima) and as an exact one-hot.
// The afterstate value, the chance logits, the policy head and the reward head are not evaluated. ----
struct StochUnrollArgs {
  const float *repr_w, *repr_b;
  Mlp2 ad, cn, pv, en;
  int obs_dim, E, A, C, F, support;
  int B, L, kp;      // windows; row stride of obs rows / act / Rn; steps evaluated (kp <= L)
  const float* obs;  // [B, L, obs_dim]
  const int* act;    // [B, L]
  const float* Rn;   // [B, L]
  float* values;     // [B, kp] or null
  float* prio;       // [B, kp] or null
  int* codes;        // [B, kp] or null: -1 at step 0, c_i behind it
};

// the chance code of one observation row: ChanceEncoder's Linear(16)-elu-Linear on the raw row (-> G.sa; no
// normalisation), the C <= 63 logits -> G.pl, one per lane, and the first lane that holds their maximum (no maximum
// among them, all NaN: 0, as argmax_first).  A stage like those of mz_mlp_blocks.cuh: it ends behind a barrier
MZ_DEV int stoch_unroll_code(const Mlp2& en, const float* obs_row, int obs_dim, int C, const GenLds& G, int tid) {
  for (int i = tid; i < obs_dim; i += 64) G.sa[i] = obs_row[i];
  __syncthreads();
  if (tid < kHidden) G.hid[tid] = elu(gen_linear(G.sa, obs_dim, en.w1, en.b1, kHidden, tid));
  __syncthreads();
  if (tid < C) G.pl[tid] = gen_linear(G.hid, kHidden, en.w2, en.b2, C, tid);
  __syncthreads();
  const float x = (tid < C) ? G.pl[tid] : -INFINITY;
  float m = x;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
  const unsigned long long at = __builtin_amdgcn_ballot_w64(x == m);
  __syncthreads();
  return at ? __builtin_ctzll(at) : 0;
}

__global__ __launch_bounds__(64) void mz_stoch_unroll_kernel(const StochUnrollArgs p) {
  extern __shared__ float stoch_unroll_f[];
  const int r = blockIdx.x, tid = threadIdx.x;
  if (r >= p.B) return;
  const int E = p.E, A = p.A, C = p.C;
  // the scratch holds the observation row, then [s | onehot(a, A)], then [after | onehot(c, C)] in G.sa
  const GenLds G = gen_lds(stoch_unroll_f, gen_obs_width(E, p.obs_dim), A > C ? A : C);
  const float* obs = p.obs + (size_t)r * p.L * p.obs_dim;
  gen_embed(p.repr_w, p.repr_b, obs, p.obs_dim, E, G, tid);
  int code = -1;  // (step 0 has no transition)
  for (int i = 0; i < p.kp; ++i) {
    const float v = gen_prediction(p.pv, p.pv, false, 0, E, p.F, p.support, G, G.ns, tid);  // (no policy head)
    if (tid == 0) {
      const size_t o = (size_t)r * p.kp + i;
      if (p.values) p.values[o] = v;
      if (p.prio) p.prio[o] = u2f(f2u(v - p.Rn[(size_t)r * p.L + i]) & 0x7fffffffu);  // (on the bits, as above)
      if (p.codes) p.codes[o] = code;
    }
    if (i + 1 == p.kp) break;
    // the heads passed in the reward head's place are never read (flag false)
    gen_stage_input(G, G.ns, E, A, p.act[(size_t)r * p.L + i], tid);
    gen_next_state(p.ad, p.ad, false, E + A, E, p.F, G, tid);
    code = stoch_unroll_code(p.en, obs + (size_t)(i + 1) * p.obs_dim, p.obs_dim, C, G, tid);
    gen_stage_input(G, G.ns, E, C, code, tid);
    gen_next_state(p.cn, p.cn, false, E + C, E, p.F, G, tid);
  }
}

}  // namespace mz
