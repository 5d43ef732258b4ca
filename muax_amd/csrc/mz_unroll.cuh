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

}  // namespace mz
