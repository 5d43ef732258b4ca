// mz_stoch_mlp.cuh -- the decision and the chance function of the default stochastic MLP family (muax_amd/nn.py,
// create_stochastic_muzero_network) for the stochastic step-wise search: what sits between
// mzs_select_stochastic and mzs_expand_backup_stochastic, for every root in ONE launch, one wavefront per root.
//
//   decision parent (the selected edge leaves a decision node), a = clamp(slot, 0, A - 1):
//       as = min_max_normalize(mlp2([s, onehot(a, A)]))                       -> afterstate_embedding
//       afterstate value logits [F], chance logits [C] = Prediction(C, F)(as) -> afterstate_value (decoded), chance_logits
//   chance parent, c = clamp(slot - A, 0, C - 1):
//       reward logits [F], s' = Dynamic(E, C, F)(as, c)                       -> reward (decoded), state_embedding
//       value logits [F], action logits [A] = Prediction(A, F)(s')            -> value (decoded), action_logits; discount
//
// Per root ONLY the function of its parent's kind is evaluated and only that kind's output rows are written: the
// expansion kernel reads no other (mz_step_kernels.cuh, step_expand_backup_stochastic_kernel).  Everything is built from
// the run-time-shape blocks of mz_mlp_generic.cuh, so the arithmetic is the project's one spec ("MZ-F32") for any widths:
// each function has the bits of the oracle's recurrent_inference with that function's weights in the trio's places.
// No atomics, nothing that depends on the launch geometry: the same bits on every run.
#pragma once
#include "mz_mlp_generic.cuh"

#pragma clang fp contract(off)

namespace mz {

// one Linear(16)-elu-Linear stack, haiku layout
struct Mlp2 {
  const float *w1, *b1, *w2, *b2;
};
struct StochMlp {
  Mlp2 ad;          // afterstate dynamics [E+A,16] [16] [16,E] [E]
  Mlp2 av, ac;      // afterstate value    [E,16] .. [16,F] [F];  chance logits [E,16] .. [16,C] [C]
  Mlp2 cr, cn;      // chance reward       [E+C,16] .. [16,F] [F]; chance next state [E+C,16] .. [16,E] [E]
  Mlp2 pv, pp;      // prediction value    [E,16] .. [16,F] [F];  prediction policy [E,16] .. [16,A] [A]
  int E, A, C, F, support;
  float discount;
};
struct StochRecurrentArgs {
  int B;
  const int32_t *slot, *parent_is_decision;  // [B]
  const float* parent_embedding;             // [B, E]
  float *chance_logits, *afterstate_value, *afterstate_embedding;      // [B, C] [B] [B, E]
  float *action_logits, *value, *reward, *discount, *state_embedding;  // [B, A] [B] [B] [B] [B, E]
};
// LDS of one root (floats): gen_lds with the one-hot as wide as the wider of the two kinds
inline __host__ __device__ int stoch_scratch_words(int E, int A, int C) { return gen_scratch_words(E, A > C ? A : C); }

// the two heads of a Prediction on the embedding `s` (LDS) through gen_prediction: value logits -> G.vl, the `n` policy
// logits -> G.pl, the decoded value -> G.scal[1]
MZ_DEV void stoch_prediction(const StochMlp& w, const GenLds& G, const Mlp2& v, const Mlp2& p, int n, const float* s, int tid) {
  MlpGen g = {};
  g.pv_w1 = v.w1; g.pv_b1 = v.b1; g.pv_w2 = v.w2; g.pv_b2 = v.b2;
  g.pp_w1 = p.w1; g.pp_b1 = p.b1; g.pp_w2 = p.w2; g.pp_b2 = p.b2;
  g.E = w.E; g.A = n; g.F = w.F; g.support = w.support;
  gen_prediction(g, G, s, tid);
}

__global__ __launch_bounds__(64) void mz_stoch_mlp_recurrent_kernel(const StochMlp w, const StochRecurrentArgs p) {
  extern __shared__ float stoch_f[];
  const int r = blockIdx.x, tid = threadIdx.x;
  if (r >= p.B) return;
  const int E = w.E, A = w.A, C = w.C, F = w.F;
  const GenLds G = gen_lds(stoch_f, E, A > C ? A : C);
  const bool decision = p.parent_is_decision[r] != 0;
  const int slot = p.slot[r];
  // the clamps search_stochastic documents for caller-run functions; the one-hot by comparison
  const int W = decision ? A : C;
  int hot = decision ? slot : slot - A;
  hot = hot < 0 ? 0 : (hot > W - 1 ? W - 1 : hot);
  const float* prow = p.parent_embedding + (size_t)r * E;
  for (int i = tid; i < E; i += 64) G.sa[i] = prow[i];
  for (int k = tid; k < W; k += 64) G.sa[E + k] = (k == hot) ? 1.0f : 0.0f;
  __syncthreads();
  const Mlp2& dn = decision ? w.ad : w.cn;
  if (tid < 32) {  // hidden layers: rows 0 (the chance function's reward head) and 1 (the next embedding)
    const int u = tid & 15;
    if (tid >= 16) G.hid[tid] = elu(gen_linear(G.sa, E + W, dn.w1, dn.b1, kGenHidden, u));
    else if (!decision) G.hid[tid] = elu(gen_linear(G.sa, E + W, w.cr.w1, w.cr.b1, kGenHidden, u));
  }
  __syncthreads();
  if (!decision)
    for (int j = tid; j < F; j += 64) G.rl[j] = gen_linear(G.hid, kGenHidden, w.cr.w2, w.cr.b2, F, j);
  for (int e = tid; e < E; e += 64) G.ns[e] = gen_linear(G.hid + 16, kGenHidden, dn.w2, dn.b2, E, e);
  __syncthreads();
  gen_min_max_normalize(G.ns, E, tid);
  __syncthreads();
  float* nrow = (decision ? p.afterstate_embedding : p.state_embedding) + (size_t)r * E;
  for (int e = tid; e < E; e += 64) nrow[e] = G.ns[e];
  if (!decision && tid >= 48) {  // the reward decode on the last row while rows 0 / 1 start the prediction net
    const float rw = gen_decode(G.rl, F, w.support, tid & 15);
    if (tid == 48) G.scal[0] = rw;
  }
  if (decision) {
    stoch_prediction(w, G, w.av, w.ac, C, G.ns, tid);
    for (int j = tid; j < C; j += 64) p.chance_logits[(size_t)r * C + j] = G.pl[j];
    if (tid == 0) p.afterstate_value[r] = G.scal[1];
  } else {
    stoch_prediction(w, G, w.pv, w.pp, A, G.ns, tid);
    for (int j = tid; j < A; j += 64) p.action_logits[(size_t)r * A + j] = G.pl[j];
    if (tid == 0) {
      p.value[r] = G.scal[1];
      p.reward[r] = G.scal[0];
      p.discount[r] = w.discount;
    }
  }
}

}  // namespace mz
