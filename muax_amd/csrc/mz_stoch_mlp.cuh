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
// the run-time-shape blocks and stages of mz_mlp_blocks.cuh, so the arithmetic is the project's one spec ("MZ-F32") for any widths:
// each function has the bits of the oracle's recurrent_inference with that function's weights in the trio's places.
// No atomics, nothing that depends on the launch geometry: the same bits on every run.
#pragma once
#include "mz_mlp_blocks.cuh"

#pragma clang fp contract(off)

namespace mz {

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
  gen_stage_input(G, p.parent_embedding + (size_t)r * E, E, W, hot, tid);
  // rows 0 (the chance function's reward head) and 1 (the next embedding), then the Prediction of this kind
  gen_next_state(decision ? w.ad : w.cn, w.cr, !decision, E + W, E, F, G, tid);
  float* nrow = (decision ? p.afterstate_embedding : p.state_embedding) + (size_t)r * E;
  for (int e = tid; e < E; e += 64) nrow[e] = G.ns[e];
  if (!decision) gen_reward_decode(G, F, w.support, tid);
  if (decision) {
    gen_prediction(w.av, w.ac, true, C, E, F, w.support, G, G.ns, tid);
    for (int j = tid; j < C; j += 64) p.chance_logits[(size_t)r * C + j] = G.pl[j];
    if (tid == 0) p.afterstate_value[r] = G.scal[1];
  } else {
    gen_prediction(w.pv, w.pp, true, A, E, F, w.support, G, G.ns, tid);
    for (int j = tid; j < A; j += 64) p.action_logits[(size_t)r * A + j] = G.pl[j];
    if (tid == 0) {
      p.value[r] = G.scal[1];
      p.reward[r] = G.scal[0];
      p.discount[r] = w.discount;
    }
  }
}

}  // namespace mz
