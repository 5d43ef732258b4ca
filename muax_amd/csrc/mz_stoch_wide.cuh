// mz_stoch_wide.cuh -- the WHOLE stochastic search of the default stochastic MLP family (mctx stochastic_muzero_policy,
// DESIGN.md 4.7) in ONE launch, the root's tree in LDS: the root set-up of mzs_root_stochastic, every simulation (select
// -> decision or chance function -> expand -> backward), the summary and the sampling of mzs_finish_stochastic.  Root
// inference is the caller's (the kernel takes the RootFnOutput arrays) or, in the ROOT instantiations, the kernel's own:
// the representation (mz_wave_tree.cuh wave_root_state, its weights read from HBM once per root) and the prediction heads
// on the observation row, as mz_wide.cuh does it; mz_stoch_root_kernel is that root inference alone, for the
// three-launch route.  The root's Dirichlet noise is an input array or, in the DRAW instantiations, drawn by the root's own
// wavefront in front of its search (mz_dirichlet.cuh wave_dirichlet_row: the bits of mzs_dirichlet).  The mapping, the tree record and the rules
// both one-launch kernels follow (pUCT score, tie-break noise, expansion, backup, summary and sampling, tree export) are
// mz_wave_tree.cuh's:
//
//   * one root per WAVEFRONT, lane i owns slot i of a node (A actions, then C chance outcomes, A + C <= 64); records lie
//     [field][slot] in LDS, the path too, the node embeddings when that costs no resident root (else HBM scratch);
//   * the seven heads' weights sit in the workgroup's LDS, loaded once and shared by its 1..4 wavefronts (roots);
//   * per simulation only the function of the selected edge's parent kind is evaluated, as mz_stoch_mlp.cuh does: sixteen
//     lanes per hidden layer, two hidden layers side by side, one lane per output.
//
// Rules, bit for bit those of the step-wise stochastic kernels (include/mzsearch.h "step-wise path, stochastic policy";
// mz_step.cuh level_decide / chance_decide, mz_step_kernels.cuh step_root_stochastic_kernel /
// step_expand_backup_stochastic_kernel / finish_row, mz_stoch_mlp.cuh): decision nodes at even depth take the MuZero
// pUCT rule over all A + C slots (qtransform_by_parent_and_siblings, tie-break uniforms of length A + C in mode 1), chance
// nodes at odd depth score p_i / (visits_i + 1), first maximum; the key chain advances one split per level; max_depth
// and re-expansion count both kinds of level.  The edge from a decision parent has reward 0 and discount 1, the edge
// from a chance parent the chance function's reward and the bound discount: the parity of the depth decides, no
// per-edge discount is stored.
//
// Arithmetic: MZ-F32 as in mz_wide.cuh.  The same liberty: of the links of a one-hot input (the action of the decision
// function, the outcome of the chance function) only the one whose input is 1 is evaluated -- fma(0, w, acc) == acc for
// finite w unless acc is -0, and an accumulator that starts at +0 and adds products of non-negative inputs is not -0.
// The condition holds for both functions: the state embedding (the caller's root inference and the chance function's
// output) and the afterstate embedding are min-max normalised, hence non-negative.  It holds for the ROOT instantiations
// as well: the root state they compute leaves wave_min_max_normalize, (s - min) / scale with scale > 0.
//
// No atomics, nothing that depends on the launch geometry: a root's bits are the same whichever wavefront of whichever
// workgroup ran it.
#pragma once
#define MZ_DIRICHLET_NO_KERNEL  // (dirichlet_kernel is mz_selftest.hip's; this unit takes wave_dirichlet_row)
#include "mz_dirichlet.cuh"
#include "mz_stoch_wide_launch.h"
#include "mz_wide.cuh"

#pragma clang fp contract(off)

namespace mz {

struct StochWideShape {
  int rec_words, root_words, wg_words, weight_words, emb_lds, waves;
};

// Prediction (muax/nn.py:73-90) on the state whose element k is in lane k of `s`, as the chance function evaluates it:
// the two hidden layers side by side (`grp`: 0 value, 1 policy; `u`: this lane's hidden unit), action logit a in lane a
// (al = min(lane, A - 1)), the decoded value in every lane.  pv, pp: the heads in LDS or in HBM
MZ_DEV void stoch_prediction(float s, const Mlp2& pv, const Mlp2& pp, int E, int F, int A, int support, int lane, float& logit,
                             float& value) {
  const int u = lane & 15, grp = (lane >> 4) & 1;
  const int fc = lane < F ? lane : 0, al = lane < A ? lane : 0;
  const float h = elu(wide_chain(s, E, (grp ? pp.w1 : pv.w1) + u) + (grp ? pp.b1 : pv.b1)[u]);
  const float vl = wide_out<0>(h, pv.w2, pv.b2, F, fc);
  logit = wide_out<16>(h, pp.w2, pp.b2, A, al);
  value = wave_decode(vl, F, support, lane);
}

// Root inference of the family on its own (mzs_mlp_stochastic_root): RootFnOutput for B observations, one root per
// wavefront, the representation by wave_root_state, the prediction heads read from HBM.  No LDS, no barrier
__global__ __launch_bounds__(64 * kWideMaxWaves) void mz_stoch_root_kernel(const StochRootParams p) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * kWideMaxWaves + (threadIdx.x >> 6);
  if (r >= p.B) return;  // (wavefront-uniform)
  const float s = wave_root_state(p.obs + (size_t)r * p.obs_dim, p.repr_w, p.repr_b, p.obs_dim, p.E, lane);
  float logit, value;
  stoch_prediction(s, p.pv, p.pp, p.E, p.F, p.A, p.support, lane, logit, value);
  if (lane < p.E) p.embedding[(size_t)r * p.E + lane] = s;
  if (lane < p.A) p.prior_logits[(size_t)r * p.A + lane] = logit;
  if (lane == 0) p.value[r] = value;
}

// MODE 0 / 1: without / with mctx's tie-break noise at the decision nodes (the handle's `tiebreak`); ROOT: root
// inference inside the launch -- the kernel reads p.obs and the representation's weights (HBM, once per root) instead of
// the RootFnOutput arrays and writes p.root_value_out; DRAW: the root's Dirichlet row drawn inside the launch
// (mz_dirichlet.cuh wave_dirichlet_row on the call's Dirichlet key, the bits of mzs_dirichlet) instead of read from
// p.dirichlet_noise, and written to p.noise_out when that is set
template <int MODE, bool ROOT = false, bool DRAW = false>
__global__ __launch_bounds__(64 * kWideMaxWaves) void mz_stoch_wide_kernel(const StochWideParams p, const StochWideShape sh) {
  static_assert(MODE == 0 || MODE == 1, "tie-break setting");
  constexpr bool TIEBREAK = MODE == 1;
  extern __shared__ int stoch_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int A = p.A, C = p.C, AC = A + C, E = p.E, F = p.F, H = kHidden;
  const int S = p.S, N = S + 1, REC = sh.rec_words;

  // ---- workgroup prologue: the seven heads and the pUCT table into LDS ----
  float* wl = reinterpret_cast<float*>(stoch_lds);
  int off = 0;
  auto stage = [&](const float* src, int cnt) {
    float* d = wl + off;
    for (int k = tid; k < cnt; k += blockDim.x) d[k] = src[k];
    off += cnt;
    return static_cast<const float*>(d);
  };
  auto head = [&](int i, int n_in, int n_out) {
    Mlp2 h;
    h.w1 = stage(p.w[4 * i], n_in * H);
    h.b1 = stage(p.w[4 * i + 1], H);
    h.w2 = stage(p.w[4 * i + 2], H * n_out);
    h.b2 = stage(p.w[4 * i + 3], n_out);
    return h;
  };
  const Mlp2 ad = head(0, E + A, E), av = head(1, E, F), ac = head(2, E, C), cr = head(3, E + C, F),
                  cn = head(4, E + C, E), pv = head(5, E, F), pp = head(6, E, A);
  float* tbl = wl + sh.weight_words;
  wave_stage_puct_table(tbl, S, p.pb_c_init, p.pb_c_base);
  __syncthreads();

  const int r = blockIdx.x * sh.waves + wave;
  if (r >= p.B) return;  // (after the only workgroup barrier; from here on a wavefront is on its own)
  const uint64_t rg = p.root_offset + (uint64_t)r;
  const int max_depth = p.max_depth > 0 ? p.max_depth : S;
  const bool ex = p.export_tree != 0;
  const bool ok = lane < AC, act = lane < A;
  const int sl = ok ? lane : 0, al = act ? lane : 0;  // this lane's slot / action, clamped for addressing
  const int ec = lane < E ? lane : 0, fc = lane < F ? lane : 0;
  const int u = lane & 15, grp = (lane >> 4) & 1;  // hidden unit and which of the two side-by-side heads
  const float disc = p.discount;
  // what a captured launch must not freeze comes from the device block when there is one
  const float temperature = p.dyn ? __uint_as_float(p.dyn[2]) : p.temperature;
  const float fraction = p.dyn ? __uint_as_float(p.dyn[3]) : p.dirichlet_fraction;

  // ---- this root's block (mz_wave_tree.cuh; a chance node's record says so in its parent word) ----
  int* tree = stoch_lds + sh.wg_words + wave * sh.root_words;
  int* path = wave_tree_setup(tree, sh.root_words, N, REC, lane);
  float* emb = sh.emb_lds ? reinterpret_cast<float*>(path + N) : (ex ? p.t_embeddings : p.emb_scratch) + (size_t)r * N * E;
  const size_t tn0 = (size_t)r * N;  // this root's first node in the export arrays
  const bool inv = (p.invalid != nullptr && act) ? p.invalid[(size_t)r * A + al] != 0 : false;
  const bool root_masked = !act || inv;  // the root's mask over all slots: the chance slots and the invalid actions
  wave_sync();

  // ---- the root (mz_step_kernels.cuh root_row with AD = A): Dirichlet mix, log, mask over the actions, -inf on the
  // chance slots, the softmax over all slots ----
  {
    [[maybe_unused]] float drawn = 0.0f;
    if constexpr (DRAW) {
      // the root's row of the global batch's draw, first: one float is all that stays live across root inference.  Key
      // and alpha behind the simulation keys of the device block when there is one
      const int tail = kStochBlockHead + 2 * S;
      const uint32_t kd0 = p.dyn ? p.dyn[tail] : p.k_dirichlet[0], kd1 = p.dyn ? p.dyn[tail + 1] : p.k_dirichlet[1];
      const float alpha = p.dyn ? __uint_as_float(p.dyn[tail + 2]) : p.dirichlet_alpha;
      drawn = wave_dirichlet_row(kd0, kd1, alpha, A, p.global_batch, rg, lane);
      if (p.noise_out != nullptr && act) p.noise_out[(size_t)r * A + al] = drawn;
    }
    float x;
    [[maybe_unused]] float root_v = 0.0f;
    if constexpr (ROOT) {
      // root inference (MuZero._root_inference_eager on the default modules): node 0's state, its logits and value
      const float s = wave_root_state(p.obs + (size_t)r * p.obs_dim, p.repr_w, p.repr_b, p.obs_dim, E, lane);
      if (lane < E) emb[lane] = s;
      stoch_prediction(s, pv, pp, E, F, A, p.support, lane, x, root_v);
    } else {
      x = act ? p.prior_logits[(size_t)r * A + al] : 0.0f;
    }
    const float pr = wave_softmax(x, A, lane);
    float nz;
    if constexpr (DRAW) nz = drawn;
    else nz = (p.dirichlet_noise != nullptr && act) ? p.dirichlet_noise[(size_t)r * A + al] : 0.0f;
    const float noisy = (1.0f - fraction) * pr + fraction * nz;
    float lg = log_pos(fmaxf(noisy, kFltTiny));
    if (p.invalid != nullptr) {
      const float top = wave_max(act ? lg : -INFINITY);
      lg = inv ? kFltLowest : lg - top;
    }
    lg = act ? lg : -INFINITY;
    const float prob = wave_softmax(lg, AC, lane);
    if constexpr (!ROOT)
      if (lane < E) emb[lane] = p.embedding[(size_t)r * E + ec];
    if (ok) {
      tree[rec_child(kChildProb, AC, sl)] = __float_as_int(prob);
      if (ex) p.t_children_prior_logits[tn0 * AC + sl] = lg;
    }
    if (lane == 0) {
      float v;
      if constexpr (ROOT) p.root_value_out[r] = v = root_v;
      else v = p.value[r];
      tree[kRecVisits] = 1;
      tree[kRecValue] = __float_as_int(v);
      tree[kRecRaw] = __float_as_int(v);
    }
    wave_sync();
  }

  // ---- simulations ----
  int depth_sum = 0;
  for (int sim = 0; sim < S; ++sim) {
    [[maybe_unused]] uint32_t kk0 = 0, kk1 = 0;  // the tie-break key walk (wave_noisy_argmax)
    [[maybe_unused]] int klevel = -1;
    int node = 0, depth = 0, parent = 0, action = 0, next = -1;
    for (;;) {
      const int* rec = tree + node * REC;
      const int link = rec[rec_child(kChildLink, AC, sl)];
      const float prob = __int_as_float(rec[rec_child(kChildProb, AC, sl)]);
      const int cvis = link_visits(link), cidx = link_child(link);
      int best;
      if (depth & 1) {
        // chance node (mz_step.cuh chance_decide): no noise, first maximum
        best = wave_first_max(ok ? prob / (float)(cvis + 1) : -INFINITY);
      } else {
        // decision node (level_decide): every edge has reward 0 and discount 1
        const int nvis = rec[kRecVisits];
        const float nval = __int_as_float(rec[kRecValue]);
        const float q = __int_as_float(rec[rec_child(kChildReward, AC, sl)]) + 1.0f * __int_as_float(rec[rec_child(kChildValue, AC, sl)]);
        float sc = wave_puct_score(ok && cvis > 0, q, nval, tbl[nvis], prob, cvis);
        if (!ok || (depth == 0 && root_masked)) sc = -INFINITY;
        best = wave_noisy_argmax<TIEBREAK>(sc, ok, sl, AC, depth, lane, p.global_batch, rg, [&](int i) {
          return p.dyn ? p.dyn[kStochBlockHead + 2 * sim + i] : p.sim_keys[sim][i];
        }, kk0, kk1, klevel);
      }
      if (lane == 0) path[depth] = path_word(node, best);
      parent = node;
      action = best;
      next = w_rdl_i(cidx, best);
      depth += 1;
      if (next == -1 || depth >= max_depth) break;
      node = next;
    }
    depth_sum += depth;
    const int newn = next == -1 ? sim + 1 : next;

    // the function of the parent's kind (mz_stoch_mlp.cuh).  Decision parent (at even depth - 1): afterstate dynamics at
    // action clamp(slot, 0, A - 1), then afterstate value | chance logits; chance parent: reward | next state at outcome
    // clamp(slot - A, 0, C - 1), then value | action logits
    const bool decision = (depth & 1) != 0;
    const int W = decision ? A : C;
    int hot = decision ? action : action - A;
    hot = hot < 0 ? 0 : (hot > W - 1 ? W - 1 : hot);
    const float s_par = lane < E ? emb[parent * E + ec] : 0.0f;
    float reward = 0.0f, value, logit;
    {
      const Mlp2 d1 = decision ? ad : cn;  // the next embedding's head; the rows of lanes without a head repeat it
      const float* w1 = ((grp || decision) ? d1.w1 : cr.w1) + u;
      float a1 = wide_chain(s_par, E, w1);
      a1 = __builtin_fmaf(1.0f, w1[(E + hot) * H], a1);  // (the one-hot's other links add nothing: see the header)
      const float h = elu(a1 + ((grp || decision) ? d1.b1 : cr.b1)[u]);
      const float ns = wave_min_max_normalize(wide_out<16>(h, d1.w2, d1.b2, E, ec), E, lane);
      if (lane < E) emb[newn * E + ec] = ns;
      if (!decision) reward = wave_decode(wide_out<0>(h, cr.w2, cr.b2, F, fc), F, p.support, lane);
      const Mlp2 hv = decision ? av : pv, hp = decision ? ac : pp;
      const int n_pol = decision ? C : A, pj = decision ? lane - A : lane;
      const int pjc = pj < 0 ? 0 : (pj > n_pol - 1 ? n_pol - 1 : pj);
      const float h2 = elu(wide_chain(ns, E, (grp ? hp.w1 : hv.w1) + u) + (grp ? hp.b1 : hv.b1)[u]);
      const float vl = wide_out<0>(h2, hv.w2, hv.b2, F, fc);
      const float pl = wide_out<16>(h2, hp.w2, hp.b2, n_pol, pjc);
      value = wave_decode(vl, F, p.support, lane);
      logit = (pj >= 0 && pj < n_pol) ? pl : -INFINITY;  // the prior row: -inf on the slots of the other kind
    }
    const float prob = wave_softmax(logit, AC, lane);

    // expand (step_expand_backup_stochastic_kernel; the reward is 0 from a decision parent) and backward
    if (ex && ok) p.t_children_prior_logits[(tn0 + newn) * AC + sl] = logit;
    wave_tree_expand<false>(tree, REC, AC, newn, parent, action, decision, ok, sl, lane, prob, logit, value, reward);
    wave_tree_backward<true>(tree, path, REC, AC, depth, value, disc, lane);
  }

  // ---- finish_row over the A actions ----
  {
    float pw;
    const int best = wave_summary_sample(tree, AC, A, act, al, lane, temperature, p.gumbel ? p.gumbel + (size_t)r * A : nullptr,
                                         p.global_batch, rg, [&](int i) { return p.dyn ? p.dyn[i] : p.k_sample[i]; }, pw);
    if (act) p.action_weights[(size_t)r * A + al] = pw;
    if (lane == 0) {
      p.action[r] = best;
      if (p.search_value) p.search_value[r] = __int_as_float(tree[kRecValue]);
      if (p.depth_sum) p.depth_sum[r] = depth_sum;
    }
  }

  // ---- the finished tree into the handle's HBM arrays, as the step-wise kernels leave them ----
  if (ex) wave_tree_export<true>(p, tree, emb, sh.emb_lds, r, N, REC, AC, E, ok, sl, lane, disc, root_masked, depth_sum);
}

}  // namespace mz
