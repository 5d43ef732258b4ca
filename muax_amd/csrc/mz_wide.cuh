// mz_wide.cuh -- act() of the default MLP trio (muax/nn.py:59-115) under either policy for 17..64 actions in ONE launch,
// the root's tree in LDS: root inference, every simulation, the summary and the sampling, like mz_fused.cuh, but mapped
// for wide action sets.  mz_fused.cuh keeps all scores of a node in one lane (A <= 16); here
//
//   * one root per WAVEFRONT, lane a owns action a (A <= 64): the mapping, the tree record and the rules of mctx that
//     mz_wave_tree.cuh states for this kernel and the stochastic one (pUCT score, tie-break noise, expansion, backup in
//     chunks of 64 levels, summary and sampling, tree export);
//   * selection walks level by level (no JUMP words, no cached decisions: a level is a few dozen instructions here);
//   * the nets: activations stay in registers, lane k holding element k, and a chain link takes its input with
//     v_readlane; the weights sit in the workgroup's LDS, loaded once and shared by its 1..4 wavefronts (roots).  Sixteen
//     lanes evaluate a hidden layer, two hidden layers (reward | next state, value | policy) side by side; an output
//     layer has one lane per output (F <= 63 support bins, E <= 64 state elements, A <= 64 prior logits).
//
// Shapes (A, E, F, S, obs_dim, max_depth, pred_on_parent) are run-time parameters: one kernel per mode of the fused
// dispatchers (0 / 1: MuZero policy without / with tie-break noise, 2 / 3: Gumbel MuZero with
// qtransform_by_parent_and_siblings / qtransform_completed_by_mix_value) serves A in 17..64, E <= 64, support_size 8..31
// and every S the LDS admits (mz_wide_launch.h, wide_plan).  The Gumbel modes share the nets, the expansion and the
// backup; their decisions (mctx gumbel_muzero_{root,interior}_action_selection, seq_halving) are lane-parallel as well:
// the completed Q of a level is computed by all lanes at once, the root Gumbel noise of action a lives in lane a's
// register for the whole act, and any max_num_considered_actions up to A is served (the top-k of sequential halving is
// the visit-count test of score_considered: nothing is sorted).
//
// Arithmetic: MZ-F32 as the oracle states it (oracle/mz_oracle.c): a linear layer is a k-ordered fma chain
// from 0 with the bias added last, ELU / exp / log / inv_scaling from mz_spec.cuh, every float sum over actions or
// support bins is 16 partials (element i in partial i & 15, slots ascending) + xor butterfly.  One liberty: the links of
// the Dynamic net's one-hot action input are not evaluated except the one whose input is 1 -- fma(0, w, acc) == acc for
// finite w unless acc is -0, and an accumulator that starts at +0 and adds products of non-negative inputs (a
// min-max-normalised state) is never -0 in round-to-nearest.
#pragma once
#include "mz_wave_tree.cuh"
#include "mz_wide_launch.h"

#pragma clang fp contract(off)

namespace mz {

struct WideShape {
  int A, E, F, rec_words, root_words, wg_words, weight_words, emb_lds, waves;
};

// the weight block in LDS, arrays in this order (haiku layout w[in][out])
struct WideNets {
  const float *pv_w1, *pv_b1, *pv_w2, *pv_b2, *pp_w1, *pp_b1, *pp_w2, *pp_b2;
  const float *dr_w1, *dr_b1, *dr_w2, *dr_b2, *dn_w1, *dn_b1, *dn_w2, *dn_b2;
};

// mctx qtransforms on the wide mapping (oracle/mz_oracle.c mzo_qtransform), this lane's child: QT 0
// qtransform_by_parent_and_siblings, QT 1 qtransform_completed_by_mix_value(value_scale 0.1, maxvisit_init 50).
// prob = softmax(prior logits) of the node; cvis = the child's visits (0 in lanes past A), sum_visits their sum (QT 1)
template <int QT>
MZ_DEV float wide_qtransform(bool ok, bool seen, float q, float nval, float raw, float prob, int cvis, int sum_visits, int A,
                             int lane) {
  if constexpr (QT == 0) {
    return wave_qtransform_by_parent_and_siblings(seen, q, nval);
  } else {
    const float prior = fmaxf(prob, kFltTiny);
    const float sum_probs = wave_sum16(seen ? prior : 0.0f, A, lane);
    const float weighted_q = wave_sum16(seen ? (prior * q) / sum_probs : 0.0f, A, lane);
    const float mixed = (raw + (float)sum_visits * weighted_q) / (float)(sum_visits + 1);
    const float out = seen ? q : mixed;
    const float lo = wave_min(ok ? out : INFINITY), hi = wave_max(ok ? out : -INFINITY);
    const float span = fmaxf(hi - lo, 1e-8f);
    const float scale = (50.0f + (float)wave_max_count(cvis)) * 0.1f;
    return scale * ((out - lo) / span);
  }
}
// seq_halving.score_considered + the root's invalid-action mask (oracle gumbel_argmax), this lane's action
MZ_DEV float wide_score_considered(bool ok, bool inv, float gum, float logit, float qv, int cvis, int considered_visit) {
  const float mx = wave_max(ok ? logit : -INFINITY);
  float sc = fmaxf((gum + (logit - mx)) + qv, -1e9f);
  sc = sc + (cvis == considered_visit ? 0.0f : -INFINITY);
  return (!ok || inv) ? -INFINITY : sc;
}

template <int MODE>
__global__ __launch_bounds__(64 * kWideMaxWaves) void mz_act_wide_kernel(const FusedParams p, const WideShape sh) {
  static_assert(MODE >= 0 && MODE <= 3, "mode of the fused dispatchers");
  constexpr bool TIEBREAK = MODE == 1, GUMBEL = MODE >= 2;
  constexpr int QT = MODE == 3 ? 1 : 0;
  extern __shared__ int wide_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int A = sh.A, E = sh.E, F = sh.F, H = kHidden, X = E + A;
  const int S = p.S, N = S + 1, REC = sh.rec_words;

  // ---- workgroup prologue: weights and the pUCT table into LDS ----
  float* wl = reinterpret_cast<float*>(wide_lds);
  WideNets nets;
  {
    const float* src[16] = {p.pv_w1, p.pv_b1, p.pv_w2, p.pv_b2, p.pp_w1, p.pp_b1, p.pp_w2, p.pp_b2,
                            p.dr_w1, p.dr_b1, p.dr_w2, p.dr_b2, p.dn_w1, p.dn_b1, p.dn_w2, p.dn_b2};
    const int cnt[16] = {E * H, H, H * F, F, E * H, H, H * A, A, X * H, H, H * F, F, X * H, H, H * E, E};
    const float** dst = &nets.pv_w1;
    int off = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      for (int k = tid; k < cnt[i]; k += blockDim.x) wl[off + k] = src[i][k];
      dst[i] = wl + off;
      off += cnt[i];
    }
  }
  float* tbl = wl + sh.weight_words;
  wave_stage_puct_table(tbl, S, p.pb_c_init, p.pb_c_base);
  __syncthreads();

  const int r = blockIdx.x * sh.waves + wave;
  if (r >= p.B) return;  // (after the only workgroup barrier; from here on a wavefront is on its own)
  const uint64_t rg = p.root_offset + (uint64_t)r;
  const int max_depth = p.max_depth > 0 ? p.max_depth : S;
  const bool ex = p.export_tree != 0;
  const bool ok = lane < A;
  const int ac = ok ? lane : 0;          // this lane's action, clamped for addressing
  const int ec = lane < E ? lane : 0, fc = lane < F ? lane : 0;
  const int u = lane & 15, grp = (lane >> 4) & 1;  // hidden unit and which of the two side-by-side nets
  const float disc = p.discount;

  // ---- this root's block (mz_wave_tree.cuh; the record has the prior logits in the Gumbel modes) ----
  int* tree = wide_lds + sh.wg_words + wave * sh.root_words;
  int* path = wave_tree_setup(tree, sh.root_words, N, REC, lane);
  float* emb = sh.emb_lds ? reinterpret_cast<float*>(path + N) : (ex ? p.t_embeddings : p.emb_scratch) + (size_t)r * N * E;
  const size_t tn0 = (size_t)r * N;  // this root's first node in the export arrays
  const bool inv = (p.invalid != nullptr && ok) ? p.invalid[(size_t)r * A + ac] != 0 : false;
  wave_sync();

  // Prediction (muax/nn.py:73-90) on the state whose element k is in lane k of `s`: prior logit a in lane a, value
  auto prediction = [&](float s, float& logit, float& value) {
    const float h = elu(wide_chain(s, E, (grp ? nets.pp_w1 : nets.pv_w1) + u) + (grp ? nets.pp_b1 : nets.pv_b1)[u]);
    const float vl = wide_out<0>(h, nets.pv_w2, nets.pv_b2, F, fc);
    logit = wide_out<16>(h, nets.pp_w2, nets.pp_b2, A, ac);
    value = wave_decode(vl, F, p.support, lane);
  };

  // Gumbel modes: this lane's root Gumbel noise, the number of root actions sequential halving considers, and whether
  // the root's mask has an invalid action (mctx masks the completed logits only then)
  [[maybe_unused]] float gum = 0.0f;
  [[maybe_unused]] int ncons = 0;
  [[maybe_unused]] bool any_inv = false;

  // ---- root inference (muax/model.py:251-263) and the policy's prelude (MuZero: Dirichlet mix, mask; Gumbel: mask) ----
  {
    const float* ob = p.obs + (size_t)r * p.obs_dim;
    float acc = 0.0f;
    int i = 0;
    for (; i + 4 <= p.obs_dim; i += 4) {
      float o4[4], w4[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        o4[q] = ob[i + q];
        w4[q] = p.repr_w[(size_t)(i + q) * E + ec];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) acc = __builtin_fmaf(o4[q], w4[q], acc);
    }
    for (; i < p.obs_dim; ++i) acc = __builtin_fmaf(ob[i], p.repr_w[(size_t)i * E + ec], acc);
    const float s = wave_min_max_normalize(acc + p.repr_b[ec], E, lane);
    if (lane < E) emb[lane] = s;
    float logit, value;
    prediction(s, logit, value);
    float lg;
    if constexpr (!GUMBEL) {
      const float pr = wave_softmax(logit, A, lane);
      const float nz = (p.dirichlet_noise != nullptr && ok) ? p.dirichlet_noise[(size_t)r * A + ac] : 0.0f;
      const float noisy = (1.0f - p.dirichlet_fraction) * pr + p.dirichlet_fraction * nz;
      lg = log_pos(fmaxf(noisy, kFltTiny));
      if (p.invalid != nullptr) {
        const float top = wave_max(ok ? lg : -INFINITY);
        lg = inv ? kFltLowest : lg - top;
      }
    } else {
      // mctx gumbel_muzero_policy prelude: the logits only pass through _mask_invalid_actions; root Gumbel noise
      lg = logit;
      const unsigned long long inv_lanes = __builtin_amdgcn_ballot_w64(inv);
      any_inv = inv_lanes != 0;
      if (any_inv) {
        const float top = wave_max(ok ? lg : -INFINITY);
        lg = inv ? kFltLowest : lg - top;
      }
      ncons = min(p.max_considered, A - (int)__builtin_popcountll(inv_lanes));
      if (p.gumbel != nullptr) {
        gum = ok ? p.gumbel[(size_t)r * A + ac] : 0.0f;
      } else {
        uint32_t x0, x1;
        bool second;
        bits_block(p.global_batch * (uint64_t)A, rg * (uint64_t)A + (uint64_t)ac, x0, x1, second);
        threefry2x32(p.k_gumbel[0], p.k_gumbel[1], x0, x1);
        gum = p.gumbel_scale * gumbel_from_bits(second ? x1 : x0);
      }
    }
    float prob = 0.0f;  // (qtransform_by_parent_and_siblings under the Gumbel policy never reads a prior probability)
    if constexpr (MODE != 2) prob = wave_softmax(lg, A, lane);
    if (ok) {
      tree[rec_child(kChildProb, A, ac)] = __float_as_int(prob);
      if constexpr (GUMBEL) tree[rec_child(kChildLogit, A, ac)] = __float_as_int(lg);
      if (ex) p.t_children_prior_logits[tn0 * A + ac] = lg;
    }
    if (lane == 0) {
      tree[kRecVisits] = 1;
      tree[kRecValue] = __float_as_int(value);
      tree[kRecRaw] = __float_as_int(value);
      p.root_value[r] = value;
    }
    wave_sync();
  }

  // ---- simulations (mctx search.simulate / expand / backward) ----
  int depth_sum = 0;
  for (int sim = 0; sim < S; ++sim) {
    [[maybe_unused]] uint32_t kk0 = 0, kk1 = 0;  // the tie-break key walk (wave_noisy_argmax)
    [[maybe_unused]] int klevel = -1;
    int node = 0, depth = 0, parent = 0, action = 0, next = -1;
    for (;;) {
      const int* rec = tree + node * REC;
      const int nvis = rec[kRecVisits];
      const float nval = __int_as_float(rec[kRecValue]);
      const int link = rec[rec_child(kChildLink, A, ac)];
      const float prob = __int_as_float(rec[rec_child(kChildProb, A, ac)]);
      const float cval = __int_as_float(rec[rec_child(kChildValue, A, ac)]);
      const float crew = __int_as_float(rec[rec_child(kChildReward, A, ac)]);
      const int cvis = link_visits(link), cidx = link_child(link);
      const bool seen = ok && cvis > 0;
      const float q = crew + disc * cval;
      float sc;
      if constexpr (!GUMBEL) {
        sc = wave_puct_score(seen, q, nval, tbl[nvis], prob, cvis);
        if (!ok || (depth == 0 && inv)) sc = -INFINITY;
      } else {
        // mctx gumbel_muzero_root_action_selection / gumbel_muzero_interior_action_selection (no tie-break noise)
        const float lgt = __int_as_float(rec[rec_child(kChildLogit, A, ac)]);
        const int vis = ok ? cvis : 0;
        const int sumv = (QT == 1 || depth != 0) ? wave_sum_i(vis) : 0;
        const float qv = wide_qtransform<QT>(ok, seen, q, nval, __int_as_float(rec[kRecRaw]), prob, vis, sumv, A, lane);
        if (depth == 0) {
          sc = wide_score_considered(ok, inv, gum, lgt, qv, vis, p.visit_table[(size_t)ncons * S + sim]);
        } else {
          const float pr = wave_softmax(lgt + qv, A, lane);
          sc = ok ? pr - (float)vis / (float)(1 + sumv) : -INFINITY;
        }
      }
      const int best = wave_noisy_argmax<TIEBREAK>(sc, ok, ac, A, depth, lane, p.global_batch, rg,
                                                   [&](int i) { return p.sim_keys[sim][i]; }, kk0, kk1, klevel);
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

    // recurrent_fn (muax/model.py:265-282): Dynamic on [state, onehot(action)], Prediction on the next state (or, the
    // pip release's quirk, on the parent's)
    const float s_par = lane < E ? emb[parent * E + ec] : 0.0f;
    float reward, logit, value;
    {
      const float* w1 = (grp ? nets.dn_w1 : nets.dr_w1) + u;
      float a1 = wide_chain(s_par, E, w1);
      a1 = __builtin_fmaf(1.0f, w1[(E + action) * H], a1);  // (the one-hot's other links add nothing: see the header)
      const float h = elu(a1 + (grp ? nets.dn_b1 : nets.dr_b1)[u]);
      const float rl = wide_out<0>(h, nets.dr_w2, nets.dr_b2, F, fc);
      const float ns = wave_min_max_normalize(wide_out<16>(h, nets.dn_w2, nets.dn_b2, E, ec), E, lane);
      if (lane < E) emb[newn * E + ec] = ns;
      reward = wave_decode(rl, F, p.support, lane);
      prediction(p.pred_on_parent ? s_par : ns, logit, value);
    }
    float prob = 0.0f;
    if constexpr (MODE != 2) prob = wave_softmax(logit, A, lane);

    if (ex && ok) p.t_children_prior_logits[(tn0 + newn) * A + ac] = logit;
    wave_tree_expand<GUMBEL>(tree, REC, A, newn, parent, action, false, ok, ac, lane, prob, logit, value, reward);
    wave_tree_backward<false>(tree, path, REC, A, depth, value, disc, lane);
  }

  if constexpr (GUMBEL) {
    // ---- tail of mctx gumbel_muzero_policy (oracle mzo_gumbel_finish): the best of the most visited actions by
    // gumbel + logits + completed Q, action_weights = softmax(logits + completed Q) under the root's mask ----
    const int vis = ok ? link_visits(tree[rec_child(kChildLink, A, ac)]) : 0;
    const float q = __int_as_float(tree[rec_child(kChildReward, A, ac)]) + disc * __int_as_float(tree[rec_child(kChildValue, A, ac)]);
    const float lgt = __int_as_float(tree[rec_child(kChildLogit, A, ac)]);
    const float nval = __int_as_float(tree[kRecValue]);
    const float qv = wide_qtransform<QT>(ok, vis > 0, q, nval, __int_as_float(tree[kRecRaw]),
                                         __int_as_float(tree[rec_child(kChildProb, A, ac)]), vis, wave_sum_i(vis), A, lane);
    const int best = wave_first_max(wide_score_considered(ok, inv, gum, lgt, qv, vis, wave_max_count(vis)));
    float x = lgt + qv;
    const float mx = wave_max(ok ? x : -INFINITY);
    if (any_inv) x = inv ? kFltLowest : x - mx;
    const float w = wave_softmax(x, A, lane);
    if (ok) p.action_weights[(size_t)r * A + ac] = w;
    if (lane == 0) {
      p.action[r] = best;
      if (p.search_value) p.search_value[r] = nval;
      if (p.depth_sum) p.depth_sum[r] = depth_sum;
    }
  } else {
    float pw;
    const int best = wave_summary_sample(tree, A, A, ok, ac, lane, p.temperature, p.gumbel ? p.gumbel + (size_t)r * A : nullptr,
                                         p.global_batch, rg, [&](int i) { return p.k_sample[i]; }, pw);
    if (ok) p.action_weights[(size_t)r * A + ac] = pw;
    if (lane == 0) {
      p.action[r] = best;
      if (p.search_value) p.search_value[r] = __int_as_float(tree[kRecValue]);
      if (p.depth_sum) p.depth_sum[r] = depth_sum;
    }
  }

  if (ex) wave_tree_export<false>(p, tree, emb, sh.emb_lds, r, N, REC, A, E, ok, ac, lane, disc);
}

}  // namespace mz
