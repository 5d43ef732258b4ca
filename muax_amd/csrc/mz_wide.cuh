// mz_wide.cuh -- act() of the default MLP trio (muax/nn.py:59-115) under either policy for 17..64 actions in ONE launch,
// the root's tree in LDS: root inference, every simulation, the summary and the sampling, like mz_fused.cuh, but mapped
// for wide action sets.  mz_fused.cuh keeps all scores of a node in one lane (A <= 16); here
//
//   * one root per WAVEFRONT, lane a owns action a (A <= 64): a node's child arrays lie [field][action], a lane reads its
//     own child with one LDS access per field, the scores of a level are computed lane-parallel, the argmax is a wavefront
//     max (DPP butterfly per row, the four rows combined through v_readlane) and the first lane that holds it (ballot);
//   * selection walks level by level (no JUMP words, no cached decisions: a level is a few dozen instructions here);
//   * backup runs lane per path entry in chunks of 64 levels: the return chain (two dependent operations per level) is
//     the only serial part, the divisions and the record updates of all levels run side by side;
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
#include "mz_fused.cuh"
#include "mz_wide_launch.h"

#pragma clang fp contract(off)

namespace mz {

struct WideShape {
  int A, E, F, rec_words, root_words, wg_words, weight_words, emb_lds, waves;
};

MZ_DEV float w_rdl(float x, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l)); }
MZ_DEV int w_rdl_i(int x, int l) { return __builtin_amdgcn_readlane(x, l); }
// reductions over the wavefront, the result uniform (min / max / integer sums do not depend on the order)
MZ_DEV float wave_max(float x) {
  x = row_max<4>(x);
  return fmaxf(fmaxf(w_rdl(x, 0), w_rdl(x, 16)), fmaxf(w_rdl(x, 32), w_rdl(x, 48)));
}
MZ_DEV float wave_min(float x) {
  x = row_min<4>(x);
  return fminf(fminf(w_rdl(x, 0), w_rdl(x, 16)), fminf(w_rdl(x, 32), w_rdl(x, 48)));
}
MZ_DEV int wave_sum_i(int x) {
  x = row_sum_i(x);
  return (w_rdl_i(x, 0) + w_rdl_i(x, 16)) + (w_rdl_i(x, 32) + w_rdl_i(x, 48));
}
// maximum of small non-negative integers (visit counts: exact as floats)
MZ_DEV int wave_max_count(int x) { return (int)wave_max((float)x); }
// first lane that holds the maximum (mctx argmax: first of equals); every lane past the action count holds -inf
MZ_DEV int wave_first_max(float sc) {
  const float m = wave_max(sc);
  const unsigned long long at = __builtin_amdgcn_ballot_w64(sc == m);
  return at ? __builtin_ctzll(at) : 0;
}
// the canonical 16-wide sum of x[0..n), element i in lane i (n >= 16: slot 0 is full): every row gathers the four slots
// of its lane index, so the sum lands in every lane
MZ_DEV float wave_sum16(float x, int n, int lane) {
  const int l = lane & 15;
  float part = __shfl(x, l);
#pragma unroll
  for (int t = 1; t < 4; ++t) {
    const float v = __shfl(x, l + 16 * t);
    part = (l + 16 * t < n) ? part + v : part;
  }
  return row_sum(part);
}
// jax.nn.softmax over x[0..n), element i in lane i (lanes past n get 0)
MZ_DEV float wave_softmax(float x, int n, int lane) {
  const bool ok = lane < n;
  const float m = wave_max(ok ? x : -INFINITY);
  const float e = ok ? exp_neg(x - m) : 0.0f;
  return e / wave_sum16(e, n, lane);
}
// support_to_scalar(softmax(logits)) (muax/utils.py:70-102), logit k in lane k
MZ_DEV float wave_decode(float logit, int F, int support, int lane) {
  const float p = wave_softmax(logit, F, lane);
  return inv_scaling(wave_sum16((float)(lane - support) * p, F, lane));
}
// links [0, n) of a hidden layer's chain: input k in lane k of x, this lane's weights w[k * 16]
MZ_DEV float wide_chain(float x, int n, const float* w) {
  float acc = 0.0f;
  int k = 0;
  for (; k + 8 <= n; k += 8) {
    float wv[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) wv[q] = w[(k + q) * kHidden];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc = __builtin_fmaf(w_rdl(x, k + q), wv[q], acc);
  }
  for (; k < n; ++k) acc = __builtin_fmaf(w_rdl(x, k), w[k * kHidden], acc);
  return acc;
}
// output j of a layer over the 16 hidden units in lanes [BASE, BASE + 16) of h; w [16][n_out], jc = min(j, n_out - 1)
template <int BASE>
MZ_DEV float wide_out(float h, const float* w, const float* b, int n_out, int jc) {
  float wv[kHidden];
#pragma unroll
  for (int k = 0; k < kHidden; ++k) wv[k] = w[k * n_out + jc];
  float acc = 0.0f;
#pragma unroll
  for (int k = 0; k < kHidden; ++k) acc = __builtin_fmaf(w_rdl(h, BASE + k), wv[k], acc);
  return acc + b[jc];
}
// LDS writes of one lane read by another lane of the same wavefront later: keep the compiler from moving either
MZ_DEV void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

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
    const float safe = seen ? q : nval;
    const float lo = fminf(nval, wave_min(safe)), hi = fmaxf(nval, wave_max(safe));
    const float span = fmaxf(hi - lo, 1e-8f);
    return ((seen ? q : lo) - lo) / span;
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
  float* tbl = wl + sh.weight_words;  // sqrt(n) pb_c(n), n = 0 .. S + 1 (a node's visit count)
  for (int n = tid; n < S + 2; n += blockDim.x) tbl[n] = puct_scale(n, p.pb_c_init, p.pb_c_base);
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

  // ---- this root's block: records [N][REC] | path [N] | embeddings [N][E] (or in HBM) ----
  // record: visits, value, raw value, (parent + 1) | (action + 1) << 16, then per action: (child + 1) | visits << 16,
  // prior probability, child value, reward[, prior logit (Gumbel modes)] -- all zero is mctx's empty tree
  int* tree = wide_lds + sh.wg_words + wave * sh.root_words;
  int* path = tree + N * REC;
  {
    int4* q4 = reinterpret_cast<int4*>(tree);
    for (int q = lane; q < sh.root_words / 4; q += 64) q4[q] = make_int4(0, 0, 0, 0);
  }
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
    float s = acc + p.repr_b[ec];
    const float mn = wave_min(lane < E ? s : INFINITY), mx = wave_max(lane < E ? s : -INFINITY);
    float scale = mx - mn;
    scale = scale < 1e-5f ? scale + 1e-5f : scale;
    s = (s - mn) / scale;
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
      tree[4 + A + ac] = __float_as_int(prob);
      if constexpr (GUMBEL) tree[4 + 4 * A + ac] = __float_as_int(lg);
      if (ex) p.t_children_prior_logits[tn0 * A + ac] = lg;
    }
    if (lane == 0) {
      tree[0] = 1;
      tree[1] = __float_as_int(value);
      tree[2] = __float_as_int(value);
      p.root_value[r] = value;
    }
    wave_sync();
  }

  // ---- simulations (mctx search.simulate / expand / backward) ----
  int depth_sum = 0;
  for (int sim = 0; sim < S; ++sim) {
    // the tie-break key walk, advanced only as far as a near tie asks for: kk = the key after `klevel` splits
    uint32_t kk0 = 0, kk1 = 0;
    int klevel = -1;
    int node = 0, depth = 0, parent = 0, action = 0, next = -1;
    for (;;) {
      const int* rec = tree + node * REC;
      const int nvis = rec[0];
      const float nval = __int_as_float(rec[1]);
      const int iv = rec[4 + ac];
      const float prob = __int_as_float(rec[4 + A + ac]);
      const float cval = __int_as_float(rec[4 + 2 * A + ac]);
      const float crew = __int_as_float(rec[4 + 3 * A + ac]);
      const int cvis = iv >> 16, cidx = (iv & 0xffff) - 1;
      const bool seen = ok && cvis > 0;
      const float q = crew + disc * cval;
      float sc;
      if constexpr (!GUMBEL) {
        const float safe = seen ? q : nval;
        const float lo = fminf(nval, wave_min(safe)), hi = fmaxf(nval, wave_max(safe));
        const float span = fmaxf(hi - lo, 1e-8f);
        const float value_score = ((seen ? q : lo) - lo) / span;
        const float policy_score = (tbl[nvis] * prob) / (float)(cvis + 1);
        sc = value_score + policy_score;
        if (!ok || (depth == 0 && inv)) sc = -INFINITY;
      } else {
        // mctx gumbel_muzero_root_action_selection / gumbel_muzero_interior_action_selection (no tie-break noise)
        const float lgt = __int_as_float(rec[4 + 4 * A + ac]);
        const int vis = ok ? cvis : 0;
        const int sumv = (QT == 1 || depth != 0) ? wave_sum_i(vis) : 0;
        const float qv = wide_qtransform<QT>(ok, seen, q, nval, __int_as_float(rec[2]), prob, vis, sumv, A, lane);
        if (depth == 0) {
          sc = wide_score_considered(ok, inv, gum, lgt, qv, vis, p.visit_table[(size_t)ncons * S + sim]);
        } else {
          const float pr = wave_softmax(lgt + qv, A, lane);
          sc = ok ? pr - (float)vis / (float)(1 + sumv) : -INFINITY;
        }
      }
      float top = wave_max(sc);
      unsigned long long at = __builtin_amdgcn_ballot_w64(sc == top);
      int best = at ? __builtin_ctzll(at) : 0;
      if constexpr (TIEBREAK) {
        // mctx adds 1e-7 * uniform[0, 1) to every score; if fl(score_a + 1e-7) < best for every other action the draw cannot
        // change the argmax (rounding is monotone): only a near tie pays for the threefry blocks (mz_step.cuh, noisy_argmax)
        const bool unsafe = ok && lane != best && !((sc + 1e-7f) < top);
        if (__builtin_amdgcn_ballot_w64(unsafe) != 0) {
          uint32_t s0 = 0, s1 = 0;
          if (klevel < 0) {  // this root's key of the simulation: split(simulate_key, global_batch)[root]
            uint32_t x0, x1;
            bool second;
            bits_block(2 * p.global_batch, 2 * rg + (uint64_t)(lane & 1), x0, x1, second);
            threefry2x32(p.sim_keys[sim][0], p.sim_keys[sim][1], x0, x1);
            const uint32_t word = second ? x1 : x0;
            kk0 = (uint32_t)w_rdl_i((int)word, 0);
            kk1 = (uint32_t)w_rdl_i((int)word, 1);
            klevel = 0;
          }
          while (klevel <= depth) {  // rng_key, action_selection_key = split(rng_key), once per level
            uint32_t x0 = (uint32_t)(lane & 1), x1 = 2u + (uint32_t)(lane & 1);
            threefry2x32(kk0, kk1, x0, x1);
            kk0 = (uint32_t)w_rdl_i((int)x0, 0);
            kk1 = (uint32_t)w_rdl_i((int)x0, 1);
            s0 = (uint32_t)w_rdl_i((int)x1, 0);
            s1 = (uint32_t)w_rdl_i((int)x1, 1);
            ++klevel;
          }
          const int NB = (A + 1) / 2, jb = ac < NB ? ac : ac - NB;
          uint32_t x0 = (uint32_t)jb, x1 = (NB + jb < A) ? (uint32_t)(NB + jb) : 0u;
          threefry2x32(s0, s1, x0, x1);
          const float noised = sc + 1e-7f * uniform_from_bits(ac < NB ? x0 : x1);
          sc = ok ? noised : -INFINITY;
          top = wave_max(sc);
          at = __builtin_amdgcn_ballot_w64(sc == top);
          best = at ? __builtin_ctzll(at) : 0;
        }
      }
      if (lane == 0) path[depth] = node | (best << 16);
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
      float ns = wide_out<16>(h, nets.dn_w2, nets.dn_b2, E, ec);
      const float mn = wave_min(lane < E ? ns : INFINITY), mx = wave_max(lane < E ? ns : -INFINITY);
      float scale = mx - mn;
      scale = scale < 1e-5f ? scale + 1e-5f : scale;
      ns = (ns - mn) / scale;
      if (lane < E) emb[newn * E + ec] = ns;
      reward = wave_decode(rl, F, p.support, lane);
      prediction(p.pred_on_parent ? s_par : ns, logit, value);
    }
    float prob = 0.0f;
    if constexpr (MODE != 2) prob = wave_softmax(logit, A, lane);

    // expand (update_tree_node + the edge); a node met again at max_depth keeps its children
    {
      int* nrec = tree + newn * REC;
      if (ok) {
        nrec[4 + A + ac] = __float_as_int(prob);
        if constexpr (GUMBEL) nrec[4 + 4 * A + ac] = __float_as_int(logit);
        if (ex) p.t_children_prior_logits[(tn0 + newn) * A + ac] = logit;
      }
      if (lane == 0) {
        nrec[0] = nrec[0] + 1;
        nrec[1] = __float_as_int(value);
        nrec[2] = __float_as_int(value);
        nrec[3] = (parent + 1) | ((action + 1) << 16);
        int* prec = tree + parent * REC;
        prec[4 + action] = (prec[4 + action] & ~0xffff) | (newn + 1);
        prec[4 + 3 * A + action] = __float_as_int(reward);
      }
      wave_sync();
    }

    // backward: lane l owns path entry base + l of a chunk of up to 64 levels, deepest chunk first
    {
      float leaf = value, childv = value;
      for (int top = depth; top > 0; top -= 64) {
        const int base = top > 64 ? top - 64 : 0, n = top - base;
        const bool mine = lane < n;
        const int pk = path[base + (mine ? lane : 0)];
        int* prec = tree + (pk & 0xffff) * REC;
        const int pa = pk >> 16;
        const int cnt = prec[0];
        const float nv = __int_as_float(prec[1]);
        const float rw = __int_as_float(prec[4 + 3 * A + pa]);
        const int iv = prec[4 + pa];
        float myleaf = 0.0f;
        for (int l = n - 1; l >= 0; --l) {  // leaf_value = reward + discount * leaf_value, level by level
          leaf = w_rdl(rw, l) + disc * leaf;
          myleaf = lane == l ? leaf : myleaf;
        }
        const float newv = (nv * (float)cnt + myleaf) / ((float)cnt + 1.0f);
        const float below = __shfl_down(newv, 1);
        const float cv = lane == n - 1 ? childv : below;  // children_values = the child's node value after ITS update
        if (mine) {
          prec[0] = cnt + 1;
          prec[1] = __float_as_int(newv);
          prec[4 + 2 * A + pa] = __float_as_int(cv);
          prec[4 + pa] = iv + (1 << 16);
        }
        childv = w_rdl(newv, 0);
      }
      wave_sync();
    }
  }

  if constexpr (GUMBEL) {
    // ---- tail of mctx gumbel_muzero_policy (oracle mzo_gumbel_finish): the best of the most visited actions by
    // gumbel + logits + completed Q, action_weights = softmax(logits + completed Q) under the root's mask ----
    const int vis = ok ? (tree[4 + ac] >> 16) : 0;
    const float q = __int_as_float(tree[4 + 3 * A + ac]) + disc * __int_as_float(tree[4 + 2 * A + ac]);
    const float lgt = __int_as_float(tree[4 + 4 * A + ac]);
    const float nval = __int_as_float(tree[1]);
    const float qv = wide_qtransform<QT>(ok, vis > 0, q, nval, __int_as_float(tree[2]), __int_as_float(tree[4 + A + ac]), vis,
                                         wave_sum_i(vis), A, lane);
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
    // ---- mctx Tree.summary + _apply_temperature + jax.random.categorical ----
    const int vc = ok ? (tree[4 + ac] >> 16) : 0;
    const float total = (float)wave_sum_i(vc);
    const float denom = fmaxf(total, 1.0f);
    float pw = (float)vc / denom;
    pw = total > 0.0f ? pw : 1.0f / (float)A;
    const float lg = log_pos(fmaxf(pw, kFltTiny));
    const float mx = wave_max(ok ? lg : -INFINITY);
    const float tden = fmaxf(p.temperature, kFltTiny);
    float g;
    if (p.gumbel != nullptr) {
      g = ok ? p.gumbel[(size_t)r * A + ac] : 0.0f;
    } else {
      uint32_t x0, x1;
      bool second;
      bits_block(p.global_batch * (uint64_t)A, rg * (uint64_t)A + (uint64_t)ac, x0, x1, second);
      threefry2x32(p.k_sample[0], p.k_sample[1], x0, x1);
      g = gumbel_from_bits(second ? x1 : x0);
    }
    const float score = ok ? (lg - mx) / tden + g : -INFINITY;
    const int best = wave_first_max(score);
    if (ok) p.action_weights[(size_t)r * A + ac] = pw;
    if (lane == 0) {
      p.action[r] = best;
      if (p.search_value) p.search_value[r] = __int_as_float(tree[1]);
      if (p.depth_sum) p.depth_sum[r] = depth_sum;
    }
  }

  // ---- tree export in mctx's layout (the prior logits of expanded nodes are there already) ----
  if (ex) {
    for (int n = lane; n < N; n += 64) {
      const int* rec = tree + n * REC;
      p.t_node_visits[tn0 + n] = rec[0];
      p.t_node_values[tn0 + n] = __int_as_float(rec[1]);
      p.t_raw_values[tn0 + n] = __int_as_float(rec[2]);
      p.t_parents[tn0 + n] = (rec[3] & 0xffff) - 1;
      p.t_action_from_parent[tn0 + n] = (rec[3] >> 16) - 1;
    }
    for (int n = 0; n < N; ++n) {
      const int* rec = tree + n * REC;
      const bool empty = rec[0] == 0;  // a node no simulation created (re-expansions at max_depth)
      if (ok) {
        const size_t o = (tn0 + n) * A + ac;
        const int iv = rec[4 + ac];
        const int cidx = (iv & 0xffff) - 1;
        p.t_children_index[o] = cidx;
        p.t_children_visits[o] = iv >> 16;
        p.t_children_values[o] = __int_as_float(rec[4 + 2 * A + ac]);
        p.t_children_rewards[o] = __int_as_float(rec[4 + 3 * A + ac]);
        p.t_children_discounts[o] = cidx >= 0 ? disc : 0.0f;
        if (empty) p.t_children_prior_logits[o] = 0.0f;
      }
      if (sh.emb_lds) {
        if (lane < E) p.t_embeddings[(tn0 + n) * E + ec] = emb[n * E + ec];
      } else if (empty && lane < E) {
        p.t_embeddings[(tn0 + n) * E + ec] = 0.0f;
      }
    }
  }
}

}  // namespace mz
