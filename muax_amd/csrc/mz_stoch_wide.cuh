// mz_stoch_wide.cuh -- the WHOLE stochastic search of the default stochastic MLP family (mctx stochastic_muzero_policy,
// DESIGN.md 4.7) in ONE launch, the root's tree in LDS: the root set-up of mzs_root_stochastic, every simulation (select
// -> decision or chance function -> expand -> backward), the summary and the sampling of mzs_finish_stochastic.  Root
// inference stays with the caller: the kernel takes the RootFnOutput arrays.  The mapping is mz_wide.cuh's, and so are
// the wavefront primitives (included, not restated):
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
// output) and the afterstate embedding are min-max normalised, hence non-negative.
//
// No atomics, nothing that depends on the launch geometry: a root's bits are the same whichever wavefront of whichever
// workgroup ran it.
#pragma once
#include "mz_stoch_wide_launch.h"
#include "mz_wide.cuh"

#pragma clang fp contract(off)

namespace mz {

struct StochWideShape {
  int rec_words, root_words, wg_words, weight_words, emb_lds, waves;
};
// one Linear(16)-elu-Linear head in LDS, haiku layout
struct StochHead {
  const float *w1, *b1, *w2, *b2;
};
// muax/nn.py:37-44 over the E elements in lanes [0, E)
MZ_DEV float wave_min_max_normalize(float s, int E, int lane) {
  const float mn = wave_min(lane < E ? s : INFINITY), mx = wave_max(lane < E ? s : -INFINITY);
  float scale = mx - mn;
  scale = scale < 1e-5f ? scale + 1e-5f : scale;
  return (s - mn) / scale;
}

// MODE 0 / 1: without / with mctx's tie-break noise at the decision nodes (the handle's `tiebreak`)
template <int MODE>
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
    StochHead h;
    h.w1 = stage(p.w[4 * i], n_in * H);
    h.b1 = stage(p.w[4 * i + 1], H);
    h.w2 = stage(p.w[4 * i + 2], H * n_out);
    h.b2 = stage(p.w[4 * i + 3], n_out);
    return h;
  };
  const StochHead ad = head(0, E + A, E), av = head(1, E, F), ac = head(2, E, C), cr = head(3, E + C, F),
                  cn = head(4, E + C, E), pv = head(5, E, F), pp = head(6, E, A);
  float* tbl = wl + sh.weight_words;  // sqrt(n) pb_c(n), n = 0 .. S + 1 (a node's visit count)
  for (int n = tid; n < S + 2; n += blockDim.x) tbl[n] = puct_scale(n, p.pb_c_init, p.pb_c_base);
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

  // ---- this root's block: records [N][REC] | path [N] | embeddings [N][E] (or in HBM) ----
  // record: visits, value, raw value, (parent + 1) | (slot + 1) << 16 | chance node << 30, then per slot: (child + 1) |
  // visits << 16, prior probability, child value, reward -- all zero is mctx's empty tree
  int* tree = stoch_lds + sh.wg_words + wave * sh.root_words;
  int* path = tree + N * REC;
  {
    int4* q4 = reinterpret_cast<int4*>(tree);
    for (int q = lane; q < sh.root_words / 4; q += 64) q4[q] = make_int4(0, 0, 0, 0);
  }
  float* emb = sh.emb_lds ? reinterpret_cast<float*>(path + N) : (ex ? p.t_embeddings : p.emb_scratch) + (size_t)r * N * E;
  const size_t tn0 = (size_t)r * N;  // this root's first node in the export arrays
  const bool inv = (p.invalid != nullptr && act) ? p.invalid[(size_t)r * A + al] != 0 : false;
  const bool root_masked = !act || inv;  // the root's mask over all slots: the chance slots and the invalid actions
  wave_sync();

  // ---- the root (mz_step_kernels.cuh root_row with AD = A): Dirichlet mix, log, mask over the actions, -inf on the
  // chance slots, the softmax over all slots ----
  {
    const float x = act ? p.prior_logits[(size_t)r * A + al] : 0.0f;
    const float pr = wave_softmax(x, A, lane);
    const float nz = (p.dirichlet_noise != nullptr && act) ? p.dirichlet_noise[(size_t)r * A + al] : 0.0f;
    const float noisy = (1.0f - fraction) * pr + fraction * nz;
    float lg = log_pos(fmaxf(noisy, kFltTiny));
    if (p.invalid != nullptr) {
      const float top = wave_max(act ? lg : -INFINITY);
      lg = inv ? kFltLowest : lg - top;
    }
    lg = act ? lg : -INFINITY;
    const float prob = wave_softmax(lg, AC, lane);
    if (lane < E) emb[lane] = p.embedding[(size_t)r * E + ec];
    if (ok) {
      tree[4 + AC + sl] = __float_as_int(prob);
      if (ex) p.t_children_prior_logits[tn0 * AC + sl] = lg;
    }
    if (lane == 0) {
      const float v = p.value[r];
      tree[0] = 1;
      tree[1] = __float_as_int(v);
      tree[2] = __float_as_int(v);
    }
    wave_sync();
  }

  // ---- simulations ----
  int depth_sum = 0;
  for (int sim = 0; sim < S; ++sim) {
    // the tie-break key walk, advanced only as far as a near tie asks for: kk = the key after `klevel` splits
    [[maybe_unused]] uint32_t kk0 = 0, kk1 = 0;
    [[maybe_unused]] int klevel = -1;
    int node = 0, depth = 0, parent = 0, action = 0, next = -1;
    for (;;) {
      const int* rec = tree + node * REC;
      const int iv = rec[4 + sl];
      const float prob = __int_as_float(rec[4 + AC + sl]);
      const int cvis = iv >> 16, cidx = (iv & 0xffff) - 1;
      int best;
      if (depth & 1) {
        // chance node (mz_step.cuh chance_decide): no noise, first maximum
        best = wave_first_max(ok ? prob / (float)(cvis + 1) : -INFINITY);
      } else {
        // decision node (level_decide): every edge has reward 0 and discount 1
        const int nvis = rec[0];
        const float nval = __int_as_float(rec[1]);
        const float q = __int_as_float(rec[4 + 3 * AC + sl]) + 1.0f * __int_as_float(rec[4 + 2 * AC + sl]);
        const bool seen = ok && cvis > 0;
        const float safe = seen ? q : nval;
        const float lo = fminf(nval, wave_min(safe)), hi = fmaxf(nval, wave_max(safe));
        const float span = fmaxf(hi - lo, 1e-8f);
        const float value_score = ((seen ? q : lo) - lo) / span;
        const float policy_score = (tbl[nvis] * prob) / (float)(cvis + 1);
        float sc = value_score + policy_score;
        if (!ok || (depth == 0 && root_masked)) sc = -INFINITY;
        float top = wave_max(sc);
        unsigned long long at = __builtin_amdgcn_ballot_w64(sc == top);
        best = at ? __builtin_ctzll(at) : 0;
        if constexpr (TIEBREAK) {
          // only a near tie pays for the threefry blocks (mz_step.cuh noisy_argmax; mz_wide.cuh)
          const bool unsafe = ok && lane != best && !((sc + 1e-7f) < top);
          if (__builtin_amdgcn_ballot_w64(unsafe) != 0) {
            uint32_t s0 = 0, s1 = 0;
            if (klevel < 0) {  // this root's key of the simulation: split(simulate_key, global_batch)[root]
              uint32_t x0, x1;
              bool second;
              bits_block(2 * p.global_batch, 2 * rg + (uint64_t)(lane & 1), x0, x1, second);
              threefry2x32(p.dyn ? p.dyn[kStochBlockHead + 2 * sim] : p.sim_keys[sim][0],
                           p.dyn ? p.dyn[kStochBlockHead + 2 * sim + 1] : p.sim_keys[sim][1], x0, x1);
              const uint32_t word = second ? x1 : x0;
              kk0 = (uint32_t)w_rdl_i((int)word, 0);
              kk1 = (uint32_t)w_rdl_i((int)word, 1);
              klevel = 0;
            }
            while (klevel <= depth) {  // rng_key, action_selection_key = split(rng_key), once per level of either kind
              uint32_t x0 = (uint32_t)(lane & 1), x1 = 2u + (uint32_t)(lane & 1);
              threefry2x32(kk0, kk1, x0, x1);
              kk0 = (uint32_t)w_rdl_i((int)x0, 0);
              kk1 = (uint32_t)w_rdl_i((int)x0, 1);
              s0 = (uint32_t)w_rdl_i((int)x1, 0);
              s1 = (uint32_t)w_rdl_i((int)x1, 1);
              ++klevel;
            }
            const int NB = (AC + 1) / 2, jb = sl < NB ? sl : sl - NB;
            uint32_t x0 = (uint32_t)jb, x1 = (NB + jb < AC) ? (uint32_t)(NB + jb) : 0u;
            threefry2x32(s0, s1, x0, x1);
            const float noised = sc + 1e-7f * uniform_from_bits(sl < NB ? x0 : x1);
            best = wave_first_max(ok ? noised : -INFINITY);
          }
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
      const StochHead d1 = decision ? ad : cn;  // the next embedding's head; the rows of lanes without a head repeat it
      const float* w1 = ((grp || decision) ? d1.w1 : cr.w1) + u;
      float a1 = wide_chain(s_par, E, w1);
      a1 = __builtin_fmaf(1.0f, w1[(E + hot) * H], a1);  // (the one-hot's other links add nothing: see the header)
      const float h = elu(a1 + ((grp || decision) ? d1.b1 : cr.b1)[u]);
      const float ns = wave_min_max_normalize(wide_out<16>(h, d1.w2, d1.b2, E, ec), E, lane);
      if (lane < E) emb[newn * E + ec] = ns;
      if (!decision) reward = wave_decode(wide_out<0>(h, cr.w2, cr.b2, F, fc), F, p.support, lane);
      const StochHead hv = decision ? av : pv, hp = decision ? ac : pp;
      const int n_pol = decision ? C : A, pj = decision ? lane - A : lane;
      const int pjc = pj < 0 ? 0 : (pj > n_pol - 1 ? n_pol - 1 : pj);
      const float h2 = elu(wide_chain(ns, E, (grp ? hp.w1 : hv.w1) + u) + (grp ? hp.b1 : hv.b1)[u]);
      const float vl = wide_out<0>(h2, hv.w2, hv.b2, F, fc);
      const float pl = wide_out<16>(h2, hp.w2, hp.b2, n_pol, pjc);
      value = wave_decode(vl, F, p.support, lane);
      logit = (pj >= 0 && pj < n_pol) ? pl : -INFINITY;  // the prior row: -inf on the slots of the other kind
    }
    const float prob = wave_softmax(logit, AC, lane);

    // expand (step_expand_backup_stochastic_kernel); a node met again at max_depth keeps its children
    {
      int* nrec = tree + newn * REC;
      if (ok) {
        nrec[4 + AC + sl] = __float_as_int(prob);
        if (ex) p.t_children_prior_logits[(tn0 + newn) * AC + sl] = logit;
      }
      if (lane == 0) {
        nrec[0] = nrec[0] + 1;
        nrec[1] = __float_as_int(value);
        nrec[2] = __float_as_int(value);
        nrec[3] = (parent + 1) | ((action + 1) << 16) | (decision ? 1 << 30 : 0);
        int* prec = tree + parent * REC;
        prec[4 + action] = (prec[4 + action] & ~0xffff) | (newn + 1);
        prec[4 + 3 * AC + action] = __float_as_int(reward);  // (0 from a decision parent)
      }
      wave_sync();
    }

    // backward: lane l owns path entry base + l of a chunk of up to 64 levels, deepest chunk first; the edge of level d
    // leaves a decision node (reward 0, discount 1) where d is even
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
        const float rw = __int_as_float(prec[4 + 3 * AC + pa]);
        const float ds = ((base + lane) & 1) ? disc : 1.0f;
        const int iv = prec[4 + pa];
        float myleaf = 0.0f;
        for (int l = n - 1; l >= 0; --l) {  // leaf_value = reward + discount * leaf_value, level by level
          leaf = w_rdl(rw, l) + w_rdl(ds, l) * leaf;
          myleaf = lane == l ? leaf : myleaf;
        }
        const float newv = (nv * (float)cnt + myleaf) / ((float)cnt + 1.0f);
        const float below = __shfl_down(newv, 1);
        const float cv = lane == n - 1 ? childv : below;  // children_values = the child's node value after ITS update
        if (mine) {
          prec[0] = cnt + 1;
          prec[1] = __float_as_int(newv);
          prec[4 + 2 * AC + pa] = __float_as_int(cv);
          prec[4 + pa] = iv + (1 << 16);
        }
        childv = w_rdl(newv, 0);
      }
      wave_sync();
    }
  }

  // ---- finish_row over the A actions: mctx Tree.summary + _apply_temperature + jax.random.categorical ----
  {
    const int vc = act ? (tree[4 + al] >> 16) : 0;
    const float total = (float)wave_sum_i(vc);
    const float denom = fmaxf(total, 1.0f);
    float pw = (float)vc / denom;
    pw = total > 0.0f ? pw : 1.0f / (float)A;
    const float lg = log_pos(fmaxf(pw, kFltTiny));
    const float mx = wave_max(act ? lg : -INFINITY);
    const float tden = fmaxf(temperature, kFltTiny);
    float g;
    if (p.gumbel != nullptr) {
      g = act ? p.gumbel[(size_t)r * A + al] : 0.0f;
    } else {
      uint32_t x0, x1;
      bool second;
      bits_block(p.global_batch * (uint64_t)A, rg * (uint64_t)A + (uint64_t)al, x0, x1, second);
      threefry2x32(p.dyn ? p.dyn[0] : p.k_sample[0], p.dyn ? p.dyn[1] : p.k_sample[1], x0, x1);
      g = gumbel_from_bits(second ? x1 : x0);
    }
    const int best = wave_first_max(act ? (lg - mx) / tden + g : -INFINITY);
    if (act) p.action_weights[(size_t)r * A + al] = pw;
    if (lane == 0) {
      p.action[r] = best;
      if (p.search_value) p.search_value[r] = __int_as_float(tree[1]);
      if (p.depth_sum) p.depth_sum[r] = depth_sum;
    }
  }

  // ---- the finished tree into the handle's HBM arrays, as the step-wise kernels leave them (the prior logits of
  // expanded nodes are there already) ----
  if (ex) {
    for (int n = lane; n < N; n += 64) {
      const int* rec = tree + n * REC;
      p.t_node_visits[tn0 + n] = rec[0];
      p.t_node_values[tn0 + n] = __int_as_float(rec[1]);
      p.t_raw_values[tn0 + n] = __int_as_float(rec[2]);
      p.t_parents[tn0 + n] = (rec[3] & 0xffff) - 1;
      p.t_action_from_parent[tn0 + n] = ((rec[3] >> 16) & 0xff) - 1;
    }
    if (ok) p.t_root_invalid[(size_t)r * AC + sl] = root_masked ? 1 : 0;
    if (lane == 0) p.t_depth_sum[r] = depth_sum;
    for (int n = 0; n < N; ++n) {
      const int* rec = tree + n * REC;
      const bool empty = rec[0] == 0;  // a node no simulation created (re-expansions at max_depth)
      const float edge_disc = (rec[3] >> 30) & 1 ? disc : 1.0f;  // the edges of a chance node carry the bound discount
      if (ok) {
        const size_t o = (tn0 + n) * AC + sl;
        const int iv = rec[4 + sl];
        const int cidx = (iv & 0xffff) - 1;
        p.t_children_index[o] = cidx;
        p.t_children_visits[o] = iv >> 16;
        p.t_children_prior_probs[o] = __int_as_float(rec[4 + AC + sl]);
        p.t_children_values[o] = __int_as_float(rec[4 + 2 * AC + sl]);
        p.t_children_rewards[o] = __int_as_float(rec[4 + 3 * AC + sl]);
        p.t_children_discounts[o] = cidx >= 0 ? edge_disc : 0.0f;
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
