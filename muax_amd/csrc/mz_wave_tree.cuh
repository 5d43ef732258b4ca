// mz_wave_tree.cuh -- what the one-launch search kernels with ONE ROOT PER WAVEFRONT share (mz_wide.cuh: the MLP trio
// for 17..64 actions; mz_stoch_wide.cuh: Stochastic MuZero): the wavefront primitives, the tree record in LDS and the
// rules of mctx that do not depend on the nets or the policy, each stated once.
//
// The mapping: lane i owns slot i of a node (W <= 64 slots: the actions, then -- stochastic search -- the chance outcomes);
// a node's child arrays lie [field][slot], so a lane reads its own child with one LDS access per field, the scores of a
// level are computed lane-parallel, the argmax is a wavefront max (DPP butterfly per row, the four rows combined through
// v_readlane) and the first lane that holds it (ballot).  Selection walks level by level; backup runs lane per path
// entry in chunks of 64 levels: the return chain (two dependent operations per level) is the only serial part.
//
// A root's block of LDS: records [N][REC] | path [N] | embeddings [N][E] (or in HBM), N = S + 1.
//   record     kRecVisits, kRecValue, kRecRaw, kRecParent = rec_parent(), then W words per child field (rec_child):
//              kChildLink (link_child, link_visits), kChildProb, kChildValue, kChildReward[, kChildLogit (Gumbel policy)]
//   path word  path_word(): the node and the slot taken there, one word per level
// All zero is mctx's empty tree (every index is stored + 1).
#pragma once
#include "mz_fused.cuh"

#pragma clang fp contract(off)

namespace mz {

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
// first lane that holds the maximum (mctx argmax: first of equals); every lane past the slot count holds -inf
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
// muax/nn.py:37-44 over the E elements in lanes [0, E)
MZ_DEV float wave_min_max_normalize(float s, int E, int lane) {
  const float mn = wave_min(lane < E ? s : INFINITY), mx = wave_max(lane < E ? s : -INFINITY);
  float scale = mx - mn;
  scale = scale < 1e-5f ? scale + 1e-5f : scale;
  return (s - mn) / scale;
}
// Representation (muax/nn.py:59-70) of one root: element k of the normalised state in lane k (lanes past E hold nothing
// of use).  ob: the root's observation row [obs_dim]; repr_w [obs_dim][E], repr_b [E] in global memory, read once per
// root.  An fma chain over the observation in index order from 0, the bias added last (oracle mzo_root_inference)
MZ_DEV float wave_root_state(const float* ob, const float* repr_w, const float* repr_b, int obs_dim, int E, int lane) {
  const int ec = lane < E ? lane : 0;
  float acc = 0.0f;
  int i = 0;
  for (; i + 4 <= obs_dim; i += 4) {
    float o4[4], w4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      o4[q] = ob[i + q];
      w4[q] = repr_w[(size_t)(i + q) * E + ec];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) acc = __builtin_fmaf(o4[q], w4[q], acc);
  }
  for (; i < obs_dim; ++i) acc = __builtin_fmaf(ob[i], repr_w[(size_t)i * E + ec], acc);
  return wave_min_max_normalize(acc + repr_b[ec], E, lane);
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

// ---- the record ----
enum { kRecVisits, kRecValue, kRecRaw, kRecParent, kRecHead };                  // header words
enum { kChildLink, kChildProb, kChildValue, kChildReward, kChildLogit };        // child fields, W words each
MZ_DEV int rec_child(int field, int W, int slot) { return kRecHead + field * W + slot; }
constexpr int kLinkVisit = 1 << 16;  // kChildLink: (child + 1) | visits << 16
MZ_DEV int link_child(int link) { return (link & 0xffff) - 1; }
MZ_DEV int link_visits(int link) { return link >> 16; }
MZ_DEV int link_to(int link, int child) { return (link & ~0xffff) | (child + 1); }
// kRecParent: (parent + 1) | (slot + 1) << 16 | chance node << 30 (a chance node's edges carry the bound discount)
MZ_DEV int rec_parent(int parent, int slot, bool chance) { return (parent + 1) | ((slot + 1) << 16) | (chance ? 1 << 30 : 0); }
MZ_DEV int parent_node(int w) { return (w & 0xffff) - 1; }
MZ_DEV int parent_slot(int w) { return ((w >> 16) & 0xff) - 1; }
MZ_DEV bool parent_chance(int w) { return (w >> 30) & 1; }
MZ_DEV int path_word(int node, int slot) { return node | (slot << 16); }
MZ_DEV int path_node(int w) { return w & 0xffff; }
MZ_DEV int path_slot(int w) { return w >> 16; }

// sqrt(n) pb_c(n), n = 0 .. S + 1 (a node's visit count), staged by the whole workgroup
MZ_DEV void wave_stage_puct_table(float* tbl, int S, float pb_c_init, float pb_c_base) {
  for (int n = threadIdx.x; n < S + 2; n += blockDim.x) tbl[n] = puct_scale(n, pb_c_init, pb_c_base);
}
// This root's block of root_words words, zeroed; returns the path's place behind the N records.  The caller's
// wave_sync() comes before the first read
MZ_DEV int* wave_tree_setup(int* block, int root_words, int N, int REC, int lane) {
  int4* q4 = reinterpret_cast<int4*>(block);
  for (int q = lane; q < root_words / 4; q += 64) q4[q] = make_int4(0, 0, 0, 0);
  return block + N * REC;
}

// mctx qtransform_by_parent_and_siblings, this lane's child: q of a visited child (seen: false in lanes past the slots)
MZ_DEV float wave_qtransform_by_parent_and_siblings(bool seen, float q, float nval) {
  const float safe = seen ? q : nval;
  const float lo = fminf(nval, wave_min(safe)), hi = fmaxf(nval, wave_max(safe));
  const float span = fmaxf(hi - lo, 1e-8f);
  return ((seen ? q : lo) - lo) / span;
}
// mctx muzero_action_selection without its noise: scale = the pUCT table at the node's visit count
MZ_DEV float wave_puct_score(bool seen, float q, float nval, float scale, float prob, int cvis) {
  const float value_score = wave_qtransform_by_parent_and_siblings(seen, q, nval);
  const float policy_score = (scale * prob) / (float)(cvis + 1);
  return value_score + policy_score;
}

// argmax over the W slots of sc (-inf in the lanes that must not win), first of equals; TIEBREAK: after mctx's
// 1e-7 * uniform[0, 1) on every score.  If fl(score + 1e-7) < best for every other slot the draw cannot change the
// argmax (rounding is monotone): only a near tie pays for the threefry blocks (mz_step.cuh, noisy_argmax).
// The key chain of the simulation is advanced only as far as a near tie asks for: (kk0, kk1) = the key after `klevel`
// splits, klevel = -1 at the simulation's start; sim_key(i): word i of the simulation's key, read at the first near tie
template <bool TIEBREAK, class SimKey>
MZ_DEV int wave_noisy_argmax(float sc, bool ok, int sl, int W, int depth, int lane, uint64_t global_batch, uint64_t rg,
                             SimKey sim_key, uint32_t& kk0, uint32_t& kk1, int& klevel) {
  const float top = wave_max(sc);
  const unsigned long long at = __builtin_amdgcn_ballot_w64(sc == top);
  int best = at ? __builtin_ctzll(at) : 0;
  if constexpr (TIEBREAK) {
    const bool unsafe = ok && lane != best && !((sc + 1e-7f) < top);
    if (__builtin_amdgcn_ballot_w64(unsafe) != 0) {
      uint32_t s0 = 0, s1 = 0;
      if (klevel < 0) {  // this root's key of the simulation: split(simulate_key, global_batch)[root]
        uint32_t x0, x1;
        bool second;
        bits_block(2 * global_batch, 2 * rg + (uint64_t)(lane & 1), x0, x1, second);
        threefry2x32(sim_key(0), sim_key(1), x0, x1);
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
      const int NB = (W + 1) / 2, jb = sl < NB ? sl : sl - NB;
      uint32_t x0 = (uint32_t)jb, x1 = (NB + jb < W) ? (uint32_t)(NB + jb) : 0u;
      threefry2x32(s0, s1, x0, x1);
      const float noised = sc + 1e-7f * uniform_from_bits(sl < NB ? x0 : x1);
      best = wave_first_max(ok ? noised : -INFINITY);
    }
  }
  return best;
}

// expand (mctx update_tree_node + the edge `slot` of `parent`) of node newn; a node met again at max_depth keeps its
// children.  LOGIT: the record has the kChildLogit field
template <bool LOGIT>
MZ_DEV void wave_tree_expand(int* tree, int REC, int W, int newn, int parent, int slot, bool chance, bool ok, int sl, int lane,
                             float prob, float logit, float value, float reward) {
  int* nrec = tree + newn * REC;
  if (ok) {
    nrec[rec_child(kChildProb, W, sl)] = __float_as_int(prob);
    if constexpr (LOGIT) nrec[rec_child(kChildLogit, W, sl)] = __float_as_int(logit);
  }
  if (lane == 0) {
    nrec[kRecVisits] = nrec[kRecVisits] + 1;
    nrec[kRecValue] = __float_as_int(value);
    nrec[kRecRaw] = __float_as_int(value);
    nrec[kRecParent] = rec_parent(parent, slot, chance);
    int* prec = tree + parent * REC;
    prec[rec_child(kChildLink, W, slot)] = link_to(prec[rec_child(kChildLink, W, slot)], newn);
    prec[rec_child(kChildReward, W, slot)] = __float_as_int(reward);
  }
  wave_sync();
}

// backward: lane l owns path entry base + l of a chunk of up to 64 levels, deepest chunk first.  PARITY: the edge of
// level d has discount 1 where d is even (it leaves a decision node of the stochastic search), else every edge has `disc`
template <bool PARITY>
MZ_DEV void wave_tree_backward(int* tree, const int* path, int REC, int W, int depth, float value, float disc, int lane) {
  float leaf = value, childv = value;
  for (int top = depth; top > 0; top -= 64) {
    const int base = top > 64 ? top - 64 : 0, n = top - base;
    const bool mine = lane < n;
    const int pk = path[base + (mine ? lane : 0)];
    int* prec = tree + path_node(pk) * REC;
    const int pa = path_slot(pk);
    const int cnt = prec[kRecVisits];
    const float nv = __int_as_float(prec[kRecValue]);
    const float rw = __int_as_float(prec[rec_child(kChildReward, W, pa)]);
    [[maybe_unused]] const float ds = ((base + lane) & 1) ? disc : 1.0f;
    const int link = prec[rec_child(kChildLink, W, pa)];
    float myleaf = 0.0f;
    for (int l = n - 1; l >= 0; --l) {  // leaf_value = reward + discount * leaf_value, level by level
      if constexpr (PARITY) leaf = w_rdl(rw, l) + w_rdl(ds, l) * leaf;
      else leaf = w_rdl(rw, l) + disc * leaf;
      myleaf = lane == l ? leaf : myleaf;
    }
    const float newv = (nv * (float)cnt + myleaf) / ((float)cnt + 1.0f);
    const float below = __shfl_down(newv, 1);
    const float cv = lane == n - 1 ? childv : below;  // children_values = the child's node value after ITS update
    if (mine) {
      prec[kRecVisits] = cnt + 1;
      prec[kRecValue] = __float_as_int(newv);
      prec[rec_child(kChildValue, W, pa)] = __float_as_int(cv);
      prec[rec_child(kChildLink, W, pa)] = link + kLinkVisit;
    }
    childv = w_rdl(newv, 0);
  }
  wave_sync();
}

// mctx Tree.summary + _apply_temperature + jax.random.categorical over the root's A actions (act: lane < A, al the
// clamped lane): the sampled action; pw = this lane's action weight.  gumbel: the root's row of given noise, or null:
// threefry from sample_key(0), sample_key(1)
template <class SampleKey>
MZ_DEV int wave_summary_sample(const int* tree, int W, int A, bool act, int al, int lane, float temperature,
                               const float* gumbel, uint64_t global_batch, uint64_t rg, SampleKey sample_key, float& pw) {
  const int vc = act ? link_visits(tree[rec_child(kChildLink, W, al)]) : 0;
  const float total = (float)wave_sum_i(vc);
  const float denom = fmaxf(total, 1.0f);
  pw = (float)vc / denom;
  pw = total > 0.0f ? pw : 1.0f / (float)A;
  const float lg = log_pos(fmaxf(pw, kFltTiny));
  const float mx = wave_max(act ? lg : -INFINITY);
  const float tden = fmaxf(temperature, kFltTiny);
  float g;
  if (gumbel != nullptr) {
    g = act ? gumbel[al] : 0.0f;
  } else {
    uint32_t x0, x1;
    bool second;
    bits_block(global_batch * (uint64_t)A, rg * (uint64_t)A + (uint64_t)al, x0, x1, second);
    threefry2x32(sample_key(0), sample_key(1), x0, x1);
    g = gumbel_from_bits(second ? x1 : x0);
  }
  return wave_first_max(act ? (lg - mx) / tden + g : -INFINITY);
}

// The finished tree of root r into the HBM arrays p.t_* in mctx's layout ([B, N], [B, N, W], [B, N, E]); the prior
// logits of expanded nodes are there already.  STOCH, the handle's tree of the stochastic search: the prior
// probabilities, the root's mask over all slots, the depth sum, and discount 1 on the edges of decision nodes
template <bool STOCH, class Params>
MZ_DEV void wave_tree_export(const Params& p, const int* tree, const float* emb, bool emb_lds, int r, int N, int REC, int W,
                             int E, bool ok, int sl, int lane, float disc, bool root_masked = false, int depth_sum = 0) {
  const size_t tn0 = (size_t)r * N;  // this root's first node in the export arrays
  for (int n = lane; n < N; n += 64) {
    const int* rec = tree + n * REC;
    p.t_node_visits[tn0 + n] = rec[kRecVisits];
    p.t_node_values[tn0 + n] = __int_as_float(rec[kRecValue]);
    p.t_raw_values[tn0 + n] = __int_as_float(rec[kRecRaw]);
    p.t_parents[tn0 + n] = parent_node(rec[kRecParent]);
    p.t_action_from_parent[tn0 + n] = parent_slot(rec[kRecParent]);
  }
  if constexpr (STOCH) {
    if (ok) p.t_root_invalid[(size_t)r * W + sl] = root_masked ? 1 : 0;
    if (lane == 0) p.t_depth_sum[r] = depth_sum;
  }
  const int ec = lane < E ? lane : 0;
  for (int n = 0; n < N; ++n) {
    const int* rec = tree + n * REC;
    const bool empty = rec[kRecVisits] == 0;  // a node no simulation created (re-expansions at max_depth)
    const float edge_disc = (!STOCH || parent_chance(rec[kRecParent])) ? disc : 1.0f;
    if (ok) {
      const size_t o = (tn0 + n) * W + sl;
      const int link = rec[rec_child(kChildLink, W, sl)];
      p.t_children_index[o] = link_child(link);
      p.t_children_visits[o] = link_visits(link);
      if constexpr (STOCH) p.t_children_prior_probs[o] = __int_as_float(rec[rec_child(kChildProb, W, sl)]);
      p.t_children_values[o] = __int_as_float(rec[rec_child(kChildValue, W, sl)]);
      p.t_children_rewards[o] = __int_as_float(rec[rec_child(kChildReward, W, sl)]);
      p.t_children_discounts[o] = link_child(link) >= 0 ? edge_disc : 0.0f;
      if (empty) p.t_children_prior_logits[o] = 0.0f;
    }
    if (emb_lds) {
      if (lane < E) p.t_embeddings[(tn0 + n) * E + ec] = emb[n * E + ec];
    } else if (empty && lane < E) {
      p.t_embeddings[(tn0 + n) * E + ec] = 0.0f;
    }
  }
}

}  // namespace mz
