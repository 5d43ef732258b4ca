// mz_step.cuh -- step-wise search for ARBITRARY plugin nets (the repr_fn /
// pred_fn / dy_fn surface of muax/model.py:52-54): the caller runs its own
// networks between mzs_select and mzs_expand_backup, exactly where mctx calls
// recurrent_fn (mctx search.expand).  The tree lives in HBM in mctx's own
// layout so that PolicyOutput.search_tree is a plain copy.  Same row mapping
// and arithmetic spec as the fused kernel; A and E are run-time (A <= 64).
//
// This header: the types and the per-node device functions BOTH sets of tree
// kernels share (every rule of the search is stated here once).  The cached-
// decision bodies are in mz_step_jump.cuh, every __global__ of the path in
// mz_step_kernels.cuh (included by mz_stepwise.hip alone).
#pragma once
#include "../../include/mzsearch.h"
#include "mz_spec.cuh"

#pragma clang fp contract(off)

namespace mz {

constexpr int kMaxAS = 4;  // action slots per lane (A <= 64)

struct StepArgs {
  int32_t B, N, A, E, S, max_depth, tiebreak;
  float pb_c_init, pb_c_base;
  uint64_t global_batch, root_offset;
  int32_t* node_visits; float* raw_values; float* node_values;
  int32_t* parents; int32_t* action_from_parent;
  int32_t* children_index; float* children_prior_logits; float* children_prior_probs;
  float* children_values; int32_t* children_visits; float* children_rewards;
  float* children_discounts; float* embeddings;
  uint8_t* root_invalid;
  int32_t *sel_parent, *sel_action, *sel_depth, *depth_sum, *path;
  // wide embeddings (E >= kWideEmb): the tree kernels only note WHICH node's row moves (xfer_node); the
  // rows themselves are moved by emb_gather / emb_scatter with a whole workgroup per KiB instead of the
  // 16 lanes that own the root
  int32_t* xfer_node;
  int32_t wide;
  const uint32_t* sim_keys;
  // gumbel policy
  int32_t qtransform, max_considered;
  float gumbel_scale;
  float* root_gumbel;           // [B, A]
  const int32_t* visit_table;   // [(max_considered + 1), S] seq_halving.get_table_of_considered_visits
  // stochastic policy: A = AD + C slots per node (AD actions, then C chance outcomes); every other policy: AD = A
  int32_t AD;
};

constexpr int kWideEmb = 256;

// children slots of a node: the actions and, under the stochastic policy, the chance outcomes after them
inline int slots_per_node(const mzs_config& c) { return c.num_actions + (c.policy == 2 ? c.num_chance_outcomes : 0); }

struct StepState {
  bool allocated = false, rooted = false;
  int32_t* node_visits = nullptr; float* raw_values = nullptr; float* node_values = nullptr;
  int32_t* parents = nullptr; int32_t* action_from_parent = nullptr;
  int32_t* children_index = nullptr; float* children_prior_logits = nullptr;
  float* children_prior_probs = nullptr; float* children_values = nullptr;
  int32_t* children_visits = nullptr; float* children_rewards = nullptr;
  float* children_discounts = nullptr; float* embeddings = nullptr;
  uint8_t* root_invalid = nullptr;
  int32_t *sel_parent = nullptr, *sel_action = nullptr, *sel_depth = nullptr, *depth_sum = nullptr,
          *path = nullptr;
  uint32_t* sim_keys = nullptr;
  int32_t* xfer_node = nullptr;
  float* root_gumbel = nullptr;
  int32_t* visit_table = nullptr;
  void* slab = nullptr;

  // one slab, carved: the only allocation the handle ever makes
  hipError_t allocate(int B, int N, int A, int E, int table_words) {
    size_t BN = (size_t)B * N;
    size_t words = 5 * BN + 7 * BN * A + BN * E + 4 * (size_t)B + BN + 2 * (size_t)N + (size_t)B * A +
                   (size_t)table_words;
    words += (size_t)B;  // xfer_node
    size_t bytes = words * 4 + (size_t)B * A + 256;
    hipError_t e = hipMalloc(&slab, bytes);
    if (e != hipSuccess) return e;
    uint32_t* w = static_cast<uint32_t*>(slab);
    auto take = [&](size_t n) { uint32_t* p = w; w += n; return p; };
    node_visits = (int32_t*)take(BN); raw_values = (float*)take(BN); node_values = (float*)take(BN);
    parents = (int32_t*)take(BN); action_from_parent = (int32_t*)take(BN);
    children_index = (int32_t*)take(BN * A); children_prior_logits = (float*)take(BN * A);
    children_prior_probs = (float*)take(BN * A); children_values = (float*)take(BN * A);
    children_visits = (int32_t*)take(BN * A); children_rewards = (float*)take(BN * A);
    children_discounts = (float*)take(BN * A); embeddings = (float*)take(BN * E);
    sel_parent = (int32_t*)take(B); sel_action = (int32_t*)take(B); sel_depth = (int32_t*)take(B);
    depth_sum = (int32_t*)take(B); path = (int32_t*)take(BN); sim_keys = take(2 * (size_t)N);
    xfer_node = (int32_t*)take(B);
    root_gumbel = (float*)take((size_t)B * A); visit_table = (int32_t*)take(table_words);
    root_invalid = reinterpret_cast<uint8_t*>(w);
    allocated = true;
    return hipSuccess;
  }
  void release() {
    if (slab) hipFree(slab);
    slab = nullptr;
    allocated = rooted = false;
  }
  StepArgs args(const mzs_config& c) const {
    StepArgs a;
    a.B = c.batch; a.N = c.num_simulations + 1; a.AD = c.num_actions; a.E = c.embed_dim;
    a.A = slots_per_node(c);
    a.S = c.num_simulations; a.max_depth = c.max_depth > 0 ? c.max_depth : c.num_simulations;
    a.tiebreak = c.tiebreak; a.pb_c_init = c.pb_c_init; a.pb_c_base = c.pb_c_base;
    a.global_batch = (uint64_t)c.global_batch; a.root_offset = (uint64_t)c.root_offset;
    a.node_visits = node_visits; a.raw_values = raw_values; a.node_values = node_values;
    a.parents = parents; a.action_from_parent = action_from_parent;
    a.children_index = children_index; a.children_prior_logits = children_prior_logits;
    a.children_prior_probs = children_prior_probs; a.children_values = children_values;
    a.children_visits = children_visits; a.children_rewards = children_rewards;
    a.children_discounts = children_discounts; a.embeddings = embeddings;
    a.root_invalid = root_invalid;
    a.sel_parent = sel_parent; a.sel_action = sel_action; a.sel_depth = sel_depth;
    a.depth_sum = depth_sum; a.path = path; a.sim_keys = sim_keys;
    a.xfer_node = xfer_node; a.wide = c.embed_dim >= kWideEmb ? 1 : 0;
    a.qtransform = c.qtransform; a.max_considered = c.max_num_considered_actions;
    a.gumbel_scale = c.gumbel_scale; a.root_gumbel = root_gumbel; a.visit_table = visit_table;
    return a;
  }
};

// canonical softmax over a row-distributed vector with run-time length A
MZ_DEV void row_softmax_rt(const float (&x)[kMaxAS], int A, int j, float (&p)[kMaxAS]) {
  float m = -INFINITY;
#pragma unroll
  for (int t = 0; t < kMaxAS; ++t) m = (j + 16 * t < A) ? fmaxf(m, x[t]) : m;
  m = row_max<4>(m);
  float e[kMaxAS];
  float part = 0.0f;
#pragma unroll
  for (int t = 0; t < kMaxAS; ++t) {
    bool ok = j + 16 * t < A;
    e[t] = ok ? exp_neg(x[t] - m) : 0.0f;
    part = (t == 0) ? e[0] : (ok ? part + e[t] : part);
  }
  float s = row_sum(part);
#pragma unroll
  for (int t = 0; t < kMaxAS; ++t) p[t] = e[t] / s;
}

// canonical 16-wide sum of a row-distributed vector with run-time length
MZ_DEV float row_sum_rt(const float (&x)[kMaxAS], int A, int j) {
  float part = 0.0f;
#pragma unroll
  for (int t = 0; t < kMaxAS; ++t) {
    bool ok = j + 16 * t < A;
    part = (t == 0) ? (ok ? x[0] : 0.0f) : (ok ? part + x[t] : part);
  }
  return row_sum(part);
}

// mctx qtransforms for one node, row-distributed (kind 0: by_parent_and_siblings, 1: completed_by_mix_value)
MZ_DEV void row_qtransform(const StepArgs& s, size_t rb, int node, int A, int j, float (&out)[kMaxAS],
                           int (&vc)[kMaxAS], float (&logits)[kMaxAS], int& sum_visits) {
  const size_t nb = (rb + node) * A;
  float q[kMaxAS];
  int part = 0, mxv = 0;
#pragma unroll
  for (int t = 0; t < kMaxAS; ++t) {
    int a = j + 16 * t;
    bool ok = a < A;
    size_t o = nb + (ok ? a : 0);
    vc[t] = ok ? s.children_visits[o] : 0;
    logits[t] = ok ? s.children_prior_logits[o] : 0.0f;
    q[t] = s.children_rewards[o] + s.children_discounts[o] * s.children_values[o];
    part += vc[t];
    mxv = max(mxv, vc[t]);
  }
  sum_visits = row_sum_i(part);
  if (s.qtransform == 0) {
    float nval = s.node_values[rb + node];
    float lo = nval, hi = nval;
#pragma unroll
    for (int t = 0; t < kMaxAS; ++t) {
      float safe = (j + 16 * t < A && vc[t] > 0) ? q[t] : nval;
      lo = fminf(lo, safe);
      hi = fmaxf(hi, safe);
    }
    lo = row_min<4>(lo);
    hi = row_max<4>(hi);
    float span = fmaxf(hi - lo, 1e-8f);
#pragma unroll
    for (int t = 0; t < kMaxAS; ++t) out[t] = ((vc[t] > 0 ? q[t] : lo) - lo) / span;
    return;
  }
  float maxvisit = (float)row_max_i(mxv);
  float prior[kMaxAS], tmp[kMaxAS];
  row_softmax_rt(logits, A, j, prior);
#pragma unroll
  for (int t = 0; t < kMaxAS; ++t) {
    prior[t] = fmaxf(prior[t], kFltTiny);
    tmp[t] = vc[t] > 0 ? prior[t] : 0.0f;
  }
  float sum_probs = row_sum_rt(tmp, A, j);
#pragma unroll
  for (int t = 0; t < kMaxAS; ++t) tmp[t] = vc[t] > 0 ? (prior[t] * q[t]) / sum_probs : 0.0f;
  float weighted_q = row_sum_rt(tmp, A, j);
  float value = (s.raw_values[rb + node] + (float)sum_visits * weighted_q) / (float)(sum_visits + 1);
  float lo = INFINITY, hi = -INFINITY;
#pragma unroll
  for (int t = 0; t < kMaxAS; ++t) {
    out[t] = vc[t] > 0 ? q[t] : value;
    bool ok = j + 16 * t < A;
    lo = ok ? fminf(lo, out[t]) : lo;
    hi = ok ? fmaxf(hi, out[t]) : hi;
  }
  lo = row_min<4>(lo);
  hi = row_max<4>(hi);
  float span = fmaxf(hi - lo, 1e-8f);
  float scale = (50.0f + maxvisit) * 0.1f;
#pragma unroll
  for (int t = 0; t < kMaxAS; ++t) out[t] = scale * ((out[t] - lo) / span);
}

// seq_halving.score_considered + masked_argmax over a row-distributed action set
MZ_DEV int row_gumbel_argmax(const StepArgs& s, int r, int A, int j, int considered_visit,
                             const float (&logits)[kMaxAS], const float (&qv)[kMaxAS], const int (&vc)[kMaxAS],
                             int (&cidx)[kMaxAS], int& next) {
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < kMaxAS; ++t) mx = (j + 16 * t < A) ? fmaxf(mx, logits[t]) : mx;
  mx = row_max<4>(mx);
  float bscore = -INFINITY;
  int best = 1 << 20, bnext = -1;
#pragma unroll
  for (int t = 0; t < kMaxAS; ++t) {
    int a = j + 16 * t;
    bool ok = a < A;
    float g = ok ? s.root_gumbel[(size_t)r * A + a] : 0.0f;
    float sc = (g + (logits[t] - mx)) + qv[t];
    sc = fmaxf(sc, -1e9f);
    sc = sc + (vc[t] == considered_visit ? 0.0f : -INFINITY);
    if (ok && s.root_invalid[(size_t)r * A + a]) sc = -INFINITY;
    if (!ok) sc = -INFINITY;
    bool take = (t == 0) || (sc > bscore);
    if (take) { bscore = sc; best = ok ? a : (1 << 20); bnext = cidx[t]; }
  }
  row_argmax<4>(bscore, best, bnext);
  next = bnext;
  return best;
}

// the cached decisions of mz_step_jump.cuh (all null in a handle whose tree is walked level by level)
struct JumpArgs {
  int32_t* jump_pa;     // [B][N]  parent | action << 16 | near tie << 31
  int32_t* jump_lv;     // [B][N]  level of `parent` (edges from the root)
  int32_t* node_depth;  // [B][N]  length of the node's own root path
  uint32_t* node_path;  // [B][N][N]  entry e = node at level e | action taken there << 16
};

// The statistics of ONE root's tree that the per-simulation step both reads and rewrites (the MuZero policy's decisions:
// children_{index, visits, prior_probs, rewards, values}, node_{visits, values}, the JUMP records), as pointers to the
// root's own rows.  The step-wise kernels point them at the HBM tree (tree_view_global).  The one-launch ResNet search
// (mz_search_conv.hip) keeps them in the CU's LDS for the whole search when they fit (round 6): between two tree steps
// of a root its XCD streams 5.7 MB of convolution weights through a 4 MB L2, so every tree step used to find its ~260
// cache lines evicted -- 4.5 of the 7 us of a 44-level decision refresh were memory round trips, not arithmetic.
struct TreeView {
  int* cidx; int* cvis; float* prob; float* rew; float* val;  // [N][A], element (node, a) at [(node * A + a) * cs]
  float* dis;    // [N][A] children_discounts, or nullptr: `disc` on every edge (an unexpanded child's value is +0, so
  float disc;    // rew + disc * val is the same +0 as with the array's 0 there)
  int* nvis; float* nval;  // [N], element `node` at [node * ns]
  int* jpa; int* jlv;      // [N]
  // word strides: 1 / 1 for the HBM tree's separate arrays; the LDS copy interleaves the five words of a child and the
  // four of a node (cs = 5, ns = 4): one address per (node, action), its fields at immediate offsets (ds_read2_b32)
  int cs, ns;
  // root_invalid_actions of this lane's actions (bit t: action j + 16 t), read once by a caller that lives for a whole
  // search; -1: level_load reads s.root_invalid whenever it meets the root (a global round trip in front of the scores)
  int inv_bits;
};
// the HBM tree of a handle without JUMP arrays (the walking kernels): no records to point at
MZ_DEV TreeView tree_view_global(const StepArgs& s, size_t rb) {
  const size_t o = rb * (size_t)s.A;
  TreeView T;
  T.cidx = s.children_index + o; T.cvis = s.children_visits + o; T.prob = s.children_prior_probs + o;
  T.rew = s.children_rewards + o; T.val = s.children_values + o; T.dis = s.children_discounts + o; T.disc = 0.0f;
  T.nvis = s.node_visits + rb; T.nval = s.node_values + rb; T.jpa = nullptr; T.jlv = nullptr;
  T.cs = 1; T.ns = 1; T.inv_bits = -1;
  return T;
}
MZ_DEV TreeView tree_view_global(const StepArgs& s, const JumpArgs& g, size_t rb) {
  TreeView T = tree_view_global(s, rb);
  T.jpa = g.jump_pa + rb; T.jlv = g.jump_lv + rb;
  return T;
}

// pUCT scores of all children of `node` (muzero_action_selection with qtransform_by_parent_and_siblings),
// noise-free; first-max argmax; `near` = some other action is within the reach of the tie-break noise.
// Split into the loads and the arithmetic so that a row can put the loads of several levels in flight before it
// computes on the first (mzs_expand_backup refreshes up to kLevelsInFlight levels per row at once).
struct LevelIn {
  int cidx[kMaxAS], cvis[kMaxAS];
  float prob[kMaxAS], rew[kMaxAS], dis[kMaxAS], val[kMaxAS];
  int nvis, inv;  // inv: bit t = action j + 16 t is invalid at the root
  float nval;
};
// AS: 0 = any action count up to 16 kMaxAS (every 16-lane slot behind a run-time test), else the number of slots the
// caller's action count fills (16 (AS - 1) < A <= 16 AS): the same operations without the dead slots' branches
template <int AS = 0>
MZ_DEV void level_load(const StepArgs& s, const TreeView& T, int r, int node, int j, LevelIn& L) {
  const int A = s.A;
  const int nb = node * A;
  L.nvis = T.nvis[node * T.ns];
  L.nval = T.nval[node * T.ns];
  L.inv = 0;
#pragma unroll
  for (int t = 0; t < (AS ? AS : kMaxAS); ++t) {
    const int a = j + 16 * t;
    const bool ok = a < A;
    L.cidx[t] = -1; L.cvis[t] = 0; L.prob[t] = 0.0f; L.rew[t] = 0.0f; L.dis[t] = 0.0f; L.val[t] = 0.0f;
    if (AS || 16 * t < A) {
      const int o = nb + (ok ? a : 0);
      L.cidx[t] = T.cidx[o * T.cs];
      L.cvis[t] = T.cvis[o * T.cs];
      L.prob[t] = T.prob[o * T.cs];
      L.rew[t] = T.rew[o * T.cs];
      L.dis[t] = T.dis ? T.dis[o * T.cs] : T.disc;
      L.val[t] = T.val[o * T.cs];
      if (T.inv_bits < 0 && node == 0 && ok && s.root_invalid[(size_t)r * A + a]) L.inv |= 1 << t;  // the root is level 0 only
    }
  }
  if (T.inv_bits >= 0 && node == 0) L.inv = T.inv_bits;
}
// `tbl` (optional, LDS): {sqrt(n) pb_c(n), RN(1 / n)} for n = 0 .. S + 1, built once per launch by a kernel that lives
// for a whole search (mz_search_conv.hip) -- the same puct_scale() values, and x / n by Markstein's exact sequence for
// n <= 1030 (div_small, mz_fused.cuh; tests/test_oracle_kat.py): the refresh of a path's decisions is arithmetic-bound,
// a log, a sqrt and three of its four IEEE divisions per level go
// TBL: `tbl` is there (the caller's launch built it): no code for the other case
template <int AS = 0, bool TBL = false>
MZ_DEV void level_compute(const StepArgs& s, int j, const LevelIn& L, float (&sc)[kMaxAS], int& best, int& child,
                          bool& near, const float* tbl = nullptr) {
  constexpr int NSLOT = AS ? AS : kMaxAS;
  const int A = s.A;
  const float nval = L.nval;
  const float tn = (TBL || tbl) ? tbl[2 * L.nvis] : puct_scale(L.nvis, s.pb_c_init, s.pb_c_base);
  float q[kMaxAS];
  float lo = nval, hi = nval;
#pragma unroll
  for (int t = 0; t < NSLOT; ++t) {
    const bool ok = j + 16 * t < A;
    q[t] = 0.0f;
    if (AS || 16 * t < A) {
      q[t] = L.rew[t] + L.dis[t] * L.val[t];
      const float safe = (ok && L.cvis[t] > 0) ? q[t] : nval;
      lo = fminf(lo, safe);
      hi = fmaxf(hi, safe);
    }
  }
  lo = row_min<4>(lo);
  hi = row_max<4>(hi);
  const float span = fmaxf(hi - lo, 1e-8f);
  float bscore = -INFINITY;
  best = 1 << 20;
  child = -1;
  // two slots of actions: the lane's two value scores share their denominator -- ONE refined reciprocal and the
  // hardware's own quotient correction on the packed pair (div_newton2, mz_spec.cuh: the IEEE quotient while every
  // numerator is 0 or >= 2^-100 and the span is below 2^100; a wave-uniform test, the IEEE divisions otherwise) as in
  // the fused kernel's puct_scores: 12 instructions instead of 26
  [[maybe_unused]] f32x2 vs2 = splat2(0.0f);
  [[maybe_unused]] bool have_vs2 = false;
  if constexpr (AS == 2) {
    const float n0 = (L.cvis[0] > 0 ? q[0] : lo) - lo, n1 = (L.cvis[1] > 0 ? q[1] : lo) - lo;
    const uint32_t low = min(f2u(n0) - 1u, f2u(n1) - 1u);  // 0 wraps to the top: only (0, 2^-100) fails the test
    const bool risky = (low < f2u(0x1p-100f) - 1u) | !(span < 0x1p100f);
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(risky) == 0, 1)) {
      const float y0 = __builtin_amdgcn_rcpf(span);
      const float y = __builtin_fmaf(__builtin_fmaf(-span, y0, 1.0f), y0, y0);
      vs2 = div_newton2((f32x2){n0, n1}, splat2(span), splat2(y));
      have_vs2 = true;
    }
  }
#pragma unroll
  for (int t = 0; t < NSLOT; ++t) {
    const int a = j + 16 * t;
    const bool ok = a < A;
    sc[t] = -INFINITY;
    if (AS || 16 * t < A) {
      float value_score;
      if (AS == 2 && have_vs2) value_score = t == 0 ? vs2.x : vs2.y;
      else value_score = ((L.cvis[t] > 0 ? q[t] : lo) - lo) / span;
      float policy_score;
      if (TBL || tbl) {
        const float x = tn * L.prob[t], d = (float)(L.cvis[t] + 1), y = tbl[2 * (L.cvis[t] + 1) + 1];
        const float q0 = x * y;
        policy_score = __builtin_fmaf(__builtin_fmaf(-q0, d, x), y, q0);
      } else {
        policy_score = (tn * L.prob[t]) / (float)(L.cvis[t] + 1);
      }
      sc[t] = value_score + policy_score;
      if ((L.inv >> t) & 1) sc[t] = -INFINITY;
      if (!ok) sc[t] = -INFINITY;
    }
    const bool take = (t == 0) || (sc[t] > bscore);  // first max wins inside the lane
    if (take) { bscore = sc[t]; best = ok ? a : (1 << 20); child = L.cidx[t]; }
  }
  row_argmax<4>(bscore, best, child);
  bool unsafe = false;
  if (s.tiebreak) {
#pragma unroll
    for (int t = 0; t < NSLOT; ++t) {
      const int a = j + 16 * t;
      unsafe = unsafe | ((a < A) & (a != best) & !((sc[t] + 1e-7f) < bscore));
    }
  }
  near = ((__builtin_amdgcn_ballot_w64(unsafe) >> (threadIdx.x & 48)) & 0xffffull) != 0;  // any lane of the row
}
MZ_DEV void level_decide(const StepArgs& s, const TreeView& T, int r, int node, int j, float (&sc)[kMaxAS],
                         int (&cidx)[kMaxAS], int& best, int& child, bool& near) {
  LevelIn L;
  level_load(s, T, r, node, j, L);
  level_compute(s, j, L, sc, best, child, near);
#pragma unroll
  for (int t = 0; t < kMaxAS; ++t) cidx[t] = L.cidx[t];
}

// mctx gumbel_muzero_{root,interior}_action_selection at `node` (the root is only ever selected at level 0):
// deterministic in the node's statistics -- the root's sequential-halving table entry is indexed by its
// own visit sum, i.e. by the number of the NEXT simulation once the backup has run.
MZ_DEV void gumbel_decide(const StepArgs& s, size_t rb, int r, int node, int j, int& best, int& child) {
  const int A = s.A;
  const size_t nb = (rb + node) * A;
  float qv[kMaxAS], logits[kMaxAS];
  int vc[kMaxAS], cidx[kMaxAS], sum_visits;
  row_qtransform(s, rb, node, A, j, qv, vc, logits, sum_visits);
#pragma unroll
  for (int t = 0; t < kMaxAS; ++t) cidx[t] = s.children_index[nb + (j + 16 * t < A ? j + 16 * t : 0)];
  if (node == 0) {
    int ninv = 0;
#pragma unroll
    for (int t = 0; t < kMaxAS; ++t) ninv += (j + 16 * t < A && s.root_invalid[(size_t)r * A + j + 16 * t]) ? 1 : 0;
    const int num_valid = A - row_sum_i(ninv);
    const int num_considered = min(s.max_considered, num_valid);
    const int si = min(sum_visits, s.S - 1);
    const int considered_visit = s.visit_table[(size_t)num_considered * s.S + si];
    best = row_gumbel_argmax(s, r, A, j, considered_visit, logits, qv, vc, cidx, child);
  } else {
    float x[kMaxAS], p[kMaxAS];
#pragma unroll
    for (int t = 0; t < kMaxAS; ++t) x[t] = logits[t] + qv[t];
    row_softmax_rt(x, A, j, p);
    float bscore = -INFINITY;
    best = 1 << 20;
    child = -1;
#pragma unroll
    for (int t = 0; t < kMaxAS; ++t) {
      const int a = j + 16 * t;
      const bool ok = a < A;
      const float sc = ok ? p[t] - (float)vc[t] / (float)(1 + sum_visits) : -INFINITY;
      const bool take = (t == 0) || (sc > bscore);
      if (take) { bscore = sc; best = ok ? a : (1 << 20); child = cidx[t]; }
    }
    row_argmax<4>(bscore, best, child);
  }
}
// mctx stochastic_muzero_policy at a CHANCE node (odd depth): slot i scores p_i / (children_visits_i + 1) with p the node's
// stored prior probabilities (the softmax of [-inf x AD, chance_logits]: exact 0 on the AD action slots), an fp32
// division, no noise, first maximum -- the visits of a chance node follow its outcome distribution (D'Hondt)
MZ_DEV void chance_decide(const StepArgs& s, const TreeView& T, int node, int j, int& best, int& child) {
  const int A = s.A;
  const int nb = node * A;
  float bscore = -INFINITY;
  best = 1 << 20;
  child = -1;
#pragma unroll
  for (int t = 0; t < kMaxAS; ++t) {
    const int a = j + 16 * t;
    const bool ok = a < A;
    const int o = (nb + (ok ? a : 0)) * T.cs;
    const int ci = T.cidx[o];
    const float sc = ok ? T.prob[o] / (float)(T.cvis[o] + 1) : -INFINITY;
    const bool take = (t == 0) || (sc > bscore);  // first max wins inside the lane
    if (take) { bscore = sc; best = ok ? a : (1 << 20); child = ci; }
  }
  row_argmax<4>(bscore, best, child);
}
template <bool GUMBEL>
MZ_DEV void decide_any(const StepArgs& s, const TreeView& T, size_t rb, int r, int node, int j, int& best, int& child, bool& near) {
  if constexpr (GUMBEL) {
    gumbel_decide(s, rb, r, node, j, best, child);  // (the Gumbel policy's statistics stay in the HBM tree)
    near = false;
  } else {
    float sc[kMaxAS];
    int cidx[kMaxAS];
    level_decide(s, T, r, node, j, sc, cidx, best, child, near);
  }
}


// JAX's key chain of one simulation, walked lazily (only a near tie needs a key): the per-simulation root key, then
// rng_key, action_selection_key = split(rng_key) once per level.  (k0, k1): rng_key after `level` splits (-1: not
// started); (s0, s1): the action_selection_key of level `level - 1`.
struct SimKeys {
  uint32_t k0 = 0, k1 = 0, s0 = 0, s1 = 0;
  int level = -1;
};
MZ_DEV void sim_keys_advance(const StepArgs& s, int sim, int r, int j, SimKeys& K, int level) {
  if (K.level < 0) {
    const uint64_t rg = s.root_offset + (uint64_t)r;
    uint32_t x0, x1;
    bool second;
    bits_block(2 * s.global_batch, 2 * rg + (uint64_t)(j & 1), x0, x1, second);
    threefry2x32(s.sim_keys[2 * sim], s.sim_keys[2 * sim + 1], x0, x1);
    const uint32_t word = second ? x1 : x0;
    K.k0 = bcast_u<0>(word);
    K.k1 = bcast_u<1>(word);
    K.level = 0;
  }
  while (K.level <= level) {
    uint32_t x0 = (uint32_t)(j & 1), x1 = 2u + (uint32_t)(j & 1);
    threefry2x32(K.k0, K.k1, x0, x1);
    K.k0 = bcast_u<0>(x0); K.k1 = bcast_u<1>(x0);
    K.s0 = bcast_u<0>(x1); K.s1 = bcast_u<1>(x1);
    K.level += 1;
  }
}

// mctx adds 1e-7 * uniform[0,1) to every score.  If fl(score_a + 1e-7) < best for every other action the argmax cannot
// depend on the draw (rounding is monotone): only a row that holds a near tie (level_compute's `near`) pays for the
// threefry blocks.  (-inf scores stay -inf with or without noise.)  This is that draw: the argmax of the row's noise-free
// scores `sc` plus the noise of the level's action_selection_key (s0, s1), and the winner's child index.
MZ_DEV void noisy_argmax(int A, int j, const float (&sc)[kMaxAS], const int (&cidx)[kMaxAS], uint32_t s0, uint32_t s1,
                         int& best, int& child) {
  const int NB = (A + 1) / 2;
  float bscore = -INFINITY;
  best = 1 << 20;
  child = -1;
#pragma unroll
  for (int t = 0; t < kMaxAS; ++t) {
    const int a = j + 16 * t;
    float score = sc[t];
    if (16 * t < A) {
      const int jb = a < NB ? a : a - NB;
      uint32_t x0 = (uint32_t)jb, x1 = (NB + jb < A) ? (uint32_t)(NB + jb) : 0u;
      threefry2x32(s0, s1, x0, x1);
      score = score + 1e-7f * uniform_from_bits(a < NB ? x0 : x1);
    }
    const bool take = (t == 0) || (score > bscore);
    if (take) { bscore = score; best = (a < A) ? a : (1 << 20); child = cidx[t]; }
  }
  row_argmax<4>(bscore, best, child);
}

// What simulate() hands to expand(): the selection record, by the row's (WG: the workgroup's) first lane, and the
// parent's embedding row into `parent_embedding_out` (nullptr: no gather -- a wide row moves by emb_xfer_kernel, or the
// caller reads the tree's row in place).  `xfer`: note the parent in xfer_node; `sel_out`: the record to every thread;
// `depth_acc`: the depth is added there (a register of the caller, who owns depth_sum[r] for the launch).
template <bool WG>
MZ_DEV void store_selection(const StepArgs& s, int r, int parent, int action, int depth, int32_t* action_out,
                            float* parent_embedding_out, bool xfer, int* sel_out = nullptr, int* depth_acc = nullptr) {
  const int j = threadIdx.x & 15;
  const int E = s.E;
  if (sel_out) { sel_out[0] = parent; sel_out[1] = action; sel_out[2] = depth; }
  if (WG ? threadIdx.x == 0 : j == 0) {
    s.sel_parent[r] = parent;
    s.sel_action[r] = action;
    s.sel_depth[r] = depth;
    if (depth_acc) *depth_acc += depth;
    else s.depth_sum[r] += depth;
    if (action_out) action_out[r] = action;
    if (xfer) s.xfer_node[r] = parent;
  }
  if (parent_embedding_out == nullptr) return;
  const float* src = s.embeddings + ((size_t)r * s.N + parent) * E;
  if (WG) {
    for (int i = threadIdx.x; i < E; i += blockDim.x) parent_embedding_out[(size_t)r * E + i] = src[i];
  } else {
    for (int i = j; i < E; i += 16) parent_embedding_out[(size_t)r * E + i] = src[i];
  }
}

// mctx _mask_invalid_actions + softmax over a row: where any lane of the row says `masked`, x - max(x) with the invalid
// actions at the lowest float; x holds what the softmax saw
MZ_DEV void row_mask_invalid(float (&x)[kMaxAS], const bool (&inv)[kMaxAS], bool masked, int A, int j) {
  if (((__builtin_amdgcn_ballot_w64(masked) >> (threadIdx.x & 48)) & 0xffffull) != 0) {  // any lane of the row
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < kMaxAS; ++t) mx = (j + 16 * t < A) ? fmaxf(mx, x[t]) : mx;
    mx = row_max<4>(mx);
#pragma unroll
    for (int t = 0; t < kMaxAS; ++t) x[t] = inv[t] ? kFltLowest : x[t] - mx;
  }
}
MZ_DEV void row_mask_invalid_softmax(float (&x)[kMaxAS], const bool (&inv)[kMaxAS], bool masked, int A, int j,
                                     float (&p)[kMaxAS]) {
  row_mask_invalid(x, inv, masked, A, j);
  row_softmax_rt(x, A, j, p);
}

// expansion of node `newn`: its prior row is the softmax of the net's logits (logits to the HBM tree, probabilities
// through the view); x: the row-distributed logits (slots past A: any finite value)
MZ_DEV void expand_prior_row(const StepArgs& s, const TreeView& T, size_t rb, int newn, const float (&x)[kMaxAS], int j) {
  const int A = s.A;
  float pr[kMaxAS];
  row_softmax_rt(x, A, j, pr);
#pragma unroll
  for (int t = 0; t < kMaxAS; ++t) {
    const int a = j + 16 * t;
    if (a < A) {
      s.children_prior_logits[(rb + newn) * A + a] = x[t];
      T.prob[(newn * A + a) * T.cs] = pr[t];
    }
  }
}
MZ_DEV void expand_prior_row(const StepArgs& s, const TreeView& T, size_t rb, int newn, const float* prior_logits_row, int j) {
  float x[kMaxAS];
#pragma unroll
  for (int t = 0; t < kMaxAS; ++t) {
    const int a = j + 16 * t;
    x[t] = a < s.A ? prior_logits_row[a] : 0.0f;
  }
  expand_prior_row(s, T, rb, newn, x, j);
}

}  // namespace mz
