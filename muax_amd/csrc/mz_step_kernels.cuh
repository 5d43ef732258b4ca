// mz_step_kernels.cuh -- every __global__ of the step-wise path, for mz_stepwise.hip alone (the unit that launches
// them): the WALKING kernels (step_*: mctx's level-by-level simulate() and a one-lane backward, for a tree of more than
// kJumpMaxNodes nodes, one over the slab budget, or MZS_STEP_WALK=1), the CACHED-DECISION kernels (jump_*: the bodies of
// mz_step_jump.cuh) and what both share (root, finish, wide embedding rows).  Both sets give the same bits: every
// per-node rule they apply is a device function of mz_step.cuh.
#pragma once
#include "mz_step_jump.cuh"

#pragma clang fp contract(off)

namespace mz {

// one 16-lane row per root
#define MZ_ROW_SETUP                                                  \
  const int lane = threadIdx.x & 63;                                  \
  const int j = lane & 15;                                            \
  const int r = blockIdx.x * (blockDim.x >> 4) + (threadIdx.x >> 4);  \
  if (r >= s.B) return;                                               \
  const int N = s.N, A = s.A, E = s.E;                                \
  const size_t rb = (size_t)r * N;                                    \
  (void)lane; (void)N; (void)A; (void)E;

// mctx instantiate_tree_from_root: the empty tree of root row rb, by the row's 16 lanes
MZ_DEV void root_clear_tree(const StepArgs& s, size_t rb, int j) {
  const int N = s.N, A = s.A, E = s.E;
  for (int n = j; n < N; n += 16) {
    s.node_visits[rb + n] = 0;
    s.raw_values[rb + n] = 0.0f;
    s.node_values[rb + n] = 0.0f;
    s.parents[rb + n] = -1;
    s.action_from_parent[rb + n] = -1;
  }
  for (int i = j; i < N * A; i += 16) {
    size_t o = rb * A + i;
    s.children_index[o] = -1;
    s.children_prior_logits[o] = 0.0f;
    s.children_prior_probs[o] = 0.0f;
    s.children_values[o] = 0.0f;
    s.children_visits[o] = 0;
    s.children_rewards[o] = 0.0f;
    s.children_discounts[o] = 0.0f;
  }
  if (!s.wide)  // (wide: zeroed by a memset on the stream)
    for (size_t i = j; i < (size_t)N * E; i += 16) s.embeddings[rb * E + i] = 0.0f;
}

// mctx instantiate_tree_from_root + the policy's prelude, for root row r.  The MuZero prelude (muzero_policy: Dirichlet
// mix, log, mask) runs over the row's first AD slots (prior_logits, invalid, noise: [B, AD]) and pads the slots AD..A with
// -inf logits and the invalid mark: AD < A is stochastic_muzero_policy's root (A - AD chance slots), AD == A pads nothing
// and IS the deterministic root -- same operations, same order.  The Gumbel prelude (AD == A) is a branch of its own.
// embedding: [B, es], es <= E, into a row that root_clear_tree zeroed.
MZ_DEV void root_row(const StepArgs& s, int r, int j, int AD, int es, const float* prior_logits, const float* value,
                     const float* embedding, const uint8_t* invalid, const float* noise, float fraction,
                     int gumbel_policy, const float* gumbel_in, uint32_t gk0, uint32_t gk1) {
  const int N = s.N, A = s.A, E = s.E;
  const size_t rb = (size_t)r * N;
  root_clear_tree(s, rb, j);
  float x[kMaxAS], pr[kMaxAS], lg[kMaxAS];
  bool inv[kMaxAS];
#pragma unroll
  for (int t = 0; t < kMaxAS; ++t) {
    int a = j + 16 * t;
    x[t] = a < AD ? prior_logits[(size_t)r * AD + a] : 0.0f;
    inv[t] = (invalid != nullptr && a < AD) ? invalid[(size_t)r * AD + a] != 0 : false;
    if (a < A) s.root_invalid[(size_t)r * A + a] = (a >= AD || inv[t]) ? 1 : 0;
  }
  bool any_invalid = false;
  if (!gumbel_policy) {
    // mctx muzero_policy prelude: Dirichlet mix, log
    row_softmax_rt(x, AD, j, pr);
    float keep = 1.0f - fraction;
#pragma unroll
    for (int t = 0; t < kMaxAS; ++t) {
      int a = j + 16 * t;
      float nz = (noise != nullptr && a < AD) ? noise[(size_t)r * AD + a] : 0.0f;
      float noisy = keep * pr[t] + fraction * nz;
      lg[t] = log_pos(fmaxf(noisy, kFltTiny));
    }
    any_invalid = invalid != nullptr;
  } else {
    // mctx gumbel_muzero_policy: the logits only pass through _mask_invalid_actions; root Gumbel noise
    const uint64_t rg = s.root_offset + (uint64_t)r;
#pragma unroll
    for (int t = 0; t < kMaxAS; ++t) {
      int a = j + 16 * t;
      lg[t] = x[t];
      any_invalid = any_invalid || inv[t];
      if (a < A) {
        float g;
        if (gumbel_in != nullptr) {
          g = gumbel_in[(size_t)r * A + a];
        } else {
          uint32_t x0, x1;
          bool second;
          bits_block(s.global_batch * (uint64_t)A, rg * (uint64_t)A + (uint64_t)a, x0, x1, second);
          threefry2x32(gk0, gk1, x0, x1);
          g = s.gumbel_scale * gumbel_from_bits(second ? x1 : x0);
        }
        s.root_gumbel[(size_t)r * A + a] = g;
      }
    }
  }
  row_mask_invalid(lg, inv, any_invalid, AD, j);
#pragma unroll
  for (int t = 0; t < kMaxAS; ++t) lg[t] = j + 16 * t < AD ? lg[t] : -INFINITY;
  float pq[kMaxAS];
  row_softmax_rt(lg, A, j, pq);
#pragma unroll
  for (int t = 0; t < kMaxAS; ++t) {
    int a = j + 16 * t;
    if (a < A) {
      s.children_prior_logits[rb * A + a] = lg[t];
      s.children_prior_probs[rb * A + a] = pq[t];
    }
  }
  if (s.wide) {
    if (j == 0) s.xfer_node[r] = 0;
  } else {
    for (int i = j; i < es; i += 16) s.embeddings[rb * E + i] = embedding[(size_t)r * es + i];
  }
  if (j == 0) {
    s.node_visits[rb] = 1;
    s.raw_values[rb] = value[r];
    s.node_values[rb] = value[r];
    s.depth_sum[r] = 0;
  }
}
__global__ __launch_bounds__(256) void step_root_kernel(StepArgs s, const float* prior_logits,
                                                         const float* value, const float* embedding,
                                                         const uint8_t* invalid, const float* noise,
                                                         float fraction, int gumbel_policy,
                                                         const float* gumbel_in, uint32_t gk0, uint32_t gk1) {
  MZ_ROW_SETUP
  root_row(s, r, j, A, E, prior_logits, value, embedding, invalid, noise, fraction, gumbel_policy, gumbel_in, gk0, gk1);
}
// ... with chance slots (stochastic policy): AD = s.AD actions, a state embedding of es floats
__global__ __launch_bounds__(256) void step_root_stochastic_kernel(StepArgs s, const float* prior_logits,
                                                                    const float* value, const float* embedding,
                                                                    int es, const uint8_t* invalid, const float* noise,
                                                                    float fraction) {
  MZ_ROW_SETUP
  root_row(s, r, j, s.AD, es, prior_logits, value, embedding, invalid, noise, fraction, 0, nullptr, 0, 0);
}

// mctx search.simulate, level by level from the root (+ the parent-embedding gather of search.expand): the decisions of
// mz_step.cuh on the HBM tree, the visited (node, action) pairs staged in `path` for the backward pass.  KIND 0: the MuZero
// rule at every node, 1: the Gumbel rules, 2 (stochastic): the MuZero rule at even depth, chance_decide at odd depth --
// `kind_out`: 1 where the selected edge leaves a decision node
template <int KIND>
MZ_DEV void walk_select(const StepArgs& s, int sim, int r, int j, int32_t* action_out, float* parent_embedding_out,
                        int32_t* kind_out = nullptr) {
  const size_t rb = (size_t)r * s.N;
  const TreeView T = tree_view_global(s, rb);
  SimKeys K;
  int node = 0, depth = 0, parent = 0, action = 0;
  for (;;) {
    int best, child;
    if constexpr (KIND == 1) {
      gumbel_decide(s, rb, r, node, j, best, child);
    } else if (KIND == 2 && (depth & 1)) {
      chance_decide(s, T, node, j, best, child);
    } else {
      float sc[kMaxAS];
      int cidx[kMaxAS];
      bool near;
      level_decide(s, T, r, node, j, sc, cidx, best, child, near);
      if (near) {  // (never without s.tiebreak)
        sim_keys_advance(s, sim, r, j, K, depth);
        noisy_argmax(s.A, j, sc, cidx, K.s0, K.s1, best, child);
      }
    }
    if (j == 0) s.path[rb + depth] = node | (best << 16);
    parent = node;
    action = best;
    depth += 1;
    if (child == -1 || depth >= s.max_depth) break;
    node = child;
  }
  store_selection<false>(s, r, parent, action, depth, action_out, s.wide ? nullptr : parent_embedding_out, s.wide != 0);
  if (KIND == 2 && j == 0) kind_out[r] = (depth & 1) ? 1 : 0;  // the parent sits at depth - 1
}
__global__ __launch_bounds__(256) void step_select_kernel(StepArgs s, int sim, int32_t* action_out,
                                                           float* parent_embedding_out) {
  MZ_ROW_SETUP
  walk_select<0>(s, sim, r, j, action_out, parent_embedding_out);
}
// ... with chance nodes at odd depth (stochastic policy)
__global__ __launch_bounds__(256) void step_select_stochastic_kernel(StepArgs s, int sim, int32_t* slot_out,
                                                                      int32_t* parent_is_decision_out,
                                                                      float* parent_embedding_out) {
  MZ_ROW_SETUP
  walk_select<2>(s, sim, r, j, slot_out, parent_embedding_out, parent_is_decision_out);
}
// ... with gumbel_muzero_{root,interior}_action_selection
__global__ __launch_bounds__(256) void step_select_gumbel_kernel(StepArgs s, int sim, int32_t* action_out,
                                                                  float* parent_embedding_out) {
  MZ_ROW_SETUP
  walk_select<1>(s, sim, r, j, action_out, parent_embedding_out);
}

// The one-lane half of an expansion: node `newn` and its edge (parent, action), then mctx search.backward along the path
// staged by walk_select (only this lane touches these words)
MZ_DEV void expand_edge_backward(const StepArgs& s, size_t rb, int parent, int action, int depth, int newn, float v,
                                 float rew_new, float dis_new) {
  const int A = s.A;
  const size_t eo = (rb + parent) * A + action;
  s.raw_values[rb + newn] = v;
  s.node_values[rb + newn] = v;
  s.node_visits[rb + newn] = s.node_visits[rb + newn] + 1;
  s.children_index[eo] = newn;
  s.children_rewards[eo] = rew_new;
  s.children_discounts[eo] = dis_new;
  s.parents[rb + newn] = parent;
  s.action_from_parent[rb + newn] = action;
  float leaf = v, childv = v;
  for (int d = depth - 1; d >= 0; --d) {
    int pk = s.path[rb + d];
    int pn = pk & 0xffff, pa = pk >> 16;
    size_t e2 = (rb + pn) * A + pa;
    int cnt = s.node_visits[rb + pn];
    float rw = (d == depth - 1) ? rew_new : s.children_rewards[e2];
    float ds = (d == depth - 1) ? dis_new : s.children_discounts[e2];
    leaf = rw + ds * leaf;
    float newv = (s.node_values[rb + pn] * (float)cnt + leaf) / ((float)cnt + 1.0f);
    s.node_values[rb + pn] = newv;
    s.node_visits[rb + pn] = cnt + 1;
    s.children_values[e2] = childv;
    s.children_visits[e2] = s.children_visits[e2] + 1;
    childv = newv;
  }
}

// What an expansion of row r starts from: the record the selection left and the node it fills -- the edge's child where
// one exists (re-expansion under max_depth), else node sim + 1
struct Expansion { int parent, action, depth, newn; };
MZ_DEV Expansion expansion_of(const StepArgs& s, size_t rb, int r, int sim) {
  const int parent = s.sel_parent[r], action = s.sel_action[r], depth = s.sel_depth[r];
  const int next = s.children_index[(rb + parent) * s.A + action];
  return {parent, action, depth, next == -1 ? sim + 1 : next};
}
// ... and its embedding row: the w <= E floats of `row`, zero-padded to E (a wide row moves by emb_xfer_kernel)
MZ_DEV void expand_embedding(const StepArgs& s, size_t rb, int r, int j, int newn, const float* row, int w) {
  const int E = s.E;
  if (s.wide) {
    if (j == 0) s.xfer_node[r] = newn;
  } else {
    for (int i = j; i < E; i += 16) s.embeddings[(rb + newn) * E + i] = i < w ? row[i] : 0.0f;
  }
}

// mctx search.expand (update_tree_node + edge) and search.backward
__global__ __launch_bounds__(256) void step_expand_backup_kernel(StepArgs s, int sim, const float* reward,
                                                                  const float* discount,
                                                                  const float* prior_logits,
                                                                  const float* value,
                                                                  const float* next_embedding) {
  MZ_ROW_SETUP
  const Expansion x = expansion_of(s, rb, r, sim);
  const float v = value[r];
  expand_prior_row(s, tree_view_global(s, rb), rb, x.newn, prior_logits + (size_t)r * A, j);
  expand_embedding(s, rb, r, j, x.newn, next_embedding + (size_t)r * E, E);
  const float rew_new = reward[r], dis_new = discount[r];
  if (j == 0) expand_edge_backward(s, rb, x.parent, x.action, x.depth, x.newn, v, rew_new, dis_new);
}

// mctx stochastic_muzero_policy's expansion: both functions' outputs arrive for every root and the row takes the set of
// its parent's kind, merged here (no per-simulation torch op): a decision parent (the selection's depth - 1 even) gets a
// chance child -- prior row [-inf x AD, chance_logits], afterstate value, edge reward 0 and discount 1, the afterstate
// embedding --, a chance parent a decision child -- [action_logits, -inf x C] and the chance function's value, reward,
// discount and state embedding.  Embedding rows are zero-padded to E.
struct StochasticOutputs {
  const float *chance_logits, *afterstate_value, *afterstate_embedding;      // [B, C] [B] [B, ea]
  const float *action_logits, *value, *reward, *discount, *state_embedding;  // [B, AD] [B] [B] [B] [B, es]
  int32_t ea, es;
};
__global__ __launch_bounds__(256) void step_expand_backup_stochastic_kernel(StepArgs s, int sim, StochasticOutputs o) {
  MZ_ROW_SETUP
  const int AD = s.AD, C = A - AD;
  const Expansion n = expansion_of(s, rb, r, sim);
  const bool chance_child = ((n.depth - 1) & 1) == 0;
  float x[kMaxAS];
#pragma unroll
  for (int t = 0; t < kMaxAS; ++t) {
    const int a = j + 16 * t;
    x[t] = -INFINITY;
    if (chance_child) {
      if (a >= AD && a < A) x[t] = o.chance_logits[(size_t)r * C + (a - AD)];
    } else {
      if (a < AD) x[t] = o.action_logits[(size_t)r * AD + a];
    }
  }
  expand_prior_row(s, tree_view_global(s, rb), rb, n.newn, x, j);
  expand_embedding(s, rb, r, j, n.newn,
                   chance_child ? o.afterstate_embedding + (size_t)r * o.ea : o.state_embedding + (size_t)r * o.es,
                   chance_child ? o.ea : o.es);
  if (j == 0) {
    const float v = chance_child ? o.afterstate_value[r] : o.value[r];
    const float rew = chance_child ? 0.0f : o.reward[r], dis = chance_child ? 1.0f : o.discount[r];
    expand_edge_backward(s, rb, n.parent, n.action, n.depth, n.newn, v, rew, dis);
  }
}

// what every policy's finish returns beside the action weights, by the row's first lane: the action, the root's value
// and the summed selection depths (both optional)
MZ_DEV void finish_store(const StepArgs& s, int r, int j, int best, int32_t* action_out, float* search_value_out,
                         int32_t* depth_sum_out) {
  if (j != 0) return;
  action_out[r] = best;
  if (search_value_out) search_value_out[r] = s.node_values[(size_t)r * s.N];
  if (depth_sum_out) depth_sum_out[r] = s.depth_sum[r];
}

// mctx Tree.summary + _apply_temperature + jax.random.categorical over the first A of the root's s.A slots (gumbel,
// action_weights_out: [B, A]; the drawn Gumbel row is that of shape [global_batch, A])
MZ_DEV void finish_row(const StepArgs& s, int r, int j, int A, float temperature, const float* gumbel, uint32_t ks0,
                       uint32_t ks1, int32_t* action_out, float* action_weights_out, float* search_value_out,
                       int32_t* depth_sum_out) {
  const size_t rb = (size_t)r * s.N;
  const uint64_t rg = s.root_offset + (uint64_t)r;
  int vc[kMaxAS];
  int part = 0;
#pragma unroll
  for (int t = 0; t < kMaxAS; ++t) {
    int a = j + 16 * t;
    vc[t] = a < A ? s.children_visits[rb * s.A + a] : 0;
    part += vc[t];
  }
  float total = (float)row_sum_i(part);
  float denom = fmaxf(total, 1.0f);
  float lg[kMaxAS], prob[kMaxAS];
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < kMaxAS; ++t) {
    int a = j + 16 * t;
    float p = (float)vc[t] / denom;
    p = total > 0.0f ? p : 1.0f / (float)A;
    prob[t] = p;
    lg[t] = log_pos(fmaxf(p, kFltTiny));
    mx = a < A ? fmaxf(mx, lg[t]) : mx;
  }
  mx = row_max<4>(mx);
  float tden = fmaxf(temperature, kFltTiny);
  float bscore = -INFINITY;
  int best = 1 << 20, dummy = 0;
#pragma unroll
  for (int t = 0; t < kMaxAS; ++t) {
    int a = j + 16 * t;
    bool ok = a < A;
    float g;
    if (gumbel != nullptr) {
      g = ok ? gumbel[(size_t)r * A + a] : 0.0f;
    } else {
      uint32_t x0, x1;
      bool second;
      bits_block(s.global_batch * (uint64_t)A, rg * (uint64_t)A + (uint64_t)(ok ? a : 0), x0, x1, second);
      threefry2x32(ks0, ks1, x0, x1);
      g = gumbel_from_bits(second ? x1 : x0);
    }
    float score = ok ? (lg[t] - mx) / tden + g : -INFINITY;
    if (ok) action_weights_out[(size_t)r * A + a] = prob[t];
    bool take = (t == 0) || (ok && score > bscore);
    if (take) { bscore = score; best = ok ? a : (1 << 20); }
  }
  row_argmax<4>(bscore, best, dummy);
  finish_store(s, r, j, best, action_out, search_value_out, depth_sum_out);
}
__global__ __launch_bounds__(256) void step_finish_kernel(StepArgs s, float temperature, const float* gumbel,
                                                           uint32_t ks0, uint32_t ks1, int32_t* action_out,
                                                           float* action_weights_out, float* search_value_out,
                                                           int32_t* depth_sum_out) {
  MZ_ROW_SETUP
  finish_row(s, r, j, A, temperature, gumbel, ks0, ks1, action_out, action_weights_out, search_value_out, depth_sum_out);
}
// ... over the decision slots of a stochastic tree (mctx _mask_tree(tree, num_actions, 'decision'))
__global__ __launch_bounds__(256) void step_finish_stochastic_kernel(StepArgs s, float temperature, const float* gumbel,
                                                                      uint32_t ks0, uint32_t ks1, int32_t* action_out,
                                                                      float* action_weights_out, float* search_value_out,
                                                                      int32_t* depth_sum_out) {
  MZ_ROW_SETUP
  finish_row(s, r, j, s.AD, temperature, gumbel, ks0, ks1, action_out, action_weights_out, search_value_out, depth_sum_out);
}

// tail of mctx gumbel_muzero_policy: best considered action + completed-Q policy target
__global__ __launch_bounds__(256) void step_finish_gumbel_kernel(StepArgs s, int32_t* action_out,
                                                                  float* action_weights_out,
                                                                  float* search_value_out, int32_t* depth_sum_out) {
  MZ_ROW_SETUP
  float qv[kMaxAS], logits[kMaxAS];
  int vc[kMaxAS], cidx[kMaxAS] = {0, 0, 0, 0}, sum_visits, next;
  row_qtransform(s, rb, 0, A, j, qv, vc, logits, sum_visits);
  int mxv = 0;
  bool inv[kMaxAS], any_inv = false;
#pragma unroll
  for (int t = 0; t < kMaxAS; ++t) {
    mxv = max(mxv, vc[t]);
    inv[t] = j + 16 * t < A && s.root_invalid[(size_t)r * A + j + 16 * t];
    any_inv = any_inv || inv[t];
  }
  const int considered_visit = row_max_i(mxv);
  const int best = row_gumbel_argmax(s, r, A, j, considered_visit, logits, qv, vc, cidx, next);
  float x[kMaxAS], w[kMaxAS];
#pragma unroll
  for (int t = 0; t < kMaxAS; ++t) x[t] = logits[t] + qv[t];
  row_mask_invalid_softmax(x, inv, any_inv, A, j, w);
#pragma unroll
  for (int t = 0; t < kMaxAS; ++t)
    if (j + 16 * t < A) action_weights_out[(size_t)r * A + j + 16 * t] = w[t];
  finish_store(s, r, j, best, action_out, search_value_out, depth_sum_out);
}

// ---- wide embedding rows: one workgroup per (root, KiB of the row) ----
// dir 0: rows[b] <- tree.embeddings[b][xfer_node[b]]   (parent embedding for recurrent_fn)
// dir 1: tree.embeddings[b][xfer_node[b]] <- rows[b]   (root / next embedding)
__global__ __launch_bounds__(256) void emb_xfer_kernel(const StepArgs s, float* rows, int dir) {
  const int b = blockIdx.x;
  const size_t E = (size_t)s.E;
  float* node = s.embeddings + ((size_t)b * s.N + s.xfer_node[b]) * E;
  float* row = rows + (size_t)b * E;
  const size_t i0 = (size_t)blockIdx.y * 1024, i1 = i0 + 1024 < E ? i0 + 1024 : E;
  if (dir == 0)
    for (size_t i = i0 + threadIdx.x; i < i1; i += 256) row[i] = node[i];
  else
    for (size_t i = i0 + threadIdx.x; i < i1; i += 256) node[i] = row[i];
}

// root decision (after step_root_kernel): one row per root
template <bool GUMBEL>
__global__ __launch_bounds__(256) void jump_root_kernel(StepArgs s, JumpArgs g) {
  MZ_ROW_SETUP
  int best, child;
  bool near;
  decide_any<GUMBEL>(s, tree_view_global(s, g, rb), rb, r, 0, j, best, child, near);
  if (j == 0) {
    g.jump_pa[rb] = best << 16 | (near ? (int)0x80000000 : 0);
    g.jump_lv[rb] = 0;
    g.node_depth[rb] = 0;
  }
}

// WIDE: one 256-thread workgroup per root (wide embedding rows), else one row per root
template <bool WIDE>
__global__ __launch_bounds__(256) void jump_select_kernel(StepArgs s, JumpArgs g, int sim, int32_t* action_out,
                                                           float* parent_embedding_out) {
  const int r = WIDE ? (int)blockIdx.x : (int)(blockIdx.x * (blockDim.x >> 4) + (threadIdx.x >> 4));
  if (r >= s.B) return;
  jump_select_body<WIDE>(s, g, tree_view_global(s, g, (size_t)r * s.N), sim, r, action_out, parent_embedding_out);
}

// mctx search.expand + search.backward + refresh of the decisions on the path, on a workgroup of its own per root
template <bool GUMBEL>
__global__ __launch_bounds__(1024) void jump_expand_backup_kernel(StepArgs s, JumpArgs g, int sim, const float* reward,
                                                                  const float* discount, const float* prior_logits,
                                                                  const float* value, const float* next_embedding,
                                                                  int32_t* next_action_out,
                                                                  float* next_parent_embedding_out) {
  extern __shared__ int lds_i[];
  const int r = blockIdx.x;
  jump_expand_backup_body<GUMBEL>(s, g, tree_view_global(s, g, (size_t)r * s.N), sim, r, lds_i, reward[r], discount[r], prior_logits + (size_t)r * s.A, value[r],
                                  next_embedding + (size_t)r * s.E, next_action_out != nullptr, next_action_out,
                                  next_parent_embedding_out);
}

#undef MZ_ROW_SETUP

}  // namespace mz
