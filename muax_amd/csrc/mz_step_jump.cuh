// mz_step_jump.cuh -- step-wise MuZero search with cached decisions (the fused kernel's scheme) on the
// HBM-resident tree of mz_step.cuh.  Same C-ABI entry points (mzs_root / mzs_select / mzs_expand_backup),
// same arithmetic per node, same results bit for bit; what changes is WHERE the per-level work happens:
//
//   * mctx's simulate() walks the tree level by level, a chain of dependent decisions.  Here every node
//     carries a JUMP record: the end point (parent, action, level) of the greedy, noise-free descent below
//     it, stopped early at the first node whose argmax is a near tie (fl(score + 1e-7) !< best for some
//     other action: only there can mctx's 1e-7 * uniform tie-break noise matter).  Sub-trees off a
//     backed-up path never change, so their records stay valid.  mzs_select reads the root's record: O(1),
//     plus one exact noisy evaluation per near tie (JAX's key chain is walked lazily down to that level);
//   * the decisions of the nodes ON the backed-up path are refreshed by mzs_expand_backup, where the path
//     is known up front: one workgroup per root, one 16-lane row per LEVEL (lanes over the actions), 16
//     levels in flight, all their loads independent.  The discounted-return chain is the only sequential
//     part and runs over LDS.
//
// Every node stores its own root path (written once at expansion: parent's path + one entry), so the
// backup finds its levels without a pointer chase.  Used (both policies) when N <= kJumpMaxNodes and B N^2
// words fit the budget; otherwise the walking kernels run.  Device functions only: the bodies below are also the tree
// step of the one-launch searches (mz_search_conv.hip, mz_mlp_generic.cuh); their kernels are in mz_step_kernels.cuh.
#pragma once
#include "mz_step.cuh"

#pragma clang fp contract(off)

namespace mz {

constexpr int kJumpMaxNodes = 1024;

// opt-in phase timers of the expand / backward / refresh body (tools/profile_search.py builds with -DMZ_PROFILE)
#ifdef MZ_PROFILE
__device__ unsigned long long g_jump_prof[1024 * 8];
#define MZ_JT_BEGIN unsigned long long jt_last = __builtin_amdgcn_s_memtime();
#define MZ_JT(k)                                                             \
  if (threadIdx.x == 0) {                                                    \
    const unsigned long long t_ = __builtin_amdgcn_s_memtime();              \
    g_jump_prof[(size_t)(blockIdx.x & 1023) * 8 + (k)] += t_ - jt_last;      \
    jt_last = t_;                                                            \
  }
#else
#define MZ_JT_BEGIN
#define MZ_JT(k)
#endif
constexpr int kLevelsInFlight = 3;  // levels of a backed-up path a 16-lane row refreshes at once (mzs_expand_backup)

// mctx search.simulate through the JUMP records, for root r.  WG: the calling workgroup belongs to this root alone
// -- every row repeats the (O(1)) selection, so every thread knows the parent and the whole workgroup gathers its
// embedding row (a separate transfer kernel costs its own 4.7 us minimum); otherwise one 16-lane row per root.
// jump_select_core: the decision alone -- every 16-lane row that calls it gets the same (parent, action, depth).
MZ_DEV void jump_select_core(const StepArgs& s, const JumpArgs& g, const TreeView& T, int sim, int r, int& parent, int& action,
                             int& depth) {
  const int lane = opaque_tid() & 63;
  const int j = lane & 15;
  const int N = s.N;
  const size_t rb = (size_t)r * N;
  SimKeys K;
  int jw = T.jpa[0], level = T.jlv[0];
  for (;;) {
    parent = jw & 0xffff;
    action = (jw >> 16) & 0xff;
    if (jw < 0 && level + 1 <= s.max_depth) {
      // near tie at `parent`: score + 1e-7 * uniform(action_selection_key of this level), as mctx
      sim_keys_advance(s, sim, r, j, K, level);
      float sc[kMaxAS];
      int cidx[kMaxAS], best, child;
      bool near;
      level_decide(s, T, r, parent, j, sc, cidx, best, child, near);
      noisy_argmax(s.A, j, sc, cidx, K.s0, K.s1, best, child);
      action = best;
      if (child >= 0 && level + 1 < s.max_depth) {
        jw = T.jpa[child * T.ns];
        level = T.jlv[child * T.ns];
        continue;
      }
    }
    break;
  }
  depth = level + 1;
  if (depth > s.max_depth) {
    // the cached descent overshoots max_depth: stop at level max_depth - 1 of the same path
    depth = s.max_depth;
    const uint32_t ent = g.node_path[(rb + parent) * N + depth - 1];
    parent = (int)(ent & 0xffffu);
    action = (int)(ent >> 16);
  }
}
// `parent_embedding_out` == nullptr: no gather (the caller reads the tree's embedding row in place)
template <bool WG>
MZ_DEV void jump_select_body(const StepArgs& s, const JumpArgs& g, const TreeView& T, int sim, int r, int32_t* action_out,
                             float* parent_embedding_out, int* sel_out = nullptr, int* depth_acc = nullptr) {
  int parent, action, depth;
  jump_select_core(s, g, T, sim, r, parent, action, depth);
  store_selection<WG>(s, r, parent, action, depth, action_out, parent_embedding_out, WG, sel_out, depth_acc);
}

// mctx search.expand + search.backward + refresh of the decisions on the path: one workgroup per root.
// `next_action_out` != null: the NEXT simulation's selection (simulate() of sim + 1: the root's fresh JUMP record is
// in this workgroup's hands) and the gather of its parent's embedding row run as the tail of this launch -- one launch
// and one kernel boundary fewer per simulation (mzs_expand_backup_select).
// The body is a device function of the calling workgroup (any multiple of 64 threads): the step-wise kernel runs
// it on a workgroup of its own, the fused ResNet search (mz_search_conv.hip) as the tail of the recurrent_fn pass of
// the same root.  `prior_logits_row`: the root's A logits; `next_embedding_row` == nullptr: the caller has written the
// new node's embedding row in place; `select_next`: also run simulate() of sim + 1 (sel_out[0..2] = its parent / action / depth
// in every thread; `next_parent_embedding_out` == nullptr: no gather).
// LDS of the body: per level e in [0, depth] (entry `depth` is the leaf), 15 arrays of N + 1 words
struct JumpLds {
  int *pn, *pa, *cnt;       // node at level e; action taken there (e < depth); node_visits before this backup
  float *val, *rw, *ds;     // node_values before this backup; reward / discount of edge e
  float *Gs, *nv;           // leaf_value arriving at level e; node value after this backup
  int *bst, *chd, *flg;     // refreshed decision, its child index, near tie
  int *cjp, *cjl;           // stored JUMP record of that child
  int *njp, *njl;           // new JUMP record of the level's node
  int *nxa, *nxb;           // pointer jumping (two buffers, in the backward pass's arrays, dead by then)
};
MZ_DEV JumpLds jump_lds(int* lds_i, int N) {
  const int D1 = N + 1;
  JumpLds L;
  L.pn = lds_i; L.pa = L.pn + D1; L.cnt = L.pa + D1;
  L.val = reinterpret_cast<float*>(L.cnt + D1); L.rw = L.val + D1; L.ds = L.rw + D1; L.Gs = L.ds + D1; L.nv = L.Gs + D1;
  L.bst = reinterpret_cast<int*>(L.nv + D1); L.chd = L.bst + D1; L.flg = L.chd + D1; L.cjp = L.flg + D1; L.cjl = L.cjp + D1;
  L.njp = L.cjl + D1; L.njl = L.njp + D1;
  L.nxa = L.cnt; L.nxb = reinterpret_cast<int*>(L.val);
  return L;
}
// The two pieces of the body that need nothing from recurrent_fn -- the fused search runs them while the root's
// convolution passes wait for their partner (mz_search_conv.hip); a barrier must separate them and follow the second.
// (1) path of the leaf: the parent's own root path + (parent, action); a fresh node gets its copy
MZ_DEV void jump_prefetch_path(const StepArgs& s, const JumpArgs& g, int r, const JumpLds& L, int tid, int nthr, int parent,
                               int action, int depth, int newn, bool fresh) {
  const int N = s.N;
  const size_t rb = (size_t)r * N;
  for (int e = tid; e < depth; e += nthr) {
    const uint32_t ent = (e < depth - 1) ? g.node_path[(rb + parent) * N + e] : ((uint32_t)parent | ((uint32_t)action << 16));
    L.pn[e] = (int)(ent & 0xffffu);
    L.pa[e] = (int)(ent >> 16);
    if (fresh) g.node_path[(rb + newn) * N + e] = ent;
  }
  if (tid == 0) {
    L.pn[depth] = newn;
    L.pa[depth] = 0;
    if (fresh) g.node_depth[rb + newn] = depth;
  }
}
// (2) per-level inputs of the backward pass (the last edge's reward / discount come from recurrent_fn: filled in later)
MZ_DEV void jump_prefetch_levels(const StepArgs& s, const TreeView& T, const JumpLds& L, int tid, int nthr, int depth) {
  for (int e = tid; e < depth; e += nthr) {
    const int e2 = L.pn[e] * s.A + L.pa[e];
    L.cnt[e] = T.nvis[(L.pn[e]) * T.ns];
    L.val[e] = T.nval[(L.pn[e]) * T.ns];
    L.rw[e] = (e == depth - 1) ? 0.0f : T.rew[e2 * T.cs];
    L.ds[e] = (e == depth - 1) ? 0.0f : (T.dis ? T.dis[e2 * T.cs] : T.disc);  // (levels above the last edge are expanded edges)
  }
}

// leaf_value = reward + discount * leaf_value, leaf to root (mctx search.backward): the one sequential chain of the step.
// One wavefront (`lane` = 0 .. 63 of the calling wavefront), 63 levels per chunk, every lane its own level: one step is
// X[e] = r[e] + d[e] * X[e + 1] on all lanes at once -- v_mul_f32_dpp wave_shl:1 + v_add_f32 -- and level e is final
// after (levels of the chunk - e) steps: ~25 cycles per level (round 3: two v_readlane + mul + add + select per level on
// the wave-uniform G, ~140 cycles as compiled; until round 6 a select per step, ~100).  The paths of a long search on few
// roots are 50 .. 150 levels deep and this chain paces the root.  Same operations in the same order for every level.
// `patch`: the last edge's (reward, discount) come from the caller's registers (rew_new, dis_new), not from rw / ds.
MZ_DEV void return_chain(const float* rw, const float* ds, float* Gs, float v, int depth, int lane, bool patch, float rew_new,
                         float dis_new) {
  float G = v;
  for (int c = (depth - 1) / 63; c >= 0; --c) {
    const int e = 63 * c + lane;
    const int cn = min(63, depth - 63 * c);
    const bool mine = lane < cn;
    // lanes past the chunk's levels run identity steps on the value arriving from below: (-0) + 1 * x == x for every x
    float rr = mine ? rw[e] : -0.0f, dd = mine ? ds[e] : 1.0f;
    if (patch && mine && e == depth - 1) {  // (`mine`: lane 63 of the chunk BELOW the last edge's has the same e)
      rr = rew_new;
      dd = dis_new;
    }
    float X = G, Xt = dd * G;  // (lane 63 has no lane above it: its Xt stays dd * G = G through every step)
    // four steps per statement: the DPP source X is the register the add before it has just written -- two wait
    // states (s_nop 1), which the hazard recogniser does not insert inside asm.  A level is final after (levels of
    // the chunk - e) steps and a further step maps it onto itself, so the count is rounded up to a multiple of four.
#define MZ_CSTEP "s_nop 1\n\tv_mul_f32_dpp %0, %1, %2 wave_shl:1 row_mask:0xf bank_mask:0xf\n\tv_add_f32 %1, %0, %3\n\t"
    for (int k = 0; k < cn; k += 4)
      asm volatile(MZ_CSTEP MZ_CSTEP MZ_CSTEP MZ_CSTEP : "+v"(Xt), "+v"(X) : "v"(dd), "v"(rr));
#undef MZ_CSTEP
    if (mine) Gs[e] = X;
    G = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(X)));  // arrival at the chunk's first level
  }
}

// `prefetched`: bit 0 = jump_prefetch_path, bit 1 = jump_prefetch_levels have run for this simulation (and a barrier since)
// AS: see level_load (0: any action count); `depth_acc` != nullptr: the next selection's depth is added there (a register
// of the caller, who owns depth_sum[r] for the launch) instead of to the HBM word -- a load-add-store round trip per
// simulation on the caller's critical path otherwise
// LDSB: every array the phases of this step hand to one another is in LDS (the LDS tree of the one-launch search): its
// barriers wait for the LDS queue only (s_waitcnt lgkmcnt(0); s_barrier) -- a __syncthreads() also drains vmcnt, i.e.
// waits for the acknowledgement of the write-only HBM stores (prior logits, parents, the selection ...) issued just before
template <bool LDSB>
MZ_DEV void step_barrier() {
  if constexpr (LDSB) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  else __syncthreads();
}
template <bool GUMBEL, int LIF = kLevelsInFlight, int AS = 0, bool TBL = false, bool LDSB = false>
MZ_DEV void jump_expand_backup_body(const StepArgs& s, const JumpArgs& g, const TreeView& T, int sim, int r, int* lds_i, float rew_new,
                                    float dis_new, const float* prior_logits_row, float v, const float* next_embedding_row,
                                    bool select_next, int32_t* next_action_out, float* next_parent_embedding_out,
                                    int* sel_out = nullptr, const int* known = nullptr, int prefetched = 0,
                                    const float* score_tbl = nullptr, int* depth_acc = nullptr) {
  const int tid = opaque_tid(), j = tid & 15, row = tid >> 4;
  MZ_JT_BEGIN
  const int nthr = blockDim.x, nrows = blockDim.x >> 4;  // 1024 / 256 threads (64 / 16 levels in flight) or one wavefront (4)
  const int N = s.N, A = s.A, E = s.E;
  const size_t rb = (size_t)r * N;
  // `known` = {parent, action, depth, new node} of this simulation when the caller has them in registers (the fused
  // search: two dependent memory round trips fewer on its critical path); an existing node has an index <= sim
  const int parent = known ? known[0] : s.sel_parent[r], action = known ? known[1] : s.sel_action[r];
  const int depth = known ? known[2] : s.sel_depth[r];
  const size_t eo = (rb + parent) * A + action;
  const int eol = parent * A + action;
  const int next = known ? (known[3] == sim + 1 ? -1 : known[3]) : T.cidx[eol * T.cs];
  __syncthreads();  // every thread has read the edge before row 0 rewrites it
  const bool fresh = next == -1;
  const int newn = fresh ? sim + 1 : next;
  const JumpLds JL = jump_lds(lds_i, N);
  int* const pn = JL.pn; int* const pa = JL.pa; int* const cnt = JL.cnt;
  float* const val = JL.val; float* const rw = JL.rw; float* const ds = JL.ds; float* const Gs = JL.Gs; float* const nv = JL.nv;
  int* const bst = JL.bst; int* const chd = JL.chd; int* const flg = JL.flg; int* const cjp = JL.cjp; int* const cjl = JL.cjl;
  int* const njp = JL.njp; int* const njl = JL.njl; int* const nxa = JL.nxa; int* const nxb = JL.nxb;

  // -- path of the leaf: the parent's own root path + (parent, action) --
  if (!(prefetched & 1)) jump_prefetch_path(s, g, r, JL, tid, nthr, parent, action, depth, newn, fresh);
  // the caller has prefetched the path AND the per-level inputs (the fused search, in idle convolution passes): the
  // discounted-return chain needs nothing else but (rew_new, dis_new, v), which are in registers -- it runs on the SECOND
  // wavefront right away, beside the expansion on the first (the new node's softmax, ~0.9 us), and the barrier between
  // the two phases goes
  const bool early_chain = prefetched == 3 && nthr >= 128;
  if (early_chain && (tid >> 6) == 1) return_chain(rw, ds, Gs, v, depth, tid & 63, true, rew_new, dis_new);
  // -- expand (row 0): prior of the new node, node and edge records --
  if (row == 0) {
    expand_prior_row(s, T, rb, newn, prior_logits_row, j);
    if (j == 0) {
      s.raw_values[rb + newn] = v;
      T.nval[newn * T.ns] = v;
      T.nvis[newn * T.ns] = T.nvis[newn * T.ns] + 1;
      T.cidx[eol * T.cs] = newn;
      T.rew[eol * T.cs] = rew_new;
      s.children_discounts[eo] = dis_new;  // (== T.dis[eol * T.cs] when the view is the HBM tree)
      s.parents[rb + newn] = parent;
      s.action_from_parent[rb + newn] = action;
      s.xfer_node[r] = newn;
    }
  }
  // (a whole workgroup per root: wide rows need no separate transfer kernel here)
  if (next_embedding_row != nullptr)
    for (int i = tid; i < E; i += nthr) s.embeddings[(rb + newn) * E + i] = next_embedding_row[i];
  step_barrier<LDSB>();
  MZ_JT(0)
  if (!early_chain) {
    // -- per-level inputs of the backward pass --
    if (!(prefetched & 2)) jump_prefetch_levels(s, T, JL, tid, nthr, depth);
    if (tid == (depth - 1) % nthr && depth > 0) {  // (the thread that wrote the entry, if it was written just now)
      rw[depth - 1] = rew_new;
      ds[depth - 1] = dis_new;
    }
    step_barrier<LDSB>();
    MZ_JT(1)
    if (tid < 64) return_chain(rw, ds, Gs, v, depth, tid, false, rew_new, dis_new);
    step_barrier<LDSB>();
  }
  MZ_JT(2)
  for (int e = tid; e <= depth; e += nthr)
    nv[e] = (e == depth) ? v : (val[e] * (float)cnt[e] + Gs[e]) / ((float)cnt[e] + 1.0f);
  step_barrier<LDSB>();
  for (int e = tid; e < depth; e += nthr) {
    const int e2 = pn[e] * A + pa[e];
    T.nval[(pn[e]) * T.ns] = nv[e];
    T.nvis[(pn[e]) * T.ns] = cnt[e] + 1;
    T.val[e2 * T.cs] = nv[e + 1];
    T.cvis[e2 * T.cs] = T.cvis[e2 * T.cs] + 1;
  }
  step_barrier<LDSB>();  // (workgroup-scope: the refreshed statistics are visible to every row below)
  MZ_JT(3)
  // -- decisions of the path nodes and the leaf: one row per level, LIF (kLevelsInFlight) levels per row at once (all
  // their loads are issued before the first is used: a deep path costs one memory round trip, not one per 64 levels) --
  for (int base = 0; base <= depth; base += nrows * LIF) {
    if constexpr (GUMBEL) {
      for (int u = 0; u < LIF; ++u) {
        const int e = base + u * nrows + row;
        if (e <= depth) {
          int best, child;
          bool near;
          decide_any<GUMBEL>(s, T, rb, r, pn[e], j, best, child, near);
          if (j == 0) {
            bst[e] = best;
            chd[e] = child;
            flg[e] = near ? 1 : 0;
            const bool off_path = child >= 0 && !(e < depth && child == pn[e + 1]);
            cjp[e] = off_path ? T.jpa[child * T.ns] : 0;
            cjl[e] = off_path ? T.jlv[child * T.ns] : 0;
          }
        }
      }
    } else {
      LevelIn L[LIF];
      int bestu[LIF], childu[LIF], cj[LIF], cl[LIF];
      bool nearu[LIF], offu[LIF];
#pragma unroll
      for (int u = 0; u < LIF; ++u) {
        const int e = base + u * nrows + row;
        level_load<AS>(s, T, r, pn[e <= depth ? e : depth], j, L[u]);
      }
#ifdef MZ_PROF_DECIDE
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      MZ_JT(7)
#endif
#pragma unroll
      for (int u = 0; u < LIF; ++u) {
        const int e = base + u * nrows + row;
        float sc[kMaxAS];
        level_compute<AS, TBL>(s, j, L[u], sc, bestu[u], childu[u], nearu[u], score_tbl);
        offu[u] = e <= depth && childu[u] >= 0 && !(e < depth && childu[u] == pn[e + 1]);
      }
#pragma unroll
      for (int u = 0; u < LIF; ++u) {  // the off-path children's stored records, all requested together
        cj[u] = offu[u] ? T.jpa[(childu[u]) * T.ns] : 0;
        cl[u] = offu[u] ? T.jlv[(childu[u]) * T.ns] : 0;
      }
#pragma unroll
      for (int u = 0; u < LIF; ++u) {
        const int e = base + u * nrows + row;
        if (e <= depth && j == 0) {
          bst[e] = bestu[u];
          chd[e] = childu[u];
          flg[e] = nearu[u] ? 1 : 0;
          cjp[e] = cj[u];
          cjl[e] = cl[u];
        }
      }
    }
  }
  step_barrier<LDSB>();
  MZ_JT(4)
  // -- JUMP records: a level takes its own end point (near tie, or an unexpanded best child), the stored record of
  // its off-path best child, or -- when its best child is the next level of this very path -- whatever that level
  // resolves to.  The bottom-up chain of the last case is resolved by pointer jumping (log2(depth) rounds over all
  // levels at once) instead of a serial walk by one thread; the leaf level never inherits, so every chain ends. --
  for (int e = tid; e <= depth; e += nthr) {
    const bool own = flg[e] || chd[e] < 0;
    const bool inherit = !own && e < depth && chd[e] == pn[e + 1];
    njp[e] = own ? (pn[e] | (bst[e] << 16) | (flg[e] ? (int)0x80000000 : 0)) : cjp[e];
    njl[e] = own ? e : cjl[e];
    nxa[e] = inherit ? e + 1 : e;
  }
  step_barrier<LDSB>();
  if (depth < 64) {
    // the whole path in one wavefront: lane e chases its pointer through ds_bpermute (a register exchange: no LDS
    // array, no barrier per round -- six rounds of ~100 cycles instead of six workgroup barriers)
    if (tid < 64) {
      const int e = tid <= depth ? tid : depth;
      int from = nxa[e];
      for (int span = 1; span <= depth; span <<= 1) from = __builtin_amdgcn_ds_bpermute(4 * from, from);
      if (tid <= depth) {
        T.jpa[(pn[e]) * T.ns] = njp[from];
        T.jlv[(pn[e]) * T.ns] = njl[from];
      }
    }
  } else {
    int* src = nxa;
    int* dst = nxb;
    for (int span = 1; span <= depth; span <<= 1) {
      for (int e = tid; e <= depth; e += nthr) dst[e] = src[src[e]];
      step_barrier<LDSB>();
      int* t = src; src = dst; dst = t;
    }
    for (int e = tid; e <= depth; e += nthr) {
      const int from = src[e];
      T.jpa[(pn[e]) * T.ns] = njp[from];
      T.jlv[(pn[e]) * T.ns] = njl[from];
    }
  }
  MZ_JT(5)
  if (select_next && sim + 1 < s.S) {
    step_barrier<LDSB>();  // the refreshed records (and, above, the statistics a near-tie evaluation reads) are visible
    jump_select_body<true>(s, g, T, sim + 1, r, next_action_out, next_parent_embedding_out, sel_out, depth_acc);
  }
  MZ_JT(6)
}

}  // namespace mz
