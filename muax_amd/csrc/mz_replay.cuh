// mz_replay.cuh -- device-resident trajectory replay (muax/replay_buffer.py:161-262 on the GPU).
//
// Whole episodes lie contiguous in per-field arenas of `max_steps` transitions, so a k-step training window is one
// contiguous range of every field.  Three kernels, one wavefront per episode / per batch row, vector stores only:
//   replay_store_kernel    copies the episodes of one add into the arenas; with `raw` it first computes the n-step
//                          returns, `done` and the priority weights (muax_amd/vector.py:25-52) in fp64; then the
//                          inclusive prefix sum `cw` of the transition weights and the episode's row of the table
//   replay_refresh_kernel  the live episodes, oldest first, as a compact table with the inclusive prefix sum CW of the
//                          weights of those longer than k_steps (one wavefront; after adds or a change of k_steps)
//   replay_sample_kernel   per batch row: two threefry draws, the episode and the start by binary search in CW / cw,
//                          then 64 lanes copy the window (obs: its first row, or with obs_steps the contiguous run
//                          of all k); replay_sample_is_kernel, the same rows, adds the row's
//                          importance-sampling weight, which replay_is_normalise_kernel scales by the batch maximum
// and the two of reanalysis (fresh search results for episodes already held), again one wavefront per episode:
//   replay_gather_obs_kernel  the observations of the selected episodes as one dense stream, zero-padded to whole chunks
//   replay_reanalyse_kernel   new pi and v in place; Rn, done, w from the STORED rewards and the new values by the store
//                             kernel's arithmetic (nstep_transition); then cw and the episode's table weight
// and the two that write training priorities back (rows (serial, start) as the sample kernel returns them), one
// wavefront per batch row, then one per live episode:
//   replay_prio_mark_kernel   finds the row's episode by its serial and enters the row's index, by atomic max, as the
//                             owner of every transition it validly addresses; flags the episode
//   replay_prio_apply_kernel  flagged episodes only: w = (|p| + eps) ** alpha from the owner's priority, then cw and
//                             the table weight; clears the owners and the flag
// and the two of collection on the device (a vector environment's steps staged in a caller-owned STEP-MAJOR ring of
// ring_steps x num_envs rows, so an episode's transitions lie num_envs rows apart and may wrap at the ring's end):
//   replay_stage_kernel        one step's obs, a, v, pi of every environment into one ring row (rewards come later)
//   replay_store_steps_kernel  the raw store reading that strided source: one wavefront per finished episode, the
//                              same transition pass (raw_store_pass, instantiated for pointers and for RingColumn)
//                              and table row, so the same bits as the dense store.  The strided reads have NOT been
//                              measured against the dense ones.
// Every kernel that has one wavefront per episode or batch row opens with wave_item.  The four that write an episode's
// weights (store, store_steps, reanalyse, prio_apply) run ONE loop, episode_weight_pass, each with its own
// per-transition body, and take the table weight from table_weight.
// Every prefix sum is the SEQUENTIAL fp64 sum (np.cumsum's order), one addition per element on a wave-uniform carry:
// monotone, so the searches are well defined, and equal to the host's bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mz_spec.cuh"

#pragma clang fp contract(off)

namespace mz {

constexpr int kReplayWaves = 4;  // wavefronts (episodes / batch rows) per workgroup

struct ReplayArena {
  long long max_steps;
  int capacity, obs_dim, A;
  float* obs; int32_t* a; float* r; float* Rn; float* v; uint8_t* done; float* pi; double* w; double* cw;
  int32_t* t_start; int32_t* t_len; double* t_w; long long* t_serial;          // [capacity], by slot
  int32_t* c_start; int32_t* c_len; double* c_CW; long long* c_serial;         // [capacity], oldest first
};

struct ReplayStoreArgs {
  ReplayArena ar;
  int episodes, raw, n_step, weight_mode, has_alpha;
  double alpha;
  const int32_t* desc;        // [episodes][4]: first transition in the stream, first in the arena, length, table slot
  const long long* serial;    // [episodes]
  const double* ep_w;         // [episodes] (weight_mode 0)
  const double* gpow;         // [n_step + 1]: gamma ** i (raw)
  const float* obs; const int32_t* a; const float* pi;
  const float* r32; const float* v32; const double* r64; const double* v64;  // raw reads the fp64 pair
  const float* Rn; const uint8_t* done; const double* w;
};

struct ReplayGatherArgs {
  ReplayArena ar;
  int episodes, pad_waves;    // wavefronts e >= episodes (pad_waves of them) zero the padding
  long long stream_rows, rows_padded;
  const int32_t* desc;        // [episodes][4], as ReplayStoreArgs
  float* obs;                 // out [rows_padded, obs_dim]
};

struct ReplayReanalyseArgs {
  ReplayArena ar;
  int episodes, n_step, weight_mode, has_alpha;
  double alpha;
  const int32_t* desc;        // [episodes][4], as ReplayStoreArgs
  const double* gpow;         // [n_step + 1]
  const float* pi;            // [stream_rows, A]
  const float* v;             // [stream_rows]
};

struct ReplaySampleArgs {
  ReplayArena ar;
  int count, B, k, spt;
  int obs_steps;              // 0: obs is [B, obs_dim], the window's first observation; k: [B, k, obs_dim], every step's
  uint32_t key0, key1;
  float* obs; int32_t* a; float* r; float* Rn; float* v; uint8_t* done; float* pi; float* w;
  long long* serial; int32_t* start;
};

struct ReplayIsArgs {
  double beta, N;             // exponent in 0..1; eligible windows: the sum of len - k over the live episodes with len > k
  double* raw;                // [B] scratch of the normalisation pass, or null: isw is written by the sample kernel
  float* isw;                 // [B]
};

struct ReplayUpdateArgs {
  ReplayArena ar;
  int head, count, B, kp, weight_mode;
  double alpha, eps;
  const long long* serial;    // [B]
  const int32_t* start;       // [B]
  const float* prio;          // [B][kp]
  int32_t* owner;             // [max_steps] scratch: -1 on entry and on exit
  int32_t* touched;           // [capacity] scratch: 0 on entry and on exit
};

struct ReplayRing {
  int steps, N;               // ring rows (environment steps), environments
  float* obs; int32_t* a; double* r; float* v; float* pi;  // [steps, N, obs_dim], [steps, N] x 3, [steps, N, A]
};

struct ReplayStageArgs {
  ReplayRing ring;
  int row, obs_dim, A;
  const float* obs; const int32_t* a; const float* v; const float* pi;
};

struct ReplayStoreStepsArgs {
  ReplayArena ar;
  ReplayRing ring;
  int episodes, n_step, weight_mode, has_alpha;
  double alpha;
  const int32_t* desc;        // [episodes][5]: environment, first ring row, length, first in the arena, table slot
  const long long* serial;    // [episodes]
  const double* gpow;         // [n_step + 1]: gamma ** i
};

struct ReplayPlanArgs {
  ReplayRing ring;
  int row0, T, min_length, max_out;
  const uint8_t* done;        // [steps, N]
  int32_t* open_len;          // [N] in/out
  double* open_ret;           // [N] in/out
  int32_t* ep;                // out [max_out][4]: environment, first ring row, length, stored
  double* ret;                // out [max_out]
  int32_t* counts;            // out [4]: episodes, stored episodes, max open_len afterwards, 0
  int32_t* scratch;           // [ceil(N / kPlanThreads) + N]: the workgroups' episode counts, then the environments'
};

// ring row of transition t of an episode that began in row `first` (t < steps: one wrap at the most)
MZ_DEV int ring_row(int first, int t, int steps) {
  const int row = first + t;
  return row >= steps ? row - steps : row;
}

// One environment's column of a [steps, N] ring field, indexed by the transition inside an episode: what
// nstep_transition reads where the dense store has a pointer.
template <typename T>
struct RingColumn {
  const T* col;               // field + environment
  int first, steps, N;
  MZ_DEV T operator[](int t) const { return col[(size_t)ring_row(first, t, steps) * N]; }
};

// the wave prologue of the kernels that have one wavefront per episode / batch row: `const int e = wave_item(), lane =
// wave_lane();` -- the item is wave-uniform; plain ints, so the kernels' lambdas may name them
MZ_DEV int wave_item() { return __builtin_amdgcn_readfirstlane(blockIdx.x * kReplayWaves + (threadIdx.x >> 6)); }
MZ_DEV int wave_lane() { return threadIdx.x & 63; }

MZ_DEV double lane_bcast(double x, int j) {  // j wave-uniform
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), j);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(x), j);
  return __hiloint2double(hi, lo);
}

// inclusive sequential prefix sum over the first `valid` lanes, continued from the wave-uniform `carry`
MZ_DEV double seq_scan(double x, int valid, int lane, double& carry) {
  double mine = 0.0;
  for (int j = 0; j < valid; ++j) {
    carry = carry + lane_bcast(x, j);
    if (lane == j) mine = carry;
  }
  return mine;
}

// (y0 << 32 | y1) >> 11 of one threefry block, as a double in [0, 1)
MZ_DEV double uniform53(uint32_t k0, uint32_t k1, uint32_t x0, uint32_t x1) {
  threefry2x32(k0, k1, x0, x1);
  const unsigned long long bits = (((unsigned long long)x0 << 32) | x1) >> 11;
  return (double)bits * 0x1p-53;
}

// first i in [0, n) with c[i] > t, n when there is none (c ascending)
MZ_DEV int upper_bound(const double* c, int n, double t) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (c[mid] > t) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// Transition t of an episode of T steps with rewards r[0..T) and values v[0..T) (double, or float widened; dense
// pointers or columns of the collection ring: anything with operator[]):
// vector.nstep_returns in its operation order -- i ascending (terms past the end are + gamma^i * 0), then the bootstrap --
// and episode_trajectory's priority weight.  Returns w; Rn and boot (false: `done`) by reference.
template <typename R, typename V>
MZ_DEV double nstep_transition(R r, V v, int t, int T, int n_step, const double* gpow, int has_alpha, double alpha,
                               double& Rn, bool& boot) {
  Rn = 0.0;
  for (int i = 0; i < n_step; ++i) Rn = Rn + gpow[i] * (t + i < T ? (double)r[t + i] : 0.0);
  boot = t + n_step < T;
  Rn = Rn + (boot ? (double)v[t + n_step] * gpow[n_step] : 0.0);
  // alpha == 1.0: no pow is executed (the device pow does not return x exactly for y == 1: measured 2.1e-16 relative),
  // so w is exactly |v - Rn|, NumPy's x ** 1.0 -- as replay_prio_apply_kernel does
  const double d = fabs((double)v[t] - Rn);
  return has_alpha ? (alpha == 1.0 ? d : pow(d, alpha)) : 1.0;
}

// The weight pass of an episode of T transitions whose arena rows begin at dst, 64 transitions at a time: f(t) is
// transition t's weight w (f also makes the kernel's own stores for t, w among them), cw its sequential prefix sum.
// Returns the sum of the episode's weights (wave-uniform).
template <typename F>
MZ_DEV double episode_weight_pass(int T, int lane, size_t dst, const ReplayArena& ar, F f) {
  double carry = 0.0;
  for (int base = 0; base < T; base += 64) {
    const int t = base + lane;
    const bool in = t < T;
    const double w = in ? f(t) : 0.0;
    const int valid = T - base < 64 ? T - base : 64;
    const double c = seq_scan(w, valid, lane, carry);
    if (in) ar.cw[dst + t] = c;
  }
  return carry;
}

// an episode's weight in the table from the sum of its transition weights: the mean (mode 1) or the sum (mode 2)
MZ_DEV double table_weight(int mode, double sum, int T) { return mode == 1 ? sum / (double)T : sum; }

// The transition pass of a raw store (p: ReplayStoreArgs or ReplayStoreStepsArgs): a, r, v of the episode from the
// dense stream (pointers at its first transition) or from the ring (RingColumn), Rn / done / w by nstep_transition.
template <typename P, typename R, typename V, typename Ac>
MZ_DEV double raw_store_pass(const P& p, R r, V v, Ac a, int T, int lane, size_t dst) {
  const ReplayArena& ar = p.ar;
  return episode_weight_pass(T, lane, dst, ar, [&](int t) {
    ar.a[dst + t] = a[t];
    double Rn;
    bool boot;
    const double w = nstep_transition(r, v, t, T, p.n_step, p.gpow, p.has_alpha, p.alpha, Rn, boot);
    ar.r[dst + t] = (float)r[t];
    ar.v[dst + t] = (float)v[t];  // (exact from the ring's float)
    ar.Rn[dst + t] = (float)Rn;
    ar.done[dst + t] = boot ? 0 : 1;
    ar.w[dst + t] = w;
    return w;
  });
}

// lane 0: the episode's row of the table
MZ_DEV void store_table_row(const ReplayArena& ar, int slot, size_t dst, int T, double w, long long serial) {
  ar.t_start[slot] = (int32_t)dst;
  ar.t_len[slot] = T;
  ar.t_w[slot] = w;
  ar.t_serial[slot] = serial;
}

__global__ void __launch_bounds__(64 * kReplayWaves) replay_store_kernel(ReplayStoreArgs p) {
  const int e = wave_item(), lane = wave_lane();
  if (e >= p.episodes) return;
  const ReplayArena& ar = p.ar;
  const size_t src = (size_t)p.desc[4 * e], dst = (size_t)p.desc[4 * e + 1];
  const int T = p.desc[4 * e + 2], slot = p.desc[4 * e + 3];
  const size_t no = (size_t)T * ar.obs_dim, np_ = (size_t)T * ar.A;
  for (size_t i = lane; i < no; i += 64) ar.obs[dst * ar.obs_dim + i] = p.obs[src * ar.obs_dim + i];
  for (size_t i = lane; i < np_; i += 64) ar.pi[dst * ar.A + i] = p.pi[src * ar.A + i];
  double sum;
  if (p.raw) {
    sum = raw_store_pass(p, p.r64 + src, p.v64 + src, p.a + src, T, lane, dst);
  } else {
    sum = episode_weight_pass(T, lane, dst, ar, [&](int t) {
      ar.a[dst + t] = p.a[src + t];
      const double w = p.w[src + t];
      ar.r[dst + t] = p.r32[src + t];
      ar.v[dst + t] = p.v32[src + t];
      ar.Rn[dst + t] = p.Rn[src + t];
      ar.done[dst + t] = p.done[src + t] ? 1 : 0;
      ar.w[dst + t] = w;
      return w;
    });
  }
  if (lane == 0)
    store_table_row(ar, slot, dst, T, p.weight_mode == 0 ? p.ep_w[e] : table_weight(p.weight_mode, sum, T), p.serial[e]);
}

// One step of a vector environment into ring row p.row: four dense copies, consecutive lanes on consecutive elements.
constexpr int kStageThreads = 256;
__global__ void __launch_bounds__(kStageThreads) replay_stage_kernel(ReplayStageArgs p) {
  const ReplayRing& g = p.ring;
  const size_t N = (size_t)g.N, row = (size_t)p.row;
  const size_t first = (size_t)blockIdx.x * kStageThreads + threadIdx.x, step = (size_t)gridDim.x * kStageThreads;
  const size_t no = N * p.obs_dim, np_ = N * p.A;
  for (size_t i = first; i < no; i += step) g.obs[row * no + i] = p.obs[i];
  for (size_t i = first; i < np_; i += step) g.pi[row * np_ + i] = p.pi[i];
  for (size_t i = first; i < N; i += step) {
    g.a[row * N + i] = p.a[i];
    g.v[row * N + i] = p.v[i];
  }
}

// replay_store_kernel with raw == 1 whose source is the ring: transition t of the episode is ring row
// (first + t) % steps, column env.  The 64 lanes run over the ELEMENTS of consecutive transitions, as the dense copy
// does: a wavefront reads whole rows of obs_dim (A) floats, each contiguous, N rows apart (the host keeps
// steps * obs_dim and steps * A below 2^31, so the element index is an int).  How much these strided reads cost
// against the dense store's has not been measured.
__global__ void __launch_bounds__(64 * kReplayWaves) replay_store_steps_kernel(ReplayStoreStepsArgs p) {
  const int e = wave_item(), lane = wave_lane();
  if (e >= p.episodes) return;
  const ReplayArena& ar = p.ar;
  const ReplayRing& g = p.ring;
  const int env = p.desc[5 * e], first = p.desc[5 * e + 1], T = p.desc[5 * e + 2], slot = p.desc[5 * e + 4];
  const size_t dst = (size_t)p.desc[5 * e + 3], N = (size_t)g.N;
  const int od = ar.obs_dim, A = ar.A;
  for (int i = lane; i < T * od; i += 64) {
    const int t = i / od, c = i - t * od;
    ar.obs[dst * od + i] = g.obs[((size_t)ring_row(first, t, g.steps) * N + env) * od + c];
  }
  for (int i = lane; i < T * A; i += 64) {
    const int t = i / A, c = i - t * A;
    ar.pi[dst * A + i] = g.pi[((size_t)ring_row(first, t, g.steps) * N + env) * A + c];
  }
  const double sum = raw_store_pass(p, RingColumn<double>{g.r + env, first, g.steps, g.N},
                                    RingColumn<float>{g.v + env, first, g.steps, g.N},
                                    RingColumn<int32_t>{g.a + env, first, g.steps, g.N}, T, lane, dst);
  if (lane == 0) store_table_row(ar, slot, dst, T, table_weight(p.weight_mode, sum, T), p.serial[e]);
}

// The episode plan of a collection call (vector.ring_plan and collect()'s returns, muax_amd/vector.py) on the device.
// One THREAD per environment walks the call's T ring rows in time order, so a wavefront reads 64 consecutive flag
// bytes and 64 consecutive doubles of every row.  Two launches on one stream:
//   replay_plan_count_kernel  every environment's number of episode ends into scratch[blocks + e], every workgroup's
//                             total into scratch[block]; clears counts
//   replay_plan_emit_kernel   the exclusive prefix of those counts (the earlier workgroups' totals summed, then a scan
//                             inside the workgroup) is the environment's first output row; it walks again, with the
//                             length and the fp64 return `g = g + r` carried in open_len / open_ret, and writes one
//                             (environment, first ring row, length, stored) row and one return per episode end
// so the output is dense, environment-major then time, and does not depend on the order in which workgroups run.
// counts[1] and counts[2] are integer atomics (a sum and a maximum: any order gives the same value); the last workgroup
// writes counts[0].  Rows at or beyond max_out are counted, not written.
// Scale: every emit workgroup sums the totals of ALL workgroups in front of it from global memory, blocks^2 / 2 reads
// in all -- 10 at 1024 environments, 8 M at a million (4096 workgroups), where a third launch that scans the totals
// once would be the better structure.
constexpr int kPlanThreads = 256;

MZ_DEV int plan_next_row(int row, int steps) { return row + 1 == steps ? 0 : row + 1; }

// sum (MAX == false) or maximum of x over the workgroup, for every thread; s is kPlanThreads ints of LDS
template <bool MAX>
MZ_DEV int plan_reduce(int x, int* s) {
  const int tid = threadIdx.x;
  s[tid] = x;
  __syncthreads();
  for (int h = kPlanThreads / 2; h > 0; h >>= 1) {
    if (tid < h) s[tid] = MAX ? (s[tid] > s[tid + h] ? s[tid] : s[tid + h]) : s[tid] + s[tid + h];
    __syncthreads();
  }
  const int out = s[0];
  __syncthreads();
  return out;
}

__global__ void __launch_bounds__(kPlanThreads) replay_plan_count_kernel(ReplayPlanArgs p) {
  __shared__ int s[kPlanThreads];
  const size_t N = (size_t)p.ring.N, e = (size_t)blockIdx.x * kPlanThreads + threadIdx.x;
  int c = 0;
  if (e < N) {
    int row = p.row0;
    for (int t = 0; t < p.T; ++t) {
      c += p.done[(size_t)row * N + e] != 0;
      row = plan_next_row(row, p.ring.steps);
    }
    p.scratch[gridDim.x + e] = c;
  }
  const int total = plan_reduce<false>(c, s);
  if (threadIdx.x == 0) {
    p.scratch[blockIdx.x] = total;
    if (blockIdx.x == 0) p.counts[0] = p.counts[1] = p.counts[2] = p.counts[3] = 0;
  }
}

__global__ void __launch_bounds__(kPlanThreads) replay_plan_emit_kernel(ReplayPlanArgs p) {
  __shared__ int s[kPlanThreads];
  const int tid = threadIdx.x, S = p.ring.steps;
  const size_t N = (size_t)p.ring.N, e = (size_t)blockIdx.x * kPlanThreads + tid;
  int mine = 0;
  for (unsigned b = tid; b < blockIdx.x; b += kPlanThreads) mine += p.scratch[b];
  const int before = plan_reduce<false>(mine, s);  // episodes of the workgroups in front of this one
  const int c = e < N ? p.scratch[gridDim.x + e] : 0;
  s[tid] = c;
  __syncthreads();
  for (int d = 1; d < kPlanThreads; d <<= 1) {  // inclusive scan of the workgroup's counts
    const int left = tid >= d ? s[tid - d] : 0;
    __syncthreads();
    s[tid] += left;
    __syncthreads();
  }
  int at = before + s[tid] - c;
  const int through = before + s[kPlanThreads - 1];
  __syncthreads();
  int stored = 0, len = 0;
  if (e < N) {
    len = p.open_len[e];
    double g = p.open_ret[e];
    int first = ((p.row0 - len % S) + S) % S, row = p.row0;
    for (int t = 0; t < p.T; ++t) {
      const size_t i = (size_t)row * N + e;
      len += 1;
      g = g + p.ring.r[i];
      row = plan_next_row(row, S);
      if (p.done[i] != 0) {
        const int keep = len >= p.min_length ? 1 : 0;
        if (at < p.max_out) {
          int32_t* o = p.ep + 4 * (size_t)at;
          o[0] = (int32_t)e; o[1] = first; o[2] = len; o[3] = keep;
          p.ret[at] = g;
        }
        stored += keep;
        ++at;
        first = row;
        len = 0;
        g = 0.0;
      }
    }
    p.open_len[e] = len;
    p.open_ret[e] = g;
  }
  const int kept = plan_reduce<false>(stored, s), longest = plan_reduce<true>(len, s);
  if (tid == 0) {
    if (kept) atomicAdd(&p.counts[1], kept);
    if (longest > 0) atomicMax(&p.counts[2], longest);
    if (blockIdx.x == gridDim.x - 1) p.counts[0] = through;
  }
}

__global__ void __launch_bounds__(64 * kReplayWaves) replay_gather_obs_kernel(ReplayGatherArgs p) {
  const int e = wave_item(), lane = wave_lane();
  const size_t od = (size_t)p.ar.obs_dim;
  if (e < p.episodes) {
    const size_t src = (size_t)p.desc[4 * e], dst = (size_t)p.desc[4 * e + 1];
    const size_t no = (size_t)p.desc[4 * e + 2] * od;
    for (size_t i = lane; i < no; i += 64) p.obs[src * od + i] = p.ar.obs[dst * od + i];
    return;
  }
  const int j = e - p.episodes;  // the padding rows, strided over the pad_waves tail wavefronts
  if (j >= p.pad_waves) return;
  const size_t first = (size_t)p.stream_rows * od, end = (size_t)p.rows_padded * od;
  for (size_t i = first + (size_t)j * 64 + lane; i < end; i += (size_t)p.pad_waves * 64) p.obs[i] = 0.f;
}

__global__ void __launch_bounds__(64 * kReplayWaves) replay_reanalyse_kernel(ReplayReanalyseArgs p) {
  const int e = wave_item(), lane = wave_lane();
  if (e >= p.episodes) return;
  const ReplayArena& ar = p.ar;
  const size_t src = (size_t)p.desc[4 * e], dst = (size_t)p.desc[4 * e + 1];
  const int T = p.desc[4 * e + 2], slot = p.desc[4 * e + 3];
  const size_t np_ = (size_t)T * ar.A;
  for (size_t i = lane; i < np_; i += 64) ar.pi[dst * ar.A + i] = p.pi[src * ar.A + i];
  // rewards: the arena's (never written here); values, the bootstrap's included: the stream's, so no lane reads what
  // another lane of the wave writes
  const float* r = ar.r + dst;
  const float* v = p.v + src;
  const double sum = episode_weight_pass(T, lane, dst, ar, [&](int t) {
    double Rn;
    bool boot;
    const double w = nstep_transition(r, v, t, T, p.n_step, p.gpow, p.has_alpha, p.alpha, Rn, boot);
    ar.v[dst + t] = v[t];
    ar.Rn[dst + t] = (float)Rn;
    ar.done[dst + t] = boot ? 0 : 1;
    ar.w[dst + t] = w;
    return w;
  });
  if (lane == 0) ar.t_w[slot] = table_weight(p.weight_mode, sum, T);
}

__global__ void __launch_bounds__(64) replay_refresh_kernel(ReplayArena ar, int head, int count, int k) {
  const int lane = threadIdx.x;
  double carry = 0.0;
  for (int base = 0; base < count; base += 64) {
    const int i = base + lane;
    const bool in = i < count;
    int slot = in ? head + i : head;
    if (slot >= ar.capacity) slot -= ar.capacity;
    const int len = ar.t_len[slot];
    const double w = in && len > k ? ar.t_w[slot] : 0.0;
    const int valid = count - base < 64 ? count - base : 64;
    const double c = seq_scan(w, valid, lane, carry);
    if (in) {
      ar.c_start[i] = ar.t_start[slot];
      ar.c_len[i] = len;
      ar.c_serial[i] = ar.t_serial[slot];
      ar.c_CW[i] = c;
    }
  }
}

// One batch row of a sample; with IS also the row's importance-sampling weight: raw = (N q) ** -beta
// in fp64 from the very sums the two searches read, 0 for a zero-filled row; to q.raw for the normalisation pass, or,
// without one, rounded to q.isw.  The draws, the searches and every copy are the same code with and without IS.
template <bool IS>
MZ_DEV void replay_sample_row(const ReplaySampleArgs& p, const ReplayIsArgs& q) {
  const int row = wave_item(), lane = wave_lane();
  if (row >= p.B) return;
  const ReplayArena& ar = p.ar;
  const int k = p.k, A = ar.A, od = ar.obs_dim;
  // floats of obs per row: the window's observations are ONE contiguous run of the arena, its first obs_dim the default
  const int no = (p.obs_steps ? k : 1) * od;
  // the draws and the two searches are wave-uniform: scalar loads, done once per row
  const double u0 = uniform53(p.key0, p.key1, (uint32_t)(row / p.spt), 0u);
  const double u1 = uniform53(p.key0, p.key1, (uint32_t)row, 1u);
  const double total = ar.c_CW[p.count - 1];
  int e = upper_bound(ar.c_CW, p.count, u0 * total);
  if (e > p.count - 1) e = p.count - 1;  // (only when every weight is zero)
  const int T = ar.c_len[e], m = T - k;
  const size_t first = (size_t)ar.c_start[e];
  const size_t ok = (size_t)row * k;
  if (m <= 0) {  // nothing to draw from (the host refuses such a buffer; all-zero weights can still lead here): zeros
    for (int i = lane; i < k * A; i += 64) p.pi[ok * A + i] = 0.f;
    for (int i = lane; i < no; i += 64) p.obs[(size_t)row * no + i] = 0.f;
    for (int i = lane; i < k; i += 64) {
      p.a[ok + i] = 0; p.r[ok + i] = 0.f; p.Rn[ok + i] = 0.f; p.v[ok + i] = 0.f; p.done[ok + i] = 0; p.w[ok + i] = 0.f;
    }
    if (lane == 0) { p.serial[row] = -1; p.start[row] = -1; }
    if constexpr (IS) {
      if (lane == 0) {
        if (q.raw) q.raw[row] = 0.0; else q.isw[row] = 0.f;
      }
    }
    return;
  }
  const double* cw = ar.cw + first;
  const double tot = cw[m - 1];
  int s;
  if (tot == 0.0) {
    s = (int)floor(u1 * (double)m);
  } else {
    s = upper_bound(cw, m, u1 * tot);
  }
  if (s > m - 1) s = m - 1;
  const size_t at = first + (size_t)s;
  for (int i = lane; i < k * A; i += 64) p.pi[ok * A + i] = ar.pi[at * A + i];
  for (int i = lane; i < k; i += 64) {
    p.a[ok + i] = ar.a[at + i];
    p.r[ok + i] = ar.r[at + i];
    p.Rn[ok + i] = ar.Rn[at + i];
    p.v[ok + i] = ar.v[at + i];
    p.done[ok + i] = ar.done[at + i];
    p.w[ok + i] = (float)ar.w[at + i];
  }
  for (int i = lane; i < no; i += 64) p.obs[(size_t)row * no + i] = ar.obs[at * od + i];
  if (lane == 0) { p.serial[row] = ar.c_serial[e]; p.start[row] = s; }
  if constexpr (IS) {
    // wave-uniform: the marginal probability of window (e, s), the same for every row whatever shares its episode
    const double p_e = total == 0.0 ? 1.0 : (ar.c_CW[e] - (e > 0 ? ar.c_CW[e - 1] : 0.0)) / total;
    const double p_s = tot == 0.0 ? 1.0 / (double)m : (cw[s] - (s > 0 ? cw[s - 1] : 0.0)) / tot;
    const double x = q.N * (p_e * p_s);
    const double raw = q.beta == 1.0 ? 1.0 / x : q.beta == 0.0 ? 1.0 : pow(x, -q.beta);
    if (lane == 0) {
      if (q.raw) q.raw[row] = raw; else q.isw[row] = (float)raw;
    }
  }
}

__global__ void __launch_bounds__(64 * kReplayWaves) replay_sample_kernel(ReplaySampleArgs p) {
  replay_sample_row<false>(p, ReplayIsArgs{});
}

__global__ void __launch_bounds__(64 * kReplayWaves) replay_sample_is_kernel(ReplaySampleArgs p, ReplayIsArgs q) {
  replay_sample_row<true>(p, q);
}

// isw = raw / max(raw) over the batch, the maximum in fp64 (exact whatever the order, so the same bits on every run);
// an all-zero batch stays zero.  ONE workgroup: the pass is a few kilobytes.
constexpr int kIsNormThreads = 1024;
__global__ void __launch_bounds__(kIsNormThreads) replay_is_normalise_kernel(ReplayIsArgs q, int B) {
  __shared__ double red[kIsNormThreads];
  const int tid = threadIdx.x;
  double top = 0.0;
  for (int i = tid; i < B; i += kIsNormThreads) {
    const double x = q.raw[i];
    top = x > top ? x : top;
  }
  red[tid] = top;
  __syncthreads();
  for (int s = kIsNormThreads / 2; s > 0; s >>= 1) {
    if (tid < s) {
      const double a = red[tid], b = red[tid + s];
      red[tid] = b > a ? b : a;
    }
    __syncthreads();
  }
  top = red[0];
  for (int i = tid; i < B; i += kIsNormThreads) q.isw[i] = top > 0.0 ? (float)(q.raw[i] / top) : 0.f;
}

// table slot of the i-th live episode, oldest first
MZ_DEV int ring_slot(const ReplayArena& ar, int head, int i) {
  const int slot = head + i;
  return slot >= ar.capacity ? slot - ar.capacity : slot;
}

// PRECONDITION of both priority kernels (mzs_replay_refresh's): the live episodes are the `count` table slots from
// `head` on, wrapping at capacity, and their serials ascend along that ring (the store's running number).
__global__ void __launch_bounds__(64 * kReplayWaves) replay_prio_mark_kernel(ReplayUpdateArgs p) {
  const int row = wave_item(), lane = wave_lane();
  if (row >= p.B) return;
  const ReplayArena& ar = p.ar;
  // wave-uniform: the row's serial, the binary search for it along the ring, the episode's place
  const long long serial = p.serial[row];
  const int start = p.start[row];
  if (start < 0) return;
  int lo = 0, hi = p.count;
  while (lo < hi) {  // first live episode whose serial is not below the row's
    const int mid = (lo + hi) >> 1;
    if (ar.t_serial[ring_slot(ar, p.head, mid)] < serial) lo = mid + 1; else hi = mid;
  }
  if (lo >= p.count) return;
  const int slot = ring_slot(ar, p.head, lo);
  if (ar.t_serial[slot] != serial) return;  // evicted since the sample, or the -1 of a zero-filled row
  const long long first = ar.t_start[slot];
  const int T = ar.t_len[slot];
  if (first < 0 || T <= 0 || first + T > ar.max_steps) return;  // (no live episode; never index outside the arena)
  // the priorities as bits: NaN and +-inf (exponent all ones) are tested so, whatever the unit's floating-point flags
  const uint32_t* prio = reinterpret_cast<const uint32_t*>(p.prio) + (size_t)row * p.kp;
  bool any = false;
  for (int i = lane; i < p.kp && i < T - start; i += 64) {
    if ((prio[i] & 0x7F800000u) == 0x7F800000u) continue;
    atomicMax(p.owner + first + start + i, row);  // the highest row with a VALID element wins
    any = true;
  }
  if (any) p.touched[slot] = 1;
}

__global__ void __launch_bounds__(64 * kReplayWaves) replay_prio_apply_kernel(ReplayUpdateArgs p) {
  const int e = wave_item(), lane = wave_lane();
  if (e >= p.count) return;
  const ReplayArena& ar = p.ar;
  const int slot = ring_slot(ar, p.head, e);
  if (!p.touched[slot]) return;  // nothing of an episode that no valid element addresses is written
  const long long first = ar.t_start[slot];
  const int T = ar.t_len[slot];
  if (first < 0 || T <= 0 || first + T > ar.max_steps) return;  // (the mark pass flags no such slot)
  const size_t dst = (size_t)first;
  const double sum = episode_weight_pass(T, lane, dst, ar, [&](int t) {
    double w = ar.w[dst + t];
    const int o = p.owner[dst + t];
    if (o >= 0) {
      p.owner[dst + t] = -1;
      const int i = o < p.B ? t - p.start[o] : -1;
      if (i >= 0 && i < p.kp) {  // (always, with the scratch as the mark pass left it)
        const double x = fabs((double)p.prio[(size_t)o * p.kp + i]) + p.eps;
        w = p.alpha == 1.0 ? x : pow(x, p.alpha);
        ar.w[dst + t] = w;
      }
    }
    return w;
  });
  if (lane == 0) {
    ar.t_w[slot] = table_weight(p.weight_mode, sum, T);
    p.touched[slot] = 0;
  }
}

}  // namespace mz
