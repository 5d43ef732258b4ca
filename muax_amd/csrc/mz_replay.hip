// mz_replay.hip -- translation unit of the device-resident trajectory replay (mz_replay.cuh): argument checks and
// launches of mzs_replay_store / mzs_replay_refresh / mzs_replay_sample / mzs_replay_sample_is / mzs_replay_gather_obs /
// mzs_replay_reanalyse / mzs_replay_update_priorities / mzs_replay_stage / mzs_replay_store_steps /
// mzs_replay_plan_steps.
#include <hip/hip_runtime.h>

#include <cstring>

#include "mz_host.h"
#include "mz_replay.cuh"

namespace {

// an argument struct is there and has the size this library was built for
template <typename A>
bool args_ok(const A* a, const char* who) {
  if (a && a->struct_size == (int32_t)sizeof(A)) return true;
  mzh::fail(nullptr, MZS_E_INVALID, "%s: null arguments or size mismatch (ABI)", who);
  return false;
}

int check_arena(const mzs_replay_arena* ar, const char* who, mz::ReplayArena* out) {
  if (!ar || ar->struct_size != (int32_t)sizeof(mzs_replay_arena))
    return mzh::fail(nullptr, MZS_E_INVALID, "%s: null arena or size mismatch (ABI)", who);
  if (ar->max_steps <= 0 || ar->max_steps >= ((int64_t)1 << 31) || ar->capacity <= 0 || ar->obs_dim <= 0 ||
      ar->num_actions <= 0)
    return mzh::fail(nullptr, MZS_E_INVALID, "%s: max_steps (< 2^31), capacity, obs_dim and num_actions must be positive", who);
  if (!ar->obs || !ar->a || !ar->r || !ar->Rn || !ar->v || !ar->done || !ar->pi || !ar->w || !ar->cw || !ar->t_start ||
      !ar->t_len || !ar->t_w || !ar->t_serial || !ar->c_start || !ar->c_len || !ar->c_CW || !ar->c_serial)
    return mzh::fail(nullptr, MZS_E_INVALID, "%s: null arena pointer", who);
  if (int rc = mzh::check_device(ar->device, who)) return rc;  // (selected after the entry point's own checks)
  out->max_steps = ar->max_steps; out->capacity = ar->capacity; out->obs_dim = ar->obs_dim; out->A = ar->num_actions;
  out->obs = ar->obs; out->a = ar->a; out->r = ar->r; out->Rn = ar->Rn; out->v = ar->v; out->done = ar->done;
  out->pi = ar->pi; out->w = ar->w; out->cw = ar->cw;
  out->t_start = ar->t_start; out->t_len = ar->t_len; out->t_w = ar->t_w; out->t_serial = (long long*)ar->t_serial;
  out->c_start = ar->c_start; out->c_len = ar->c_len; out->c_CW = ar->c_CW; out->c_serial = (long long*)ar->c_serial;
  return MZS_OK;
}

// finite, tested on the bits: the units are built with -fno-honor-nans, under which a comparison or std::isfinite may
// be compiled as if no NaN could reach it
bool finite_bits(double x) {
  uint64_t u;
  std::memcpy(&u, &x, sizeof u);
  return (u & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
}

// one launch of a kernel that has one wavefront per item, kReplayWaves of them per workgroup
template <typename... KernelArgs, typename... Args>
int launch_waves(void (*kernel)(KernelArgs...), int items, void* stream, const Args&... args) {
  hipLaunchKernelGGL(kernel, dim3((items + mz::kReplayWaves - 1) / mz::kReplayWaves), dim3(64 * mz::kReplayWaves), 0,
                     static_cast<hipStream_t>(stream), args...);
  MZS_HIP(nullptr, hipGetLastError());
  return MZS_OK;
}

// the [episodes][4] descriptors of a dense stream (host copy): every range inside the stream, the arena and the table
int check_desc_ranges(const mzs_replay_arena* ar, const char* who, int32_t episodes, int64_t stream_rows,
                      const int32_t* desc_host) {
  for (int e = 0; e < episodes; ++e) {
    const int32_t* d = desc_host + 4 * e;
    const int64_t src = d[0], dst = d[1], len = d[2];
    if (len <= 0 || src < 0 || src + len > stream_rows || dst < 0 || dst + len > ar->max_steps || d[3] < 0 ||
        d[3] >= ar->capacity)
      return mzh::fail(nullptr, MZS_E_INVALID, "%s: an episode's range leaves the stream, the arena or the table", who);
  }
  return MZS_OK;
}

// the stream and the episode descriptors of a reanalysis call
int check_stream_desc(const mzs_replay_arena* ar, const char* who, int32_t episodes, int64_t stream_rows,
                      int64_t rows_padded, const int32_t* desc, const int32_t* desc_host) {
  if (episodes <= 0 || episodes > ar->capacity || stream_rows <= 0 || rows_padded < stream_rows ||
      rows_padded >= ((int64_t)1 << 31))
    return mzh::fail(nullptr, MZS_E_INVALID, "%s: episodes must be 1..capacity, 1 <= stream_rows <= rows_padded < 2^31", who);
  if (!desc || !desc_host) return mzh::fail(nullptr, MZS_E_INVALID, "%s: null descriptor pointer", who);
  return check_desc_ranges(ar, who, episodes, stream_rows, desc_host);
}

// what nstep_transition needs (raw store, store from the ring, reanalysis) ...
int check_nstep(int32_t n_step, const double* gpow, const char* who) {
  if (n_step < 1 || !gpow) return mzh::fail(nullptr, MZS_E_INVALID, "%s: needs n_step >= 1 and gpow", who);
  return MZS_OK;
}

// ... and the table weight of an episode whose transition weights the device computes
int check_weight_mode(int32_t weight_mode, const char* who) {
  if (weight_mode != 1 && weight_mode != 2)
    return mzh::fail(nullptr, MZS_E_INVALID, "%s: weight_mode must be 1 (mean) or 2 (sum)", who);
  return MZS_OK;
}

// the checks and the kernel arguments both sample entries share (the device is selected by the caller afterwards)
int check_sample(const mzs_replay_arena* arena, const mzs_replay_sample_args* a, const char* who, mz::ReplaySampleArgs* p) {
  if (int rc = check_arena(arena, who, &p->ar)) return rc;
  if (!args_ok(a, who)) return MZS_E_INVALID;
  if (a->count <= 0 || a->count > arena->capacity || a->batch <= 0 || a->k_steps <= 0 || a->sample_per_trajectory <= 0)
    return mzh::fail(nullptr, MZS_E_INVALID, "%s: count in 1..capacity; batch, k_steps, sample_per_trajectory >= 1", who);
  if ((int64_t)a->k_steps * arena->num_actions >= ((int64_t)1 << 31) || a->k_steps >= arena->max_steps)
    return mzh::fail(nullptr, MZS_E_INVALID, "%s: k_steps too large", who);
  if (a->obs_steps != 0 && a->obs_steps != a->k_steps)
    return mzh::fail(nullptr, MZS_E_INVALID, "%s: obs_steps must be 0 (the first observation) or k_steps (every step's)", who);
  if (a->obs_steps != 0 && (int64_t)a->k_steps * arena->obs_dim >= ((int64_t)1 << 31))
    return mzh::fail(nullptr, MZS_E_INVALID, "%s: with obs_steps, k_steps * obs_dim must be below 2^31", who);
  if (!a->obs || !a->a || !a->r || !a->Rn || !a->v || !a->done || !a->pi || !a->w || !a->serial || !a->start)
    return mzh::fail(nullptr, MZS_E_INVALID, "%s: null output pointer", who);
  p->count = a->count; p->B = a->batch; p->k = a->k_steps; p->spt = a->sample_per_trajectory;
  p->obs_steps = a->obs_steps; p->key0 = a->key[0]; p->key1 = a->key[1];
  p->obs = a->obs; p->a = a->a; p->r = a->r; p->Rn = a->Rn; p->v = a->v; p->done = a->done; p->pi = a->pi; p->w = a->w;
  p->serial = (long long*)a->serial; p->start = a->start;
  return MZS_OK;
}

// the wider of a ring row's two vector fields, in floats
int64_t ring_widest(const mzs_replay_ring* g) { return g->obs_dim > g->num_actions ? g->obs_dim : g->num_actions; }

int check_ring(const mzs_replay_ring* g, const char* who, mz::ReplayRing* out) {
  if (!g || g->struct_size != (int32_t)sizeof(mzs_replay_ring))
    return mzh::fail(nullptr, MZS_E_INVALID, "%s: null ring or size mismatch (ABI)", who);
  if (g->ring_steps <= 0 || g->num_envs <= 0 || g->obs_dim <= 0 || g->num_actions <= 0)
    return mzh::fail(nullptr, MZS_E_INVALID, "%s: ring_steps, num_envs, obs_dim and num_actions must be positive", who);
  if (g->ring_steps * ring_widest(g) >= ((int64_t)1 << 31))
    return mzh::fail(nullptr, MZS_E_INVALID, "%s: ring_steps * max(obs_dim, num_actions) must be below 2^31", who);
  if (!g->obs || !g->a || !g->r || !g->v || !g->pi) return mzh::fail(nullptr, MZS_E_INVALID, "%s: null ring pointer", who);
  if (int rc = mzh::check_device(g->device, who)) return rc;
  out->steps = g->ring_steps; out->N = g->num_envs;
  out->obs = g->obs; out->a = g->a; out->r = g->r; out->v = g->v; out->pi = g->pi;
  return MZS_OK;
}

}  // namespace

extern "C" {

int mzs_replay_store(const mzs_replay_arena* arena, const mzs_replay_store_args* a, void* stream_) {
  mz::ReplayStoreArgs p{};
  if (int rc = check_arena(arena, "mzs_replay_store", &p.ar)) return rc;
  if (!args_ok(a, "mzs_replay_store")) return MZS_E_INVALID;
  if (a->episodes <= 0 || a->episodes > arena->capacity || a->stream_steps <= 0 || a->stream_steps >= ((int64_t)1 << 31))
    return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_store: episodes must be 1..capacity, stream_steps 1..2^31 - 1");
  if (!a->desc_host || !a->desc || !a->serial || !a->obs || !a->a || !a->pi || !a->r || !a->v)
    return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_store: null pointer");
  if (a->weight_mode < 0 || a->weight_mode > 2 || (a->weight_mode == 0 && !a->ep_w))
    return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_store: weight_mode must be 0 (with ep_w), 1 or 2");
  if (a->raw) {
    if (int rc = check_nstep(a->n_step, a->gpow, "mzs_replay_store")) return rc;
  } else if (!a->Rn || !a->done || !a->w || a->weight_mode != 0) {
    return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_store: without raw, Rn, done, w and ep_w must be given");
  }
  if (int rc = check_desc_ranges(arena, "mzs_replay_store", a->episodes, a->stream_steps, a->desc_host)) return rc;
  MZS_HIP(nullptr, hipSetDevice(arena->device));
  p.episodes = a->episodes; p.raw = a->raw ? 1 : 0; p.n_step = a->n_step; p.weight_mode = a->weight_mode;
  p.has_alpha = a->has_alpha ? 1 : 0; p.alpha = a->alpha;
  p.desc = a->desc; p.serial = (const long long*)a->serial; p.ep_w = a->ep_w; p.gpow = a->gpow;
  p.obs = a->obs; p.a = a->a; p.pi = a->pi;
  if (a->raw) { p.r64 = static_cast<const double*>(a->r); p.v64 = static_cast<const double*>(a->v); }
  else { p.r32 = static_cast<const float*>(a->r); p.v32 = static_cast<const float*>(a->v); }
  p.Rn = a->Rn; p.done = a->done; p.w = a->w;
  return launch_waves(mz::replay_store_kernel, a->episodes, stream_, p);
}

int mzs_replay_refresh(const mzs_replay_arena* arena, int32_t head, int32_t count, int32_t k_steps, void* stream_) {
  mz::ReplayArena ar{};
  if (int rc = check_arena(arena, "mzs_replay_refresh", &ar)) return rc;
  if (count <= 0 || count > arena->capacity || head < 0 || head >= arena->capacity || k_steps <= 0)
    return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_refresh: head in 0..capacity - 1, count in 1..capacity, k_steps >= 1");
  MZS_HIP(nullptr, hipSetDevice(arena->device));
  hipLaunchKernelGGL(mz::replay_refresh_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream_), ar, (int)head,
                     (int)count, (int)k_steps);
  MZS_HIP(nullptr, hipGetLastError());
  return MZS_OK;
}

int mzs_replay_sample(const mzs_replay_arena* arena, const mzs_replay_sample_args* a, void* stream_) {
  mz::ReplaySampleArgs p{};
  if (int rc = check_sample(arena, a, "mzs_replay_sample", &p)) return rc;
  MZS_HIP(nullptr, hipSetDevice(arena->device));
  return launch_waves(mz::replay_sample_kernel, a->batch, stream_, p);
}

int mzs_replay_sample_is(const mzs_replay_arena* arena, const mzs_replay_sample_args* a, const mzs_replay_is_args* w,
                         void* stream_) {
  mz::ReplaySampleArgs p{};
  if (int rc = check_sample(arena, a, "mzs_replay_sample_is", &p)) return rc;
  if (!args_ok(w, "mzs_replay_sample_is")) return MZS_E_INVALID;
  if (!finite_bits(w->beta) || w->beta < 0.0 || w->beta > 1.0)
    return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_sample_is: beta must be in 0..1");
  if (!finite_bits(w->num_windows) || w->num_windows < 1.0)
    return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_sample_is: num_windows must be finite and at least 1");
  if (!w->isw || (w->normalize && !w->scratch))
    return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_sample_is: null isw, or normalize without scratch");
  MZS_HIP(nullptr, hipSetDevice(arena->device));
  mz::ReplayIsArgs q{};
  q.beta = w->beta; q.N = w->num_windows; q.raw = w->normalize ? w->scratch : nullptr; q.isw = w->isw;
  if (int rc = launch_waves(mz::replay_sample_is_kernel, a->batch, stream_, p, q)) return rc;
  if (w->normalize) {
    hipLaunchKernelGGL(mz::replay_is_normalise_kernel, dim3(1), dim3(mz::kIsNormThreads), 0,
                       static_cast<hipStream_t>(stream_), q, (int)a->batch);
    MZS_HIP(nullptr, hipGetLastError());
  }
  return MZS_OK;
}

int mzs_replay_gather_obs(const mzs_replay_arena* arena, const mzs_replay_gather_args* a, void* stream_) {
  mz::ReplayGatherArgs p{};
  if (int rc = check_arena(arena, "mzs_replay_gather_obs", &p.ar)) return rc;
  if (!args_ok(a, "mzs_replay_gather_obs")) return MZS_E_INVALID;
  if (int rc = check_stream_desc(arena, "mzs_replay_gather_obs", a->episodes, a->stream_rows, a->rows_padded, a->desc,
                                 a->desc_host))
    return rc;
  if (!a->obs) return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_gather_obs: null output pointer");
  MZS_HIP(nullptr, hipSetDevice(arena->device));
  p.episodes = a->episodes; p.stream_rows = a->stream_rows; p.rows_padded = a->rows_padded;
  p.desc = a->desc; p.obs = a->obs;
  // one tail wavefront per 1024 padding floats, 64 at the most (they stride)
  const int64_t pad = (a->rows_padded - a->stream_rows) * (int64_t)arena->obs_dim;
  p.pad_waves = (int)(pad <= 0 ? 0 : (pad + 1023) / 1024 < 64 ? (pad + 1023) / 1024 : 64);
  return launch_waves(mz::replay_gather_obs_kernel, a->episodes + p.pad_waves, stream_, p);
}

int mzs_replay_reanalyse(const mzs_replay_arena* arena, const mzs_replay_reanalyse_args* a, void* stream_) {
  mz::ReplayReanalyseArgs p{};
  if (int rc = check_arena(arena, "mzs_replay_reanalyse", &p.ar)) return rc;
  if (!args_ok(a, "mzs_replay_reanalyse")) return MZS_E_INVALID;
  if (int rc = check_stream_desc(arena, "mzs_replay_reanalyse", a->episodes, a->stream_rows, a->rows_padded, a->desc,
                                 a->desc_host))
    return rc;
  if (int rc = check_nstep(a->n_step, a->gpow, "mzs_replay_reanalyse")) return rc;
  if (int rc = check_weight_mode(a->weight_mode, "mzs_replay_reanalyse")) return rc;
  if (!a->pi || !a->v) return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_reanalyse: null pi or v");
  MZS_HIP(nullptr, hipSetDevice(arena->device));
  p.episodes = a->episodes; p.n_step = a->n_step; p.weight_mode = a->weight_mode;
  p.has_alpha = a->has_alpha ? 1 : 0; p.alpha = a->alpha;
  p.desc = a->desc; p.gpow = a->gpow; p.pi = a->pi; p.v = a->v;
  return launch_waves(mz::replay_reanalyse_kernel, a->episodes, stream_, p);
}

int mzs_replay_update_priorities(const mzs_replay_arena* arena, const mzs_replay_update_args* a, void* stream_) {
  mz::ReplayUpdateArgs p{};
  if (int rc = check_arena(arena, "mzs_replay_update_priorities", &p.ar)) return rc;
  if (!args_ok(a, "mzs_replay_update_priorities")) return MZS_E_INVALID;
  if (a->head < 0 || a->head >= arena->capacity)
    return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_update_priorities: head must be in 0..capacity - 1");
  if (a->count < 0 || a->count > arena->capacity)
    return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_update_priorities: count must be in 0..capacity");
  if (a->batch < 0) return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_update_priorities: batch must not be negative");
  if (a->k_prio < 1 || (int64_t)a->batch * a->k_prio >= ((int64_t)1 << 31))
    return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_update_priorities: k_prio must be >= 1, batch * k_prio < 2^31");
  if (int rc = check_weight_mode(a->weight_mode, "mzs_replay_update_priorities")) return rc;
  if (!finite_bits(a->alpha) || a->alpha < 0.0 || a->alpha > 1.0)
    return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_update_priorities: alpha must be in 0..1");
  if (!finite_bits(a->eps) || a->eps < 0.0)
    return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_update_priorities: eps must be finite and not negative");
  if (a->batch > 0 && (!a->serial || !a->start || !a->prio))
    return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_update_priorities: null serial, start or prio");
  if (a->batch > 0 && (!a->owner || !a->touched))
    return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_update_priorities: null owner or touched scratch");
  if (a->batch == 0 || a->count == 0) return MZS_OK;
  MZS_HIP(nullptr, hipSetDevice(arena->device));
  p.head = a->head; p.count = a->count; p.B = a->batch; p.kp = a->k_prio; p.weight_mode = a->weight_mode;
  p.alpha = a->alpha; p.eps = a->eps;
  p.serial = (const long long*)a->serial; p.start = a->start; p.prio = a->prio;
  p.owner = a->owner; p.touched = a->touched;
  if (int rc = launch_waves(mz::replay_prio_mark_kernel, a->batch, stream_, p)) return rc;
  return launch_waves(mz::replay_prio_apply_kernel, a->count, stream_, p);
}

int mzs_replay_stage(const mzs_replay_ring* ring, const mzs_replay_stage_args* a, void* stream_) {
  mz::ReplayStageArgs p{};
  if (int rc = check_ring(ring, "mzs_replay_stage", &p.ring)) return rc;
  if (!args_ok(a, "mzs_replay_stage")) return MZS_E_INVALID;
  if (a->row < 0 || a->row >= ring->ring_steps)
    return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_stage: row must be in 0..ring_steps - 1");
  if (!a->obs || !a->a || !a->v || !a->pi) return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_stage: null pointer");
  MZS_HIP(nullptr, hipSetDevice(ring->device));
  p.row = a->row; p.obs_dim = ring->obs_dim; p.A = ring->num_actions;
  p.obs = a->obs; p.a = a->a; p.v = a->v; p.pi = a->pi;
  const int64_t blocks = (ring->num_envs * ring_widest(ring) + mz::kStageThreads - 1) / mz::kStageThreads;
  hipLaunchKernelGGL(mz::replay_stage_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(mz::kStageThreads), 0,
                     static_cast<hipStream_t>(stream_), p);
  MZS_HIP(nullptr, hipGetLastError());
  return MZS_OK;
}

int mzs_replay_store_steps(const mzs_replay_arena* arena, const mzs_replay_ring* ring,
                           const mzs_replay_store_steps_args* a, void* stream_) {
  mz::ReplayStoreStepsArgs p{};
  if (int rc = check_arena(arena, "mzs_replay_store_steps", &p.ar)) return rc;
  if (int rc = check_ring(ring, "mzs_replay_store_steps", &p.ring)) return rc;
  if (!args_ok(a, "mzs_replay_store_steps")) return MZS_E_INVALID;
  if (ring->obs_dim != arena->obs_dim || ring->num_actions != arena->num_actions || ring->device != arena->device)
    return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_store_steps: ring and arena disagree in obs_dim, num_actions or device");
  if (a->episodes <= 0 || a->episodes > arena->capacity)
    return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_store_steps: episodes must be 1..capacity");
  if (!a->desc_host || !a->desc || !a->serial)
    return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_store_steps: null pointer");
  if (int rc = check_nstep(a->n_step, a->gpow, "mzs_replay_store_steps")) return rc;
  if (int rc = check_weight_mode(a->weight_mode, "mzs_replay_store_steps")) return rc;
  for (int e = 0; e < a->episodes; ++e) {
    const int32_t* d = a->desc_host + 5 * e;
    const int64_t len = d[2], dst = d[3];
    if (d[0] < 0 || d[0] >= ring->num_envs)
      return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_store_steps: an episode's environment is outside 0..num_envs - 1");
    if (len < 1 || len > ring->ring_steps || d[1] < 0 || d[1] >= ring->ring_steps)
      return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_store_steps: an episode's first row or length leaves the ring");
    if (dst < 0 || dst + len > arena->max_steps || d[4] < 0 || d[4] >= arena->capacity)
      return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_store_steps: an episode's range leaves the arena or the table");
  }
  MZS_HIP(nullptr, hipSetDevice(arena->device));
  p.episodes = a->episodes; p.n_step = a->n_step; p.weight_mode = a->weight_mode;
  p.has_alpha = a->has_alpha ? 1 : 0; p.alpha = a->alpha;
  p.desc = a->desc; p.serial = (const long long*)a->serial; p.gpow = a->gpow;
  return launch_waves(mz::replay_store_steps_kernel, a->episodes, stream_, p);
}

int mzs_replay_plan_steps(const mzs_replay_ring* ring, const mzs_replay_plan_args* a, void* stream_) {
  mz::ReplayPlanArgs p{};
  if (int rc = check_ring(ring, "mzs_replay_plan_steps", &p.ring)) return rc;
  if (!args_ok(a, "mzs_replay_plan_steps")) return MZS_E_INVALID;
  if (a->row0 < 0 || a->row0 >= ring->ring_steps)
    return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_plan_steps: row0 must be in 0..ring_steps - 1");
  if (a->steps < 1 || a->steps > ring->ring_steps)
    return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_plan_steps: steps must be in 1..ring_steps");
  if ((int64_t)ring->num_envs * a->steps >= ((int64_t)1 << 31))
    return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_plan_steps: num_envs * steps must be below 2^31");
  if (a->min_length < 1) return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_plan_steps: min_length must be >= 1");
  if (a->max_out < 1) return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_plan_steps: max_out must be >= 1");
  const void* ptrs[] = {a->done, a->open_len, a->open_ret, a->ep, a->ret, a->counts, a->scratch};
  const char* names[] = {"done", "open_len", "open_ret", "ep", "ret", "counts", "scratch"};
  for (int i = 0; i < 7; ++i)
    if (!ptrs[i]) return mzh::fail(nullptr, MZS_E_INVALID, "mzs_replay_plan_steps: null %s", names[i]);
  MZS_HIP(nullptr, hipSetDevice(ring->device));
  p.row0 = a->row0; p.T = a->steps; p.min_length = a->min_length; p.max_out = a->max_out;
  p.done = a->done; p.open_len = a->open_len; p.open_ret = a->open_ret; p.ep = a->ep; p.ret = a->ret;
  p.counts = a->counts; p.scratch = a->scratch;
  const unsigned blocks = (unsigned)(((int64_t)ring->num_envs + mz::kPlanThreads - 1) / mz::kPlanThreads);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(mz::replay_plan_count_kernel, dim3(blocks), dim3(mz::kPlanThreads), 0, stream, p);
  MZS_HIP(nullptr, hipGetLastError());
  hipLaunchKernelGGL(mz::replay_plan_emit_kernel, dim3(blocks), dim3(mz::kPlanThreads), 0, stream, p);
  MZS_HIP(nullptr, hipGetLastError());
  return MZS_OK;
}

}  // extern "C"
