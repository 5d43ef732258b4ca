// mz_env2048.hip -- translation unit of the device 2048 (mz_env2048.cuh): the descriptor check and the three entries
// mzs_env_2048_reset / mzs_env_2048_step / mzs_env_2048_mask.  Everything is refused on the host, before any launch,
// with the argument named.
#include <hip/hip_runtime.h>

#include "mz_env2048.cuh"
#include "mz_host.h"

namespace {

bool aligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

int check_env(const mzs_env_2048* g, const char* who, mz::Env2048* out) {
  if (!g || g->struct_size != (int32_t)sizeof(mzs_env_2048))
    return mzh::fail(nullptr, MZS_E_INVALID, "%s: null environment or size mismatch (ABI)", who);
  if (g->num_envs < 1 || g->max_episode_steps < 1)
    return mzh::fail(nullptr, MZS_E_INVALID, "%s: num_envs and max_episode_steps must be at least 1", who);
  if (g->reward_shift < 0 || g->reward_shift > 11)
    return mzh::fail(nullptr, MZS_E_INVALID, "%s: reward_shift must be 0..11", who);
  if (!g->board || !g->t || !g->draws || !g->invalid)
    return mzh::fail(nullptr, MZS_E_INVALID, "%s: null environment pointer", who);
  if (!aligned(g->board, 8)) return mzh::fail(nullptr, MZS_E_INVALID, "%s: board must be 8-byte aligned", who);
  if (!aligned(g->t, 4) || !aligned(g->draws, 4))
    return mzh::fail(nullptr, MZS_E_INVALID, "%s: t and draws must be 4-byte aligned", who);
  if (!aligned(g->invalid, 4)) return mzh::fail(nullptr, MZS_E_INVALID, "%s: invalid must be 4-byte aligned", who);
  if (int rc = mzh::check_device(g->device, who)) return rc;
  out->N = g->num_envs; out->max_steps = g->max_episode_steps;
  out->key0 = g->key[0]; out->key1 = g->key[1];
  out->reward_scale = 1.0 / (double)(1u << g->reward_shift);
  out->board = g->board; out->t = g->t; out->draws = g->draws;
  out->invalid = reinterpret_cast<uint32_t*>(g->invalid);
  return MZS_OK;
}

// the observations of a row are moved as four float4; `out`: the argument is called obs_out, else obs
int check_obs(const float* obs, bool out, const char* who) {
  if (!obs) return mzh::fail(nullptr, MZS_E_INVALID, out ? "%s: null obs_out" : "%s: null obs", who);
  if (!aligned(obs, 16))
    return mzh::fail(nullptr, MZS_E_INVALID,
                     out ? "%s: obs_out must be 16-byte aligned" : "%s: obs must be 16-byte aligned", who);
  return MZS_OK;
}

int grid(int n) { return (n + mz::kEnv2048Threads - 1) / mz::kEnv2048Threads; }

}  // namespace

extern "C" {

int mzs_env_2048_reset(const mzs_env_2048* env, float* obs_out, void* stream) {
  const char* who = "mzs_env_2048_reset";
  mz::Env2048 p{};
  if (int rc = check_env(env, who, &p)) return rc;
  if (int rc = check_obs(obs_out, true, who)) return rc;
  MZS_HIP(nullptr, hipSetDevice(env->device));
  hipLaunchKernelGGL(mz::env2048_reset_kernel, dim3(grid(p.N)), dim3(mz::kEnv2048Threads), 0,
                     static_cast<hipStream_t>(stream), p, obs_out);
  MZS_HIP(nullptr, hipGetLastError());
  return MZS_OK;
}

int mzs_env_2048_step(const mzs_env_2048* env, const mzs_env_step_args* a, void* stream) {
  const char* who = "mzs_env_2048_step";
  mz::Env2048 p{};
  if (int rc = check_env(env, who, &p)) return rc;
  if (!a || a->struct_size != (int32_t)sizeof(mzs_env_step_args))
    return mzh::fail(nullptr, MZS_E_INVALID, "%s: null arguments or size mismatch (ABI)", who);
  if (!a->a || !a->r_out || !a->done_out) return mzh::fail(nullptr, MZS_E_INVALID, "%s: null pointer", who);
  if (int rc = check_obs(a->obs_out, true, who)) return rc;
  if (!aligned(a->a, 4)) return mzh::fail(nullptr, MZS_E_INVALID, "%s: a must be 4-byte aligned", who);
  if (!aligned(a->r_out, 8)) return mzh::fail(nullptr, MZS_E_INVALID, "%s: r_out must be 8-byte aligned", who);
  MZS_HIP(nullptr, hipSetDevice(env->device));
  const mz::Env2048StepArgs q{p, a->a, a->obs_out, a->r_out, a->done_out};
  hipLaunchKernelGGL(mz::env2048_step_kernel, dim3(grid(p.N)), dim3(mz::kEnv2048Threads), 0,
                     static_cast<hipStream_t>(stream), q);
  MZS_HIP(nullptr, hipGetLastError());
  return MZS_OK;
}

int mzs_env_2048_mask(int32_t device, const float* obs, uint8_t* invalid_out, int32_t B, void* stream) {
  const char* who = "mzs_env_2048_mask";
  if (B < 1) return mzh::fail(nullptr, MZS_E_INVALID, "%s: B must be at least 1", who);
  if (int rc = check_obs(obs, false, who)) return rc;
  if (!invalid_out) return mzh::fail(nullptr, MZS_E_INVALID, "%s: null invalid_out", who);
  if (!aligned(invalid_out, 4)) return mzh::fail(nullptr, MZS_E_INVALID, "%s: invalid_out must be 4-byte aligned", who);
  if (int rc = mzh::check_device(device, who)) return rc;
  MZS_HIP(nullptr, hipSetDevice(device));
  hipLaunchKernelGGL(mz::env2048_mask_kernel, dim3(grid(B)), dim3(mz::kEnv2048Threads), 0,
                     static_cast<hipStream_t>(stream), obs, reinterpret_cast<uint32_t*>(invalid_out), (int)B);
  MZS_HIP(nullptr, hipGetLastError());
  return MZS_OK;
}

}  // extern "C"
