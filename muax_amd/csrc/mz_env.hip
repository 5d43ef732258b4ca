// mz_env.hip -- translation unit of the device vector environments (mz_env.cuh): argument checks and launches of
// mzs_env_cartpole_reset / mzs_env_cartpole_step, then of mzs_env_classic_reset / mzs_env_classic_step.
#include <hip/hip_runtime.h>

#include "mz_env.cuh"
#include "mz_host.h"

namespace {

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int check_env(const mzs_env_cartpole* g, const char* who, mz::EnvCartPole* out) {
  if (!g || g->struct_size != (int32_t)sizeof(mzs_env_cartpole))
    return mzh::fail(nullptr, MZS_E_INVALID, "%s: null environment or size mismatch (ABI)", who);
  if (g->num_envs < 1 || g->max_episode_steps < 1)
    return mzh::fail(nullptr, MZS_E_INVALID, "%s: num_envs and max_episode_steps must be at least 1", who);
  if (!g->state || !g->t || !g->draws) return mzh::fail(nullptr, MZS_E_INVALID, "%s: null environment pointer", who);
  if (!aligned16(g->state)) return mzh::fail(nullptr, MZS_E_INVALID, "%s: state must be 16-byte aligned", who);
  if (int rc = mzh::check_device(g->device, who)) return rc;
  out->N = g->num_envs; out->max_steps = g->max_episode_steps;
  out->key0 = g->key[0]; out->key1 = g->key[1];
  out->state = g->state; out->t = g->t; out->draws = g->draws;
  return MZS_OK;
}

int env_grid(int n) { return (n + mz::kEnvThreads - 1) / mz::kEnvThreads; }

}  // namespace

extern "C" {

int mzs_env_cartpole_reset(const mzs_env_cartpole* env, float* obs_out, void* stream_) {
  mz::EnvCartPole p{};
  if (int rc = check_env(env, "mzs_env_cartpole_reset", &p)) return rc;
  if (!obs_out) return mzh::fail(nullptr, MZS_E_INVALID, "mzs_env_cartpole_reset: null obs_out");
  if (!aligned16(obs_out)) return mzh::fail(nullptr, MZS_E_INVALID, "mzs_env_cartpole_reset: obs_out must be 16-byte aligned");
  MZS_HIP(nullptr, hipSetDevice(env->device));
  hipLaunchKernelGGL(mz::env_cartpole_reset_kernel, dim3(env_grid(p.N)), dim3(mz::kEnvThreads), 0,
                     static_cast<hipStream_t>(stream_), p, obs_out);
  MZS_HIP(nullptr, hipGetLastError());
  return MZS_OK;
}

int mzs_env_cartpole_step(const mzs_env_cartpole* env, const mzs_env_step_args* a, void* stream_) {
  mz::EnvStepArgs q{};
  if (int rc = check_env(env, "mzs_env_cartpole_step", &q.env)) return rc;
  if (!a || a->struct_size != (int32_t)sizeof(mzs_env_step_args))
    return mzh::fail(nullptr, MZS_E_INVALID, "mzs_env_cartpole_step: null arguments or size mismatch (ABI)");
  if (!a->a || !a->obs_out || !a->r_out || !a->done_out)
    return mzh::fail(nullptr, MZS_E_INVALID, "mzs_env_cartpole_step: null pointer");
  if (!aligned16(a->obs_out)) return mzh::fail(nullptr, MZS_E_INVALID, "mzs_env_cartpole_step: obs_out must be 16-byte aligned");
  MZS_HIP(nullptr, hipSetDevice(env->device));
  q.a = a->a; q.obs = a->obs_out; q.r = a->r_out; q.done = a->done_out;
  hipLaunchKernelGGL(mz::env_cartpole_step_kernel, dim3(env_grid(q.env.N)), dim3(mz::kEnvThreads), 0,
                     static_cast<hipStream_t>(stream_), q);
  MZS_HIP(nullptr, hipGetLastError());
  return MZS_OK;
}

}  // extern "C"

// ---- Acrobot and MountainCar: mzs_env_classic_reset / mzs_env_classic_step ----
namespace {

bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

int check_classic(const mzs_env_classic* g, const char* who, mz::EnvClassic* out) {
  if (!g || g->struct_size != (int32_t)sizeof(mzs_env_classic))
    return mzh::fail(nullptr, MZS_E_INVALID, "%s: null environment or size mismatch (ABI)", who);
  if (g->kind != MZS_ENV_ACROBOT && g->kind != MZS_ENV_MOUNTAINCAR)
    return mzh::fail(nullptr, MZS_E_INVALID, "%s: unknown kind (MZS_ENV_ACROBOT or MZS_ENV_MOUNTAINCAR)", who);
  if (g->num_envs < 1 || g->max_episode_steps < 1)
    return mzh::fail(nullptr, MZS_E_INVALID, "%s: num_envs and max_episode_steps must be at least 1", who);
  if (!g->state || !g->t || !g->draws) return mzh::fail(nullptr, MZS_E_INVALID, "%s: null environment pointer", who);
  if (!aligned16(g->state)) return mzh::fail(nullptr, MZS_E_INVALID, "%s: state must be 16-byte aligned", who);
  if (int rc = mzh::check_device(g->device, who)) return rc;
  out->N = g->num_envs; out->max_steps = g->max_episode_steps;
  out->key0 = g->key[0]; out->key1 = g->key[1];
  out->state = g->state; out->t = g->t; out->draws = g->draws;
  return MZS_OK;
}

}  // namespace

extern "C" {

int mzs_env_classic_reset(const mzs_env_classic* env, float* obs_out, void* stream_) {
  mz::EnvClassic p{};
  if (int rc = check_classic(env, "mzs_env_classic_reset", &p)) return rc;
  if (!obs_out) return mzh::fail(nullptr, MZS_E_INVALID, "mzs_env_classic_reset: null obs_out");
  if (!aligned8(obs_out)) return mzh::fail(nullptr, MZS_E_INVALID, "mzs_env_classic_reset: obs_out must be 8-byte aligned");
  MZS_HIP(nullptr, hipSetDevice(env->device));
  const dim3 grid(env_grid(p.N)), block(mz::kEnvThreads);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (env->kind == MZS_ENV_ACROBOT) hipLaunchKernelGGL(mz::env_acrobot_reset_kernel, grid, block, 0, stream, p, obs_out);
  else hipLaunchKernelGGL(mz::env_mountaincar_reset_kernel, grid, block, 0, stream, p, obs_out);
  MZS_HIP(nullptr, hipGetLastError());
  return MZS_OK;
}

int mzs_env_classic_step(const mzs_env_classic* env, const mzs_env_step_args* a, void* stream_) {
  mz::EnvClassicStepArgs q{};
  if (int rc = check_classic(env, "mzs_env_classic_step", &q.env)) return rc;
  if (!a || a->struct_size != (int32_t)sizeof(mzs_env_step_args))
    return mzh::fail(nullptr, MZS_E_INVALID, "mzs_env_classic_step: null arguments or size mismatch (ABI)");
  if (!a->a || !a->obs_out || !a->r_out || !a->done_out)
    return mzh::fail(nullptr, MZS_E_INVALID, "mzs_env_classic_step: null pointer");
  if (!aligned8(a->obs_out)) return mzh::fail(nullptr, MZS_E_INVALID, "mzs_env_classic_step: obs_out must be 8-byte aligned");
  MZS_HIP(nullptr, hipSetDevice(env->device));
  q.a = a->a; q.obs = a->obs_out; q.r = a->r_out; q.done = a->done_out;
  const dim3 grid(env_grid(q.env.N)), block(mz::kEnvThreads);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (env->kind == MZS_ENV_ACROBOT) hipLaunchKernelGGL(mz::env_acrobot_step_kernel, grid, block, 0, stream, q);
  else hipLaunchKernelGGL(mz::env_mountaincar_step_kernel, grid, block, 0, stream, q);
  MZS_HIP(nullptr, hipGetLastError());
  return MZS_OK;
}

}  // extern "C"
