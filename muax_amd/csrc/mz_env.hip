// mz_env.hip -- translation unit of the device vector environments (mz_env.cuh): ONE descriptor check, one reset body
// and one step body (argument checks and launch of env_reset_kernel<D> / env_step_kernel<D>) behind the four entries
// mzs_env_cartpole_reset / mzs_env_cartpole_step and mzs_env_classic_reset / mzs_env_classic_step; the classic entries
// choose D by the checked descriptor's `kind`.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "mz_env.cuh"
#include "mz_host.h"

namespace {

bool aligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

template <class G>  // mzs_env_cartpole or mzs_env_classic: the same fields, the classic one with a `kind`
int check_env(const G* g, const char* who, mz::Env* out) {
  if (!g || g->struct_size != (int32_t)sizeof(G))
    return mzh::fail(nullptr, MZS_E_INVALID, "%s: null environment or size mismatch (ABI)", who);
  if constexpr (std::is_same_v<G, mzs_env_classic>)
    if (g->kind != MZS_ENV_ACROBOT && g->kind != MZS_ENV_MOUNTAINCAR)
      return mzh::fail(nullptr, MZS_E_INVALID, "%s: unknown kind (MZS_ENV_ACROBOT or MZS_ENV_MOUNTAINCAR)", who);
  if (g->num_envs < 1 || g->max_episode_steps < 1)
    return mzh::fail(nullptr, MZS_E_INVALID, "%s: num_envs and max_episode_steps must be at least 1", who);
  if (!g->state || !g->t || !g->draws) return mzh::fail(nullptr, MZS_E_INVALID, "%s: null environment pointer", who);
  if (!aligned(g->state, 16)) return mzh::fail(nullptr, MZS_E_INVALID, "%s: state must be 16-byte aligned", who);
  if (int rc = mzh::check_device(g->device, who)) return rc;
  out->N = g->num_envs; out->max_steps = g->max_episode_steps;
  out->key0 = g->key[0]; out->key1 = g->key[1];
  out->state = g->state; out->t = g->t; out->draws = g->draws;
  return MZS_OK;
}

// obs_out must be aligned to D's observation store (D::kObsAlign: 16 or 8 bytes)
template <class D>
int check_obs(const float* obs_out, const char* who) {
  if (aligned(obs_out, D::kObsAlign)) return MZS_OK;
  return mzh::fail(nullptr, MZS_E_INVALID,
                   D::kObsAlign == 16 ? "%s: obs_out must be 16-byte aligned" : "%s: obs_out must be 8-byte aligned", who);
}

int env_grid(int n) { return (n + mz::kEnvThreads - 1) / mz::kEnvThreads; }

// The two bodies, after check_env has accepted the descriptor and filled `p`.
template <class D>
int env_reset(const mz::Env& p, int device, float* obs_out, void* stream_, const char* who) {
  if (!obs_out) return mzh::fail(nullptr, MZS_E_INVALID, "%s: null obs_out", who);
  if (int rc = check_obs<D>(obs_out, who)) return rc;
  MZS_HIP(nullptr, hipSetDevice(device));
  hipLaunchKernelGGL(mz::env_reset_kernel<D>, dim3(env_grid(p.N)), dim3(mz::kEnvThreads), 0,
                     static_cast<hipStream_t>(stream_), p, obs_out);
  MZS_HIP(nullptr, hipGetLastError());
  return MZS_OK;
}

template <class D>
int env_step(const mz::Env& p, int device, const mzs_env_step_args* a, void* stream_, const char* who) {
  if (!a || a->struct_size != (int32_t)sizeof(mzs_env_step_args))
    return mzh::fail(nullptr, MZS_E_INVALID, "%s: null arguments or size mismatch (ABI)", who);
  if (!a->a || !a->obs_out || !a->r_out || !a->done_out)
    return mzh::fail(nullptr, MZS_E_INVALID, "%s: null pointer", who);
  if (int rc = check_obs<D>(a->obs_out, who)) return rc;
  MZS_HIP(nullptr, hipSetDevice(device));
  const mz::EnvStepArgs q{p, a->a, a->obs_out, a->r_out, a->done_out};
  hipLaunchKernelGGL(mz::env_step_kernel<D>, dim3(env_grid(p.N)), dim3(mz::kEnvThreads), 0,
                     static_cast<hipStream_t>(stream_), q);
  MZS_HIP(nullptr, hipGetLastError());
  return MZS_OK;
}

}  // namespace

extern "C" {

int mzs_env_cartpole_reset(const mzs_env_cartpole* env, float* obs_out, void* stream) {
  const char* who = "mzs_env_cartpole_reset";
  mz::Env p{};
  if (int rc = check_env(env, who, &p)) return rc;
  return env_reset<mz::CartPole>(p, env->device, obs_out, stream, who);
}

int mzs_env_cartpole_step(const mzs_env_cartpole* env, const mzs_env_step_args* a, void* stream) {
  const char* who = "mzs_env_cartpole_step";
  mz::Env p{};
  if (int rc = check_env(env, who, &p)) return rc;
  return env_step<mz::CartPole>(p, env->device, a, stream, who);
}

int mzs_env_classic_reset(const mzs_env_classic* env, float* obs_out, void* stream) {
  const char* who = "mzs_env_classic_reset";
  mz::Env p{};
  if (int rc = check_env(env, who, &p)) return rc;
  return env->kind == MZS_ENV_ACROBOT ? env_reset<mz::Acrobot>(p, env->device, obs_out, stream, who)
                                      : env_reset<mz::MountainCar>(p, env->device, obs_out, stream, who);
}

int mzs_env_classic_step(const mzs_env_classic* env, const mzs_env_step_args* a, void* stream) {
  const char* who = "mzs_env_classic_step";
  mz::Env p{};
  if (int rc = check_env(env, who, &p)) return rc;
  return env->kind == MZS_ENV_ACROBOT ? env_step<mz::Acrobot>(p, env->device, a, stream, who)
                                      : env_step<mz::MountainCar>(p, env->device, a, stream, who);
}

}  // extern "C"
