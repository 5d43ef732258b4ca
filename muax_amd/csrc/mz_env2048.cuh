// mz_env2048.cuh -- 2048 stepped on the device, with the legal-move mask of every returned observation (DESIGN.md 4.7,
// "Device 2048").  The rules are mz_2048.h's; here are the three kernels, one thread per environment (or per row),
// everything in registers, vector stores only:
//   env2048_reset_kernel  every environment spawns twice on an empty board, t = 0
//   env2048_step_kernel   the move; after a legal one a spawn; a finished environment resets in the same launch, so
//                         obs and mask are already the next episode's
//   env2048_mask_kernel   the mask of observations [B, 16] (reanalysis of stored observations; a second witness of the
//                         step kernel's mask in the tests)
// Spawn d of environment e (d = draws[e], which then grows by one) takes the block threefry2x32(key, (e, d)) --
// env_uniform53's block and counter convention (mz_env.cuh).  An illegal move (one that leaves the board unchanged, or
// an action outside 0..3) is a no-op: reward 0, no spawn, no draw consumed; t still advances.
// reward = (sum of the tiles the merges created) * 2^-reward_shift in fp64: exact, and so is every partial sum.
// terminated = the board after the step is dead (also after a no-op); done = terminated or t >= max_episode_steps.
// obs [N, 16] float32, obs[i] = exponent_i / 16 (exact), stored as four float4; the mask uint8 [N, 4] as one 32-bit
// store, byte a = 1 where move a is illegal for the returned observation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mz_2048.h"
#include "mz_spec.cuh"

namespace mz {

constexpr int kEnv2048Threads = 256;

struct Env2048 {
  int N, max_steps;
  uint32_t key0, key1;
  double reward_scale;        // 2^-reward_shift
  uint64_t* board;            // [N]
  int32_t* t;                 // [N] steps of the open episode
  int32_t* draws;             // [N] spawns drawn so far
  uint32_t* invalid;          // [N] four mask bytes each (4-byte aligned)
};

struct Env2048StepArgs {
  Env2048 env;
  const int32_t* a;           // [N]
  float* obs;                 // [N, 16] (16-byte aligned)
  double* r;                  // [N]
  uint8_t* done;              // [N]
};

MZ_DEV uint64_t env2048_spawn(const Env2048& p, int e, int& d, uint64_t board) {
  uint32_t x0 = (uint32_t)e, x1 = (uint32_t)d;
  threefry2x32(p.key0, p.key1, x0, x1);
  d += 1;
  return mz2048::spawn(board, x0, x1);
}

MZ_DEV uint64_t env2048_fresh(const Env2048& p, int e, int& d) {
  return env2048_spawn(p, e, d, env2048_spawn(p, e, d, 0));
}

MZ_DEV void env2048_store_obs(uint64_t board, int row, float* obs) {
  float4* o = reinterpret_cast<float4*>(obs) + 4 * (size_t)row;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint32_t line = (uint32_t)(board >> (16 * r));
    o[r] = make_float4((float)(line & 15u) * 0.0625f, (float)((line >> 4) & 15u) * 0.0625f,
                       (float)((line >> 8) & 15u) * 0.0625f, (float)((line >> 12) & 15u) * 0.0625f);
  }
}

// board, observation and mask of environment e, the three that always go together
MZ_DEV void env2048_put(const Env2048& p, int e, uint64_t board, float* obs) {
  p.board[e] = board;
  env2048_store_obs(board, e, obs);
  p.invalid[e] = mz2048::mask_word(board);
}

__global__ void __launch_bounds__(kEnv2048Threads) env2048_reset_kernel(Env2048 p, float* obs) {
  const int e = blockIdx.x * kEnv2048Threads + threadIdx.x;
  if (e >= p.N) return;
  int d = p.draws[e];
  env2048_put(p, e, env2048_fresh(p, e, d), obs);
  p.t[e] = 0;
  p.draws[e] = d;
}

__global__ void __launch_bounds__(kEnv2048Threads) env2048_step_kernel(Env2048StepArgs q) {
  const Env2048& p = q.env;
  const int e = blockIdx.x * kEnv2048Threads + threadIdx.x;
  if (e >= p.N) return;
  const uint64_t before = p.board[e];
  int d = p.draws[e];
  uint32_t gained;
  uint64_t board = mz2048::move(before, q.a[e], gained);
  if (board != before) board = env2048_spawn(p, e, d, board);
  int t = p.t[e] + 1;
  const bool done = mz2048::dead(board) || t >= p.max_steps;
  if (done) {
    board = env2048_fresh(p, e, d);
    t = 0;
  }
  env2048_put(p, e, board, q.obs);
  p.t[e] = t;
  p.draws[e] = d;
  q.r[e] = (double)gained * p.reward_scale;
  q.done[e] = done ? 1 : 0;
}

// exponent = lrintf(obs * 16) clamped to 0..15
MZ_DEV uint64_t env2048_decode4(float4 v) {
  const float c[4] = {v.x, v.y, v.z, v.w};
  uint64_t line = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    long k = lrintf(c[i] * 16.0f);
    k = k < 0 ? 0 : (k > 15 ? 15 : k);
    line |= (uint64_t)k << (4 * i);
  }
  return line;
}

__global__ void __launch_bounds__(kEnv2048Threads) env2048_mask_kernel(const float* obs, uint32_t* invalid, int B) {
  const int j = blockIdx.x * kEnv2048Threads + threadIdx.x;
  if (j >= B) return;
  const float4* o = reinterpret_cast<const float4*>(obs) + 4 * (size_t)j;
  uint64_t board = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) board |= env2048_decode4(o[r]) << (16 * r);
  invalid[j] = mz2048::mask_word(board);
}

}  // namespace mz
