// mz_env.cuh -- vector environments stepped on the device ("Device environments").
//
// One environment so far: the cart-pole of examples/cartpole_env.py (Barto, Sutton, Anderson 1983; explicit Euler at
// 50 Hz, reward 1 per step, the episode ends when |x| > 2.4 or |theta| > 12 degrees or after max_episode_steps steps).
// Two kernels, one thread per environment, vector stores only:
//   env_cartpole_reset_kernel  every environment draws a start state, t = 0, obs = (float)state
//   env_cartpole_step_kernel   VectorCartPole.step in fp64, operation by operation; a finished environment draws its
//                              next start state in the same launch, so obs is already the next episode's first one
// The start state of environment e, its d-th draw (d = draws[e], which then grows by one), component c:
//   state[c] = -0.05 + 0.1 * u53(key, e, 4 d + c)      u53 = ((y0 << 32 | y1) >> 11) * 2^-53 of threefry2x32
// the replay sampler's uniform (mz_replay.cuh): no libm call, so a draw is reproducible on the host bit for bit.  The
// step itself calls the device's fp64 sin and cos, which agree with a host libm to the last bits only.  The units are
// built with -ffp-contract=off: no multiply-add is fused.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mz_spec.cuh"

#pragma clang fp contract(off)

namespace mz {

constexpr int kEnvThreads = 256;

struct EnvCartPole {
  int N, max_steps;
  uint32_t key0, key1;
  double* state;              // [N, 4]: x, x_dot, theta, theta_dot (16-byte aligned)
  int32_t* t;                 // [N] steps of the open episode
  int32_t* draws;             // [N] start states drawn so far
};

struct EnvStepArgs {
  EnvCartPole env;
  const int32_t* a;           // [N]
  float* obs;                 // [N, 4] (16-byte aligned)
  double* r;                  // [N]
  uint8_t* done;              // [N]
};

// (y0 << 32 | y1) >> 11 of one threefry block, as a double in [0, 1): mz_replay.cuh's uniform53
MZ_DEV double env_uniform53(uint32_t k0, uint32_t k1, uint32_t x0, uint32_t x1) {
  threefry2x32(k0, k1, x0, x1);
  const unsigned long long bits = (((unsigned long long)x0 << 32) | x1) >> 11;
  return (double)bits * 0x1p-53;
}

MZ_DEV void cartpole_draw(const EnvCartPole& p, int e, int d, double (&s)[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c)
    s[c] = -0.05 + 0.1 * env_uniform53(p.key0, p.key1, (uint32_t)e, 4u * (uint32_t)d + (uint32_t)c);
}

MZ_DEV void cartpole_put(const EnvCartPole& p, int e, const double (&s)[4], float* obs) {
  double2* st = reinterpret_cast<double2*>(p.state) + 2 * (size_t)e;
  st[0] = make_double2(s[0], s[1]);
  st[1] = make_double2(s[2], s[3]);
  reinterpret_cast<float4*>(obs)[e] = make_float4((float)s[0], (float)s[1], (float)s[2], (float)s[3]);
}

__global__ void __launch_bounds__(kEnvThreads) env_cartpole_reset_kernel(EnvCartPole p, float* obs) {
  const int e = blockIdx.x * kEnvThreads + threadIdx.x;
  if (e >= p.N) return;
  const int d = p.draws[e];
  double s[4];
  cartpole_draw(p, e, d, s);
  cartpole_put(p, e, s, obs);
  p.t[e] = 0;
  p.draws[e] = d + 1;
}

__global__ void __launch_bounds__(kEnvThreads) env_cartpole_step_kernel(EnvStepArgs q) {
  const EnvCartPole& p = q.env;
  const int e = blockIdx.x * kEnvThreads + threadIdx.x;
  if (e >= p.N) return;
  constexpr double kGravity = 9.8, kMCart = 1.0, kMPole = 0.1, kHalfLen = 0.5, kForce = 10.0, kDt = 0.02;
  constexpr double kXLimit = 2.4, kThetaLimit = 12 * 2 * 3.141592653589793 / 360;  // (the host's expression)
  constexpr double m_total = kMCart + kMPole, pm_l = kMPole * kHalfLen;
  const double2* st = reinterpret_cast<const double2*>(p.state) + 2 * (size_t)e;
  const double2 s01 = st[0], s23 = st[1];
  double x = s01.x, x_dot = s01.y, th = s23.x, th_dot = s23.y;
  const double f = q.a[e] == 1 ? kForce : -kForce;
  const double c = cos(th), s = sin(th);
  const double tmp = (f + pm_l * th_dot * th_dot * s) / m_total;
  const double th_acc = (kGravity * s - c * tmp) / (kHalfLen * (4.0 / 3.0 - kMPole * c * c / m_total));
  const double x_acc = tmp - pm_l * th_acc * c / m_total;
  x = x + kDt * x_dot;
  x_dot = x_dot + kDt * x_acc;
  th = th + kDt * th_dot;
  th_dot = th_dot + kDt * th_acc;
  int t = p.t[e] + 1;
  const bool done = fabs(x) > kXLimit || fabs(th) > kThetaLimit || t >= p.max_steps;
  double ns[4] = {x, x_dot, th, th_dot};
  if (done) {
    const int d = p.draws[e];
    cartpole_draw(p, e, d, ns);
    p.draws[e] = d + 1;
    t = 0;
  }
  cartpole_put(p, e, ns, q.obs);
  p.t[e] = t;
  q.r[e] = 1.0;
  q.done[e] = done ? 1 : 0;
}

}  // namespace mz
