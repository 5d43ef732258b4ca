// mz_env.cuh -- vector environments stepped on the device ("Device environments").
//
// Three environments.  Acrobot and MountainCar are in the second half of this file; first the cart-pole of
// examples/cartpole_env.py (Barto, Sutton, Anderson 1983; explicit Euler at
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

// ---- the two other discrete classic-control tasks: Acrobot and MountainCar (mzs_env_classic_*) ----
// The same conventions: one thread per environment, fp64 operation by operation in the order of the host restatements
// (tests/acrobot_reference.py, tests/mountaincar_reference.py), state read and written as double2 (state: 16-byte
// aligned), auto-reset inside the step launch, start states from env_uniform53.  With C drawn components, component c
// of environment e's d-th draw is  lo_c + width_c * u53(key, e, C d + c):
//   Acrobot      state (th1, th2, dth1, dth2), all four drawn: -0.1 + 0.2 u          (C = 4)
//   MountainCar  state (x, v), x = -0.6 + 0.2 u, v = 0                               (C = 1)
// obs is stored as float2 -- three per Acrobot (cos th1, sin th1 | cos th2, sin th2 | dth1, dth2; 24 bytes per
// environment), one per MountainCar ((float)x, (float)v) -- so obs_out must be 8-BYTE aligned for both kinds, which is
// what the host entries demand and refuse.
constexpr int kEnvAcrobot = 1, kEnvMountainCar = 2;  // = MZS_ENV_ACROBOT, MZS_ENV_MOUNTAINCAR
constexpr int kEnvWrapMax = 64;  // +-2 pi at most this often each way (see wrap_pi)

struct EnvClassic {
  int N, max_steps;
  uint32_t key0, key1;
  double* state;              // [N, 4] (Acrobot) or [N, 2] (MountainCar), 16-byte aligned
  int32_t* t;                 // [N] steps of the open episode
  int32_t* draws;             // [N] start states drawn so far
};

struct EnvClassicStepArgs {
  EnvClassic env;
  const int32_t* a;           // [N]
  float* obs;                 // [N, 6] or [N, 2] (8-byte aligned)
  double* r;                  // [N]
  uint8_t* done;              // [N]
};

constexpr double kPi = 3.141592653589793;

// ---- Acrobot (Sutton & Barto's "book" equations, Gym's Acrobot-v1) ----
constexpr double kAcM1 = 1.0, kAcM2 = 1.0, kAcL1 = 1.0, kAcLc1 = 0.5, kAcLc2 = 0.5, kAcI1 = 1.0, kAcI2 = 1.0, kAcG = 9.8;
constexpr double kAcDt = 0.2, kAcMaxVel1 = 4 * kPi, kAcMaxVel2 = 9 * kPi;

MZ_DEV void acrobot_draw(const EnvClassic& p, int e, int d, double (&s)[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c)
    s[c] = -0.1 + 0.2 * env_uniform53(p.key0, p.key1, (uint32_t)e, 4u * (uint32_t)d + (uint32_t)c);
}

MZ_DEV void acrobot_put(const EnvClassic& p, int e, const double (&s)[4], float* obs) {
  double2* st = reinterpret_cast<double2*>(p.state) + 2 * (size_t)e;
  st[0] = make_double2(s[0], s[1]);
  st[1] = make_double2(s[2], s[3]);
  float2* o = reinterpret_cast<float2*>(obs) + 3 * (size_t)e;
  o[0] = make_float2((float)cos(s[0]), (float)sin(s[0]));
  o[1] = make_float2((float)cos(s[1]), (float)sin(s[1]));
  o[2] = make_float2((float)s[2], (float)s[3]);
}

// d/dt of (th1, th2, dth1, dth2) under torque `a`
MZ_DEV void acrobot_dsdt(const double (&s)[4], double a, double (&k)[4]) {
  const double th1 = s[0], th2 = s[1], dth1 = s[2], dth2 = s[3];
  const double c2 = cos(th2), s2 = sin(th2);
  const double d1 = kAcM1 * kAcLc1 * kAcLc1 + kAcM2 * (kAcL1 * kAcL1 + kAcLc2 * kAcLc2 + 2.0 * kAcL1 * kAcLc2 * c2) + kAcI1 + kAcI2;
  const double d2 = kAcM2 * (kAcLc2 * kAcLc2 + kAcL1 * kAcLc2 * c2) + kAcI2;
  const double phi2 = kAcM2 * kAcLc2 * kAcG * cos(th1 + th2 - kPi / 2.0);
  const double phi1 = -kAcM2 * kAcL1 * kAcLc2 * dth2 * dth2 * s2 - 2.0 * kAcM2 * kAcL1 * kAcLc2 * dth2 * dth1 * s2 +
                      (kAcM1 * kAcLc1 + kAcM2 * kAcL1) * kAcG * cos(th1 - kPi / 2.0) + phi2;
  const double ddth2 = (a + d2 / d1 * phi1 - kAcM2 * kAcL1 * kAcLc2 * dth1 * dth1 * s2 - phi2) /
                       (kAcM2 * kAcLc2 * kAcLc2 + kAcI2 - d2 * d2 / d1);
  const double ddth1 = -(d2 * ddth2 + phi1) / d1;
  k[0] = dth1; k[1] = dth2; k[2] = ddth1; k[3] = ddth2;
}

// Into [-pi, pi] by repeated -+2 pi, each way at most kEnvWrapMax times: a step from a wrapped state with clamped
// velocities needs a handful, and an angle a caller uploaded that is infinite or beyond 2^55 (where x - 2 pi == x)
// leaves the loop after 64 rounds instead of keeping the launch running for ever.
MZ_DEV double wrap_pi(double x) {
  constexpr double two_pi = kPi - (-kPi);
  for (int i = 0; i < kEnvWrapMax && x > kPi; ++i) x = x - two_pi;
  for (int i = 0; i < kEnvWrapMax && x < -kPi; ++i) x = x + two_pi;
  return x;
}

MZ_DEV double bound(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

__global__ void __launch_bounds__(kEnvThreads) env_acrobot_reset_kernel(EnvClassic p, float* obs) {
  const int e = blockIdx.x * kEnvThreads + threadIdx.x;
  if (e >= p.N) return;
  const int d = p.draws[e];
  double s[4];
  acrobot_draw(p, e, d, s);
  acrobot_put(p, e, s, obs);
  p.t[e] = 0;
  p.draws[e] = d + 1;
}

__global__ void __launch_bounds__(kEnvThreads) env_acrobot_step_kernel(EnvClassicStepArgs q) {
  const EnvClassic& p = q.env;
  const int e = blockIdx.x * kEnvThreads + threadIdx.x;
  if (e >= p.N) return;
  const double2* st = reinterpret_cast<const double2*>(p.state) + 2 * (size_t)e;
  const double2 s01 = st[0], s23 = st[1];
  const double y0[4] = {s01.x, s01.y, s23.x, s23.y};
  const int ai = q.a[e];
  const double a = ai <= 0 ? -1.0 : (ai >= 2 ? 1.0 : 0.0);
  // one classical Runge-Kutta step of dt (Gym's rk4 over [0, dt])
  constexpr double dt2 = kAcDt / 2.0, dt6 = kAcDt / 6.0;
  double k1[4], k2[4], k3[4], k4[4], y[4];
  acrobot_dsdt(y0, a, k1);
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = y0[i] + dt2 * k1[i];
  acrobot_dsdt(y, a, k2);
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = y0[i] + dt2 * k2[i];
  acrobot_dsdt(y, a, k3);
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = y0[i] + kAcDt * k3[i];
  acrobot_dsdt(y, a, k4);
  double ns[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) ns[i] = y0[i] + dt6 * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]);
  ns[0] = wrap_pi(ns[0]);
  ns[1] = wrap_pi(ns[1]);
  ns[2] = bound(ns[2], -kAcMaxVel1, kAcMaxVel1);
  ns[3] = bound(ns[3], -kAcMaxVel2, kAcMaxVel2);
  const bool terminated = -cos(ns[0]) - cos(ns[0] + ns[1]) > 1.0;
  int t = p.t[e] + 1;
  const bool done = terminated || t >= p.max_steps;
  if (done) {
    const int d = p.draws[e];
    acrobot_draw(p, e, d, ns);
    p.draws[e] = d + 1;
    t = 0;
  }
  acrobot_put(p, e, ns, q.obs);
  p.t[e] = t;
  q.r[e] = terminated ? 0.0 : -1.0;
  q.done[e] = done ? 1 : 0;
}

// ---- MountainCar (Gym's MountainCar-v0 in fp64) ----
constexpr double kMcMinX = -1.2, kMcMaxX = 0.6, kMcMaxV = 0.07, kMcGoalX = 0.5, kMcGoalV = 0.0;
constexpr double kMcForce = 0.001, kMcGravity = 0.0025;

MZ_DEV void mountaincar_draw(const EnvClassic& p, int e, int d, double (&s)[2]) {
  s[0] = -0.6 + 0.2 * env_uniform53(p.key0, p.key1, (uint32_t)e, (uint32_t)d);
  s[1] = 0.0;
}

MZ_DEV void mountaincar_put(const EnvClassic& p, int e, const double (&s)[2], float* obs) {
  reinterpret_cast<double2*>(p.state)[e] = make_double2(s[0], s[1]);
  reinterpret_cast<float2*>(obs)[e] = make_float2((float)s[0], (float)s[1]);
}

__global__ void __launch_bounds__(kEnvThreads) env_mountaincar_reset_kernel(EnvClassic p, float* obs) {
  const int e = blockIdx.x * kEnvThreads + threadIdx.x;
  if (e >= p.N) return;
  const int d = p.draws[e];
  double s[2];
  mountaincar_draw(p, e, d, s);
  mountaincar_put(p, e, s, obs);
  p.t[e] = 0;
  p.draws[e] = d + 1;
}

__global__ void __launch_bounds__(kEnvThreads) env_mountaincar_step_kernel(EnvClassicStepArgs q) {
  const EnvClassic& p = q.env;
  const int e = blockIdx.x * kEnvThreads + threadIdx.x;
  if (e >= p.N) return;
  const double2 s = reinterpret_cast<const double2*>(p.state)[e];
  double x = s.x, v = s.y;
  const int ai = q.a[e];
  const int a = ai <= 0 ? 0 : (ai >= 2 ? 2 : ai);
  v = v + ((double)(a - 1) * kMcForce + cos(3.0 * x) * (-kMcGravity));
  v = bound(v, -kMcMaxV, kMcMaxV);
  x = x + v;
  x = bound(x, kMcMinX, kMcMaxX);
  if (x == kMcMinX && v < 0.0) v = 0.0;
  const bool terminated = x >= kMcGoalX && v >= kMcGoalV;
  int t = p.t[e] + 1;
  const bool done = terminated || t >= p.max_steps;
  double ns[2] = {x, v};
  if (done) {
    const int d = p.draws[e];
    mountaincar_draw(p, e, d, ns);
    p.draws[e] = d + 1;
    t = 0;
  }
  mountaincar_put(p, e, ns, q.obs);
  p.t[e] = t;
  q.r[e] = -1.0;
  q.done[e] = done ? 1 : 0;
}

}  // namespace mz
