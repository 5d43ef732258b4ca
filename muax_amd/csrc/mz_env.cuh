// mz_env.cuh -- vector environments stepped on the device ("Device environments").
//
// Three environments -- CartPole, Acrobot, MountainCar -- on ONE skeleton.  Two kernel templates, one thread per
// environment, vector stores only:
//   env_reset_kernel<D>  every environment draws a start state, t = 0, obs from the state
//   env_step_kernel<D>   D's step in fp64, operation by operation in the order of the host restatement; a finished
//                        environment draws its next start state in the same launch, so obs is already the next
//                        episode's first one
// An environment D is a struct of static members that supplies what differs: the state width kState, the draw constants
// (kDrawn, kLo, kWidth), advance(state, action, new_state, terminated), reward(terminated) and store_obs.  The state is
// read and written as double2 (state: 16-byte aligned).
// The start state of environment e, its d-th draw (d = draws[e], which then grows by one): with C = kDrawn drawn
// components, component c < C is
//   state[c] = lo + width * u53(key, e, C d + c)      u53 = ((y0 << 32 | y1) >> 11) * 2^-53 of threefry2x32
// and every other component is 0:
//   CartPole     state (x, x_dot, theta, theta_dot), all four drawn: -0.05 + 0.1 u    (C = 4)
//   Acrobot      state (th1, th2, dth1, dth2), all four drawn: -0.1 + 0.2 u           (C = 4)
//   MountainCar  state (x, v), x = -0.6 + 0.2 u, v = 0                                (C = 1)
// u53 is the replay sampler's uniform (mz_replay.cuh): no libm call, so a draw is reproducible on the host bit for bit.
// The steps themselves call the device's fp64 sin and cos, which agree with a host libm to the last bits only.  The
// units are built with -ffp-contract=off: no multiply-add is fused.
// The width of an environment's observation store decides the alignment the host entries demand of obs_out, and refuse:
// the cart-pole's one float4 16 bytes; float2 -- three per Acrobot (cos th1, sin th1 | cos th2, sin th2 | dth1, dth2; 24
// bytes per environment), one per MountainCar ((float)x, (float)v) -- 8 BYTES for both kinds of mzs_env_classic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mz_spec.cuh"

#pragma clang fp contract(off)

namespace mz {

constexpr int kEnvThreads = 256;
constexpr int kEnvWrapMax = 64;  // +-2 pi at most this often each way (see wrap_pi)

struct Env {
  int N, max_steps;
  uint32_t key0, key1;
  double* state;              // [N, kState] (16-byte aligned)
  int32_t* t;                 // [N] steps of the open episode
  int32_t* draws;             // [N] start states drawn so far
};

struct EnvStepArgs {
  Env env;
  const int32_t* a;           // [N]
  float* obs;                 // [N, obs_dim] (aligned to the environment's observation store)
  double* r;                  // [N]
  uint8_t* done;              // [N]
};

// (y0 << 32 | y1) >> 11 of one threefry block, as a double in [0, 1): mz_replay.cuh's uniform53
MZ_DEV double env_uniform53(uint32_t k0, uint32_t k1, uint32_t x0, uint32_t x1) {
  threefry2x32(k0, k1, x0, x1);
  const unsigned long long bits = (((unsigned long long)x0 << 32) | x1) >> 11;
  return (double)bits * 0x1p-53;
}

// ---- the skeleton ----
template <class D>
MZ_DEV void env_draw(const Env& p, int e, int d, double (&s)[D::kState]) {
#pragma unroll
  for (int c = 0; c < D::kState; ++c)
    s[c] = c < D::kDrawn ? D::kLo + D::kWidth * env_uniform53(p.key0, p.key1, (uint32_t)e,
                                                             (uint32_t)D::kDrawn * (uint32_t)d + (uint32_t)c)
                         : 0.0;
}

template <class D>
MZ_DEV void env_put(const Env& p, int e, const double (&s)[D::kState], float* obs) {
  double2* st = reinterpret_cast<double2*>(p.state) + (D::kState / 2) * (size_t)e;
#pragma unroll
  for (int i = 0; i < D::kState / 2; ++i) st[i] = make_double2(s[2 * i], s[2 * i + 1]);
  D::store_obs(s, e, obs);
}

template <class D>
__global__ void __launch_bounds__(kEnvThreads) env_reset_kernel(Env p, float* obs) {
  const int e = blockIdx.x * kEnvThreads + threadIdx.x;
  if (e >= p.N) return;
  const int d = p.draws[e];
  double s[D::kState];
  env_draw<D>(p, e, d, s);
  env_put<D>(p, e, s, obs);
  p.t[e] = 0;
  p.draws[e] = d + 1;
}

template <class D>
__global__ void __launch_bounds__(kEnvThreads) env_step_kernel(EnvStepArgs q) {
  const Env& p = q.env;
  const int e = blockIdx.x * kEnvThreads + threadIdx.x;
  if (e >= p.N) return;
  const double2* st = reinterpret_cast<const double2*>(p.state) + (D::kState / 2) * (size_t)e;
  double s[D::kState], ns[D::kState];
#pragma unroll
  for (int i = 0; i < D::kState / 2; ++i) {
    const double2 v = st[i];
    s[2 * i] = v.x;
    s[2 * i + 1] = v.y;
  }
  bool terminated;
  D::advance(s, q.a[e], ns, terminated);
  int t = p.t[e] + 1;
  const bool done = terminated || t >= p.max_steps;
  if (done) {
    const int d = p.draws[e];
    env_draw<D>(p, e, d, ns);
    p.draws[e] = d + 1;
    t = 0;
  }
  env_put<D>(p, e, ns, q.obs);
  p.t[e] = t;
  q.r[e] = D::reward(terminated);
  q.done[e] = done ? 1 : 0;
}

// ---- the cart-pole of examples/cartpole_env.py (Barto, Sutton, Anderson 1983; explicit Euler at 50 Hz, reward 1 per
// step, the episode ends when |x| > 2.4 or |theta| > 12 degrees or after max_episode_steps steps) ----
struct CartPole {
  static constexpr int kState = 4, kDrawn = 4, kObsAlign = 16;  // store_obs: one float4
  static constexpr double kLo = -0.05, kWidth = 0.1;

  // VectorCartPole.step: force +10 where a == 1, -10 for anything else
  static MZ_DEV void advance(const double (&s0)[4], int a, double (&ns)[4], bool& terminated) {
    constexpr double kGravity = 9.8, kMCart = 1.0, kMPole = 0.1, kHalfLen = 0.5, kForce = 10.0, kDt = 0.02;
    constexpr double kXLimit = 2.4, kThetaLimit = 12 * 2 * 3.141592653589793 / 360;  // (the host's expression)
    constexpr double m_total = kMCart + kMPole, pm_l = kMPole * kHalfLen;
    double x = s0[0], x_dot = s0[1], th = s0[2], th_dot = s0[3];
    const double f = a == 1 ? kForce : -kForce;
    const double c = cos(th), s = sin(th);
    const double tmp = (f + pm_l * th_dot * th_dot * s) / m_total;
    const double th_acc = (kGravity * s - c * tmp) / (kHalfLen * (4.0 / 3.0 - kMPole * c * c / m_total));
    const double x_acc = tmp - pm_l * th_acc * c / m_total;
    x = x + kDt * x_dot;
    x_dot = x_dot + kDt * x_acc;
    th = th + kDt * th_dot;
    th_dot = th_dot + kDt * th_acc;
    terminated = fabs(x) > kXLimit || fabs(th) > kThetaLimit;
    ns[0] = x; ns[1] = x_dot; ns[2] = th; ns[3] = th_dot;
  }

  static MZ_DEV double reward(bool) { return 1.0; }

  static MZ_DEV void store_obs(const double (&s)[4], int e, float* obs) {
    reinterpret_cast<float4*>(obs)[e] = make_float4((float)s[0], (float)s[1], (float)s[2], (float)s[3]);
  }
};

constexpr double kPi = 3.141592653589793;

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

// ---- Acrobot (Sutton & Barto's "book" equations, Gym's Acrobot-v1; tests/acrobot_reference.py) ----
struct Acrobot {
  static constexpr int kState = 4, kDrawn = 4, kObsAlign = 8;  // store_obs: three float2
  static constexpr double kLo = -0.1, kWidth = 0.2;
  static constexpr double kM1 = 1.0, kM2 = 1.0, kL1 = 1.0, kLc1 = 0.5, kLc2 = 0.5, kI1 = 1.0, kI2 = 1.0, kG = 9.8;
  static constexpr double kDt = 0.2, kMaxVel1 = 4 * kPi, kMaxVel2 = 9 * kPi;

  // d/dt of (th1, th2, dth1, dth2) under torque `a`
  static MZ_DEV void dsdt(const double (&s)[4], double a, double (&k)[4]) {
    const double th1 = s[0], th2 = s[1], dth1 = s[2], dth2 = s[3];
    const double c2 = cos(th2), s2 = sin(th2);
    const double d1 = kM1 * kLc1 * kLc1 + kM2 * (kL1 * kL1 + kLc2 * kLc2 + 2.0 * kL1 * kLc2 * c2) + kI1 + kI2;
    const double d2 = kM2 * (kLc2 * kLc2 + kL1 * kLc2 * c2) + kI2;
    const double phi2 = kM2 * kLc2 * kG * cos(th1 + th2 - kPi / 2.0);
    const double phi1 = -kM2 * kL1 * kLc2 * dth2 * dth2 * s2 - 2.0 * kM2 * kL1 * kLc2 * dth2 * dth1 * s2 +
                        (kM1 * kLc1 + kM2 * kL1) * kG * cos(th1 - kPi / 2.0) + phi2;
    const double ddth2 = (a + d2 / d1 * phi1 - kM2 * kL1 * kLc2 * dth1 * dth1 * s2 - phi2) /
                         (kM2 * kLc2 * kLc2 + kI2 - d2 * d2 / d1);
    const double ddth1 = -(d2 * ddth2 + phi1) / d1;
    k[0] = dth1; k[1] = dth2; k[2] = ddth1; k[3] = ddth2;
  }

  // action <= 0 is torque -1, 1 is 0, >= 2 is +1
  static MZ_DEV void advance(const double (&y0)[4], int ai, double (&ns)[4], bool& terminated) {
    const double a = ai <= 0 ? -1.0 : (ai >= 2 ? 1.0 : 0.0);
    // one classical Runge-Kutta step of dt (Gym's rk4 over [0, dt])
    constexpr double dt2 = kDt / 2.0, dt6 = kDt / 6.0;
    double k1[4], k2[4], k3[4], k4[4], y[4];
    dsdt(y0, a, k1);
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = y0[i] + dt2 * k1[i];
    dsdt(y, a, k2);
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = y0[i] + dt2 * k2[i];
    dsdt(y, a, k3);
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = y0[i] + kDt * k3[i];
    dsdt(y, a, k4);
#pragma unroll
    for (int i = 0; i < 4; ++i) ns[i] = y0[i] + dt6 * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]);
    ns[0] = wrap_pi(ns[0]);
    ns[1] = wrap_pi(ns[1]);
    ns[2] = bound(ns[2], -kMaxVel1, kMaxVel1);
    ns[3] = bound(ns[3], -kMaxVel2, kMaxVel2);
    terminated = -cos(ns[0]) - cos(ns[0] + ns[1]) > 1.0;
  }

  static MZ_DEV double reward(bool terminated) { return terminated ? 0.0 : -1.0; }

  static MZ_DEV void store_obs(const double (&s)[4], int e, float* obs) {
    float2* o = reinterpret_cast<float2*>(obs) + 3 * (size_t)e;
    o[0] = make_float2((float)cos(s[0]), (float)sin(s[0]));
    o[1] = make_float2((float)cos(s[1]), (float)sin(s[1]));
    o[2] = make_float2((float)s[2], (float)s[3]);
  }
};

// ---- MountainCar (Gym's MountainCar-v0 in fp64; tests/mountaincar_reference.py) ----
struct MountainCar {
  static constexpr int kState = 2, kDrawn = 1, kObsAlign = 8;  // store_obs: one float2
  static constexpr double kLo = -0.6, kWidth = 0.2;
  static constexpr double kMinX = -1.2, kMaxX = 0.6, kMaxV = 0.07, kGoalX = 0.5, kGoalV = 0.0;
  static constexpr double kForce = 0.001, kGravity = 0.0025;

  // the action is clamped to 0..2
  static MZ_DEV void advance(const double (&s)[2], int ai, double (&ns)[2], bool& terminated) {
    double x = s[0], v = s[1];
    const int a = ai <= 0 ? 0 : (ai >= 2 ? 2 : ai);
    v = v + ((double)(a - 1) * kForce + cos(3.0 * x) * (-kGravity));
    v = bound(v, -kMaxV, kMaxV);
    x = x + v;
    x = bound(x, kMinX, kMaxX);
    if (x == kMinX && v < 0.0) v = 0.0;
    terminated = x >= kGoalX && v >= kGoalV;
    ns[0] = x; ns[1] = v;
  }

  static MZ_DEV double reward(bool) { return -1.0; }

  static MZ_DEV void store_obs(const double (&s)[2], int e, float* obs) {
    reinterpret_cast<float2*>(obs)[e] = make_float2((float)s[0], (float)s[1]);
  }
};

}  // namespace mz
