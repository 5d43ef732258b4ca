// mz_train_blocks.cuh -- what the fused training-step kernels (mz_train.cuh, mz_stoch_train.cuh) are made of: the
// argument block, the row-distributed layer primitives, the Linear(16)-elu-Linear stacks built from them, and the
// reduction that follows either kernel.
//
// Mapping (the search kernel's): one sample owns one DPP row of 16 lanes, feature k of a vector lives in
// lane k & 15 (slot k >> 4), four samples per wavefront.  That layout is ALSO the operand layout of
// v_mfma_f32_16x16x4_f32 with the sample index as its k dimension:
//     A[i][k] : lane 16 k + i holds x_i of sample k        B[k][j] : lane 16 k + j holds dy_j of sample k
// so one MFMA adds X^T dY of the wave's four samples into a 16 x 16 tile of a weight gradient, which stays
// in accumulator registers across samples and unroll steps.  Activations move through the layers as
// row-distributed fma chains (row_newbcast DPP), the weights sit in LDS with odd row strides so that both
// W[k][lane] (forward) and W[lane][n] (backward) are bank-conflict free.  Each wavefront writes its partial gradient
// to a workspace row; mz_train_reduce_kernel sums the rows in a fixed order (deterministic, no float atomics) and adds
// the L2 term.
//
// Every block states its operations in ONE order (fp contract off): a kernel that calls a block computes the bits of
// the block, whichever kernel it is.
#pragma once
#include "mz_spec.cuh"

#pragma clang fp contract(off)

namespace mz {

// THE argument block of a training step over NA weight arrays (18: the default MLP trio, 34: the stochastic family)
template <int NA>
struct TrainParamsT {
  const float* obs;     // [B][obs_dim] (batch.obs[:, 0]); the stochastic family: [B][L][obs_dim]
  const int32_t* act;   // [B][L]
  const float* rew;     // [B][L]
  const float* ret;     // [B][L]         (n-step returns Rn)
  const float* pi;      // [B][L][A]
  const float* w[NA];   // the arrays in the member order of the C ABI's weight struct
  int off[NA + 1];      // flat offsets of the arrays in the gradient vector; off[NA] = total
  int B, L, obs_dim, support;
  float loss_scale;     // 1/B (muax/loss.py) or 1/(B L) (coax variant)
  float l2;             // 1e-4
  float beta;           // weight of the VQ commitment term (read by the stochastic kernel only)
  float* ws;            // [waves][off[NA] + 1] partial gradients + partial loss
  float* grads;         // [off[NA]]
  float* loss;          // [1]
  int waves;
  const float* row_w;   // [B] per-row weight of the cross entropies (importance sampling), or null: all 1
};

constexpr int TRAIN_LDS_BYTES = 160 * 1024;  // one workgroup may take all of a CU's LDS

// ---- row-distributed linear layers on LDS weights ----
// y[n] = sum_k x[k] W[k][n] + b[n]
template <int K, int N>
MZ_DEV void lin_fwd(const float (&x)[(K + 15) / 16], const float* W, int j, float (&y)[(N + 15) / 16]) {
  constexpr int NS = (N + 15) / 16, LD = 16 * NS + 1;
#pragma unroll
  for (int t = 0; t < NS; ++t) y[t] = 0.0f;
  StaticFor<0, K>::run([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    const float xb = bcast<(k & 15)>(x[k >> 4]);
#pragma unroll
    for (int t = 0; t < NS; ++t) y[t] = __builtin_fmaf(xb, W[k * LD + j + 16 * t], y[t]);
  });
  const float* b = W + K * LD;
#pragma unroll
  for (int t = 0; t < NS; ++t) y[t] = y[t] + b[j + 16 * t];
}
// dx[k] = sum_n dy[n] W[k][n]
template <int K, int N>
MZ_DEV void lin_bwd(const float (&dy)[(N + 15) / 16], const float* W, int j, float (&dx)[(K + 15) / 16]) {
  constexpr int KS = (K + 15) / 16, LD = 16 * ((N + 15) / 16) + 1;
#pragma unroll
  for (int t = 0; t < KS; ++t) dx[t] = 0.0f;
  StaticFor<0, N>::run([&](auto nc) {
    constexpr int n = decltype(nc)::value;
    const float db = bcast<(n & 15)>(dy[n >> 4]);
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      const int k = j + 16 * t;
      dx[t] = __builtin_fmaf(db, W[(k < K ? k : 0) * LD + n], dx[t]);
    }
  });
#pragma unroll
  for (int t = 0; t < KS; ++t) dx[t] = (j + 16 * t < K) ? dx[t] : 0.0f;
}
// weight-gradient tiles: acc[kt][nt] += X^T dY over the wave's four samples
template <int KS, int NS>
MZ_DEV void grad_tiles(const float (&x)[KS], const float (&dy)[NS], f32x4 (&acc)[KS][NS]) {
#pragma unroll
  for (int kt = 0; kt < KS; ++kt)
#pragma unroll
    for (int nt = 0; nt < NS; ++nt)
      acc[kt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[kt], dy[nt], acc[kt][nt], 0, 0, 0);
}
template <int KS, int NS>
MZ_DEV void zero_tiles(f32x4 (&acc)[KS][NS]) {
#pragma unroll
  for (int kt = 0; kt < KS; ++kt)
#pragma unroll
    for (int nt = 0; nt < NS; ++nt) acc[kt][nt] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
}
// D tile layout of v_mfma_f32_16x16x4_f32: register v of lane l holds D[4 (l >> 4) + v][l & 15]
template <int KS, int NS>
MZ_DEV void store_tiles(const f32x4 (&acc)[KS][NS], float* dst, int K, int N, int lane) {
#pragma unroll
  for (int kt = 0; kt < KS; ++kt)
#pragma unroll
    for (int nt = 0; nt < NS; ++nt)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int k = 16 * kt + 4 * (lane >> 4) + v, n = 16 * nt + (lane & 15);
        if (k < K && n < N) dst[k * N + n] = acc[kt][nt][v];
      }
}
// sum of a per-row value over the wave's four rows (lanes of row 0 hold the result afterwards)
MZ_DEV float rows_sum(float v) {
  v = v + __shfl_xor(v, 16);
  v = v + __shfl_xor(v, 32);
  return v;
}
template <int NS>
MZ_DEV void store_bias(const float (&db)[NS], float* dst, int N, int lane) {
#pragma unroll
  for (int t = 0; t < NS; ++t) {
    const float s = rows_sum(db[t]);
    if (lane < 16 && lane + 16 * t < N) dst[lane + 16 * t] = s;
  }
}

template <int N>
MZ_DEV void elu_vec(float (&h)[N]) {
#pragma unroll
  for (int t = 0; t < N; ++t) h[t] = elu(h[t]);
}
// d elu / dh from a = elu(h): 1 for h > 0 (a > 0), exp(h) = a + 1 otherwise
MZ_DEV float elu_grad(float a) { return a > 0.0f ? 1.0f : a + 1.0f; }

// softmax probabilities and log-sum-exp of a row-distributed logit vector (lanes >= N: p = 0)
template <int N>
MZ_DEV void softmax_lse(const float (&x)[(N + 15) / 16], int j, float (&p)[(N + 15) / 16], float& lse) {
  constexpr int NS = (N + 15) / 16;
  float m = -INFINITY;
#pragma unroll
  for (int t = 0; t < NS; ++t) m = (j + 16 * t < N) ? fmaxf(m, x[t]) : m;
  m = row_max<4>(m);
  float part = 0.0f;
#pragma unroll
  for (int t = 0; t < NS; ++t) {
    p[t] = (j + 16 * t < N) ? exp_neg(x[t] - m) : 0.0f;
    part = part + p[t];
  }
  const float s = row_sum(part);
#pragma unroll
  for (int t = 0; t < NS; ++t) p[t] = p[t] / s;
  lse = m + log_pos(s);
}
// muax/utils.py:65-67,79-91: two-hot target of a scalar on the 2 S + 1 bins
template <int F>
MZ_DEV void support_target(float x, int support, int j, float (&t)[(F + 15) / 16]) {
  const float sg = x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f);
  float xs = sg * (__builtin_sqrtf(__builtin_fabsf(x) + 1.0f) - 1.0f) + 1e-3f * x;
  xs = fminf(fmaxf(xs, -(float)support), (float)support);
  const float lo = __builtin_floorf(xs), hi = __builtin_ceilf(xs);
  const float ph = xs - lo, pl = 1.0f - ph;
  const int ilo = (int)lo + support, ihi = (int)hi + support;
#pragma unroll
  for (int s = 0; s < (F + 15) / 16; ++s) {
    const int k = j + 16 * s;
    t[s] = (k == ilo ? pl : 0.0f) + (k == ihi ? ph : 0.0f);
  }
}
// cross entropy -sum t log_softmax(l) and its logit gradient (p sum(t) - t) * scale
template <int N>
MZ_DEV float ce_and_grad(const float (&l)[(N + 15) / 16], const float (&t)[(N + 15) / 16], int j, float scale,
                         float (&dl)[(N + 15) / 16]) {
  constexpr int NS = (N + 15) / 16;
  float p[NS], lse;
  softmax_lse<N>(l, j, p, lse);
  float pt = 0.0f, ptl = 0.0f;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const bool ok = j + 16 * s < N;
    pt = pt + (ok ? t[s] : 0.0f);
    ptl = ptl + (ok ? t[s] * l[s] : 0.0f);
  }
  const float T = row_sum(pt), TL = row_sum(ptl);
#pragma unroll
  for (int s = 0; s < NS; ++s) dl[s] = (j + 16 * s < N) ? (p[s] * T - t[s]) * scale : 0.0f;
  return T * lse - TL;
}

// muax/nn.py:37-44 forward, keeping what the backward needs
template <int E>
MZ_DEV void minmax_fwd(const float (&u)[(E + 15) / 16], int j, float (&s)[(E + 15) / 16], float& mn, float& mx,
                       float& c) {
  constexpr int ES = (E + 15) / 16;
  mn = INFINITY;
  mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < ES; ++t) {
    const bool ok = j + 16 * t < E;
    mn = ok ? fminf(mn, u[t]) : mn;
    mx = ok ? fmaxf(mx, u[t]) : mx;
  }
  mn = row_min<4>(mn);
  mx = row_max<4>(mx);
  c = mx - mn;
  c = c < 1e-5f ? c + 1e-5f : c;
#pragma unroll
  for (int t = 0; t < ES; ++t) s[t] = (j + 16 * t < E) ? (u[t] - mn) / c : 0.0f;
}
// gradient of s = (u - min u) / c, c = max u - min u (+1e-5 when tiny), w.r.t. u; ties of the min / max
// share their gradient evenly (jax's reduce_min / reduce_max rule)
template <int E>
MZ_DEV void minmax_bwd(const float (&g)[(E + 15) / 16], const float (&u)[(E + 15) / 16],
                       const float (&s)[(E + 15) / 16], float mn, float mx, float c, int j,
                       float (&du)[(E + 15) / 16]) {
  constexpr int ES = (E + 15) / 16;
  float pg = 0.0f, pgs = 0.0f, pmin = 0.0f, pmax = 0.0f;
#pragma unroll
  for (int t = 0; t < ES; ++t) {
    const bool ok = j + 16 * t < E;
    pg = pg + (ok ? g[t] : 0.0f);
    pgs = pgs + (ok ? g[t] * s[t] : 0.0f);
    pmin = pmin + ((ok && u[t] == mn) ? 1.0f : 0.0f);
    pmax = pmax + ((ok && u[t] == mx) ? 1.0f : 0.0f);
  }
  const float sg = row_sum(pg), sgs = row_sum(pgs), nmin = row_sum(pmin), nmax = row_sum(pmax);
  const float dmax = -sgs / c;          // through c
  const float dmin = (sgs - sg) / c;    // through the numerator and through c
#pragma unroll
  for (int t = 0; t < ES; ++t) {
    const bool ok = j + 16 * t < E;
    float d = g[t] / c;
    d = d + ((u[t] == mn) ? dmin / nmin : 0.0f);
    d = d + ((u[t] == mx) ? dmax / nmax : 0.0f);
    du[t] = ok ? d : 0.0f;
  }
}

// index of the largest of the C logits of a row, the lowest index among equal maxima
template <int C>
MZ_DEV int argmax_first(const float (&e)[(C + 15) / 16], int j) {
  float best = -INFINITY, bi = 1024.0f;
#pragma unroll
  for (int t = 0; t < (C + 15) / 16; ++t) {
    const bool up = (j + 16 * t < C) && e[t] > best;
    best = up ? e[t] : best;
    bi = up ? (float)(j + 16 * t) : bi;
  }
  const float m = row_max<4>(best);
  const int c = (int)row_min<4>(best == m ? bi : 1024.0f);
  return c < C ? c : 0;
}

// x = [v, onehot(a)] as a row-distributed vector of E + N elements.  (The one liberty of the stochastic kernel lives
// here: its chance dynamics read this EXACT one-hot of the code where torch computes e + (onehot - e) in floating point.)
template <int E, int N>
MZ_DEV void concat_onehot(const float (&v)[(E + 15) / 16], int a, int j, float (&x)[(E + N + 15) / 16]) {
#pragma unroll
  for (int t = 0; t < (E + N + 15) / 16; ++t) {
    const int k = j + 16 * t;
    float s = 0.0f;
    if (t < (E + 15) / 16) s = (k < E) ? v[t] : 0.0f;
    x[t] = (k >= E && k < E + N) ? ((k - E == a) ? 1.0f : 0.0f) : s;
  }
}

// ---- Linear(16)-elu-Linear stacks.  Each is forward, then backward from the output to the hidden layer, in this
// order: layer-2 tiles and bias sums, lin_bwd through W2, the elu, layer-1 tiles and bias sum ----
// One stack under a cross entropy: forward from x, CE(logits, t) into the return value, both layers' gradient tiles and
// bias sums, and dh, the gradient at the hidden layer's pre-activation (the caller takes it back through W1 to whichever
// inputs it needs).
template <int K, int N>
MZ_DEV float head_ce(const float (&x)[(K + 15) / 16], const float* W1, const float* W2, const float (&t)[(N + 15) / 16],
                     int j, float scale, f32x4 (&g1)[(K + 15) / 16][1], float (&b1)[1], f32x4 (&g2)[1][(N + 15) / 16],
                     float (&b2)[(N + 15) / 16], float (&dh)[1]) {
  constexpr int NS = (N + 15) / 16;
  float h[1], l[NS], dl[NS];
  lin_fwd<K, 16>(x, W1, j, h);
  elu_vec(h);
  lin_fwd<16, N>(h, W2, j, l);
  const float ce = ce_and_grad<N>(l, t, j, scale, dl);
  grad_tiles(h, dl, g2);
#pragma unroll
  for (int s = 0; s < NS; ++s) b2[s] = b2[s] + dl[s];
  lin_bwd<16, N>(dl, W2, j, dh);
  dh[0] = dh[0] * elu_grad(h[0]);
  grad_tiles(x, dh, g1);
  b1[0] = b1[0] + dh[0];
  return ce;
}

// One stack under min_max_normalize: forward from x (the normalised output is re-evaluated, not read back), the gradient
// g of the output taken through the normaliser and both layers; dh as in head_ce.
template <int K, int E>
MZ_DEV void state_bwd(const float (&x)[(K + 15) / 16], const float* W1, const float* W2, const float (&g)[(E + 15) / 16],
                      int j, f32x4 (&g1)[(K + 15) / 16][1], float (&b1)[1], f32x4 (&g2)[1][(E + 15) / 16],
                      float (&b2)[(E + 15) / 16], float (&dh)[1]) {
  constexpr int ES = (E + 15) / 16;
  float h[1], u[ES], s[ES], du[ES], mn, mx, c;
  lin_fwd<K, 16>(x, W1, j, h);
  elu_vec(h);
  lin_fwd<16, E>(h, W2, j, u);
  minmax_fwd<E>(u, j, s, mn, mx, c);
  minmax_bwd<E>(g, u, s, mn, mx, c, j, du);
  grad_tiles(h, du, g2);
#pragma unroll
  for (int t = 0; t < ES; ++t) b2[t] = b2[t] + du[t];
  lin_bwd<16, E>(du, W2, j, dh);
  dh[0] = dh[0] * elu_grad(h[0]);
  grad_tiles(x, dh, g1);
  b1[0] = b1[0] + dh[0];
}

template <int K, int E>
MZ_DEV void state_fwd(const float (&x)[(K + 15) / 16], const float* W1, const float* W2, int j, float (&s)[(E + 15) / 16]) {
  float h[1], u[(E + 15) / 16], mn, mx, c;
  lin_fwd<K, 16>(x, W1, j, h);
  elu_vec(h);
  lin_fwd<16, E>(h, W2, j, u);
  minmax_fwd<E>(u, j, s, mn, mx, c);
}

// Second launch of a training step: the fixed-order sum of the per-wavefront partials, plus the L2 term
// 1e-4 * 0.5 * sum w^2 (muax/loss.py:84-87).
template <int NA>
__global__ __launch_bounds__(256) void mz_train_reduce_kernel(const TrainParamsT<NA> p) {
  // block = 32 gradient entries x 8 groups of workspace rows; partials meet in LDS in a fixed order
  const int NP = p.off[NA];
  __shared__ float red[256];
  const int pl = threadIdx.x & 31, q = threadIdx.x >> 5;
  const int idx = blockIdx.x * 32 + pl;
  const int per = (p.waves + 7) / 8;
  const int w0 = q * per, w1 = min(p.waves, w0 + per);
  float acc = 0.0f;
  if (idx < NP) {
    const float* src = p.ws + idx;
    int w = w0;
    for (; w + 8 <= w1; w += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = src[(size_t)(w + u) * (NP + 1)];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc = acc + v[u];
    }
    for (; w < w1; ++w) acc = acc + src[(size_t)w * (NP + 1)];
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  if (q == 0 && idx < NP) {
    float t = red[pl];
#pragma unroll
    for (int g = 1; g < 8; ++g) t = t + red[32 * g + pl];
    int a = 0;
    while (idx >= p.off[a + 1]) ++a;
    p.grads[idx] = t + p.l2 * p.w[a][idx - p.off[a]];
  }
  if (blockIdx.x == gridDim.x - 1) {  // loss: partial sums of every wavefront + 0.5 l2 sum w^2
    __syncthreads();
    float la = 0.0f;
    for (int w = threadIdx.x; w < p.waves; w += 256) la = la + p.ws[(size_t)w * (NP + 1) + NP];
    float sq = 0.0f;
    for (int a = 0; a < NA; ++a)
      for (int i = threadIdx.x; i < p.off[a + 1] - p.off[a]; i += 256) sq = __builtin_fmaf(p.w[a][i], p.w[a][i], sq);
    red[threadIdx.x] = la + 0.5f * p.l2 * sq;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) p.loss[0] = red[0];
  }
}

}  // namespace mz
