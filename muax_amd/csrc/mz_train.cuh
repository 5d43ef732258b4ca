// mz_train.cuh -- fused forward + backward of the k-step unrolled MuZero loss for the default MLP trio
// (muax/loss.py:10-88 through jax.value_and_grad at muax/model.py:245-249).
//
// The mapping (one sample per DPP row of 16 lanes, four per wavefront, weights in LDS, gradient tiles in MFMA
// accumulators), the argument block, the layer primitives and the reduction are mz_train_blocks.cuh's; this file is
// the graph of the trio: TrainCfg (the LDS plan of an (A, E, F) instance) and mz_train_kernel.
//
// Sweep 1 walks s_0 -> s_1 -> ... -> s_{L-1} through the dynamics' next-state branch only and keeps the
// L hidden states in LDS (64 ES bytes per sample and step).  Sweep 2 goes back from step L-1 to 0: it
// re-evaluates the step's four heads from the kept state, adds the three cross entropies to the loss and
// back-propagates, halving the state gradient that comes back through the dynamics (Appendix G,
// muax/loss.py:60-61).  Within a step the order is: next-state branch, reward head, the halving, value head, policy
// head.  Each wavefront writes its partial gradient to a workspace row for mz_train_reduce_kernel<18>.
//
// This is a floating-point kernel: its check is torch autograd on the same formula (tests), tolerance
// in the test, not the bit-exact oracle of the search path.
#pragma once
#include "mz_train_blocks.cuh"

#pragma clang fp contract(off)

namespace mz {

using TrainParams = TrainParamsT<18>;  // MLP_WEIGHT order: repr_w, repr_b, pv_w1, pv_b1, pv_w2, pv_b2, pp_*, dr_*, dn_*

template <int A_, int E_, int F_>
struct TrainCfg {
  static constexpr int A = A_, E = E_, F = F_, H = 16, X = E_ + A_;
  static constexpr int ES = (E + 15) / 16, FS = (F + 15) / 16, XS = (X + 15) / 16, AS = (A + 15) / 16;
  static constexpr int NA = 18;                      // weight arrays
  static constexpr const char* DIMS = "(A, E, F)";   // what an instance is named by, for the launcher's refusal
  // The listed instances and the narrow on-demand ones keep the policy head in one slot; a translation unit built
  // with -DMZ_TRAIN_WIDE=1 (muax_amd/_jit.py::ensure_wide_train_instance) spreads it over AS <= 4 slots.
#if defined(MZ_TRAIN_WIDE) && MZ_TRAIN_WIDE
  static constexpr bool WIDE = true;
  static_assert(A <= 64, "policy head in at most four slots");
#else
  static constexpr bool WIDE = false;
  static_assert(A <= 16, "policy head in one slot");
#endif
  static constexpr int ld(int n) { return 16 * ((n + 15) / 16) + 1; }  // odd, zero padded
  // LDS weight blocks: [K][ld(N)] then the bias padded to a multiple of 16
  static constexpr int blk(int k, int n) { return k * ld(n) + 16 * ((n + 15) / 16); }
  static constexpr int PV1 = 0;
  static constexpr int PV2 = PV1 + blk(E, H);
  static constexpr int PP1 = PV2 + blk(H, F);
  static constexpr int PP2 = PP1 + blk(E, H);
  static constexpr int DR1 = PP2 + blk(H, A);
  static constexpr int DR2 = DR1 + blk(X, H);
  static constexpr int DN1 = DR2 + blk(H, F);
  static constexpr int DN2 = DN1 + blk(X, H);
  static constexpr int WEIGHT_WORDS = ((DN2 + blk(H, E) + 3) / 4) * 4;
  static constexpr int CK_WORDS_PER_STEP = 16 * 16 * ES;  // 16 samples per workgroup
  // dynamic LDS of a workgroup (weights + L kept states) is at most TRAIN_LDS_BYTES: the longest unroll it admits
  static constexpr int MAX_UNROLL = (TRAIN_LDS_BYTES / 4 - WEIGHT_WORDS) / CK_WORDS_PER_STEP;
};

template <class C>
__global__ __launch_bounds__(256) void mz_train_kernel(const TrainParams p) {
  constexpr int A = C::A, E = C::E, F = C::F, H = C::H, X = C::X;
  constexpr int ES = C::ES, FS = C::FS, XS = C::XS, AS = C::AS;
  extern __shared__ float lds[];
  const int tid = threadIdx.x, lane = tid & 63, j = tid & 15;
  const int row = tid >> 4;

  // ---- weights -> LDS, [K][ld(N)] blocks with zero padding, bias behind each block ----
  for (int i = tid; i < C::WEIGHT_WORDS; i += 256) lds[i] = 0.0f;
  __syncthreads();
  {
    const int Ks[8] = {E, H, E, H, X, H, X, H};
    const int Ns[8] = {H, F, H, A, H, F, H, E};
    const int Os[8] = {C::PV1, C::PV2, C::PP1, C::PP2, C::DR1, C::DR2, C::DN1, C::DN2};
    for (int l = 0; l < 8; ++l) {
      const int K = Ks[l], N = Ns[l], LD = 16 * ((N + 15) / 16) + 1;
      const float* W = p.w[2 + 2 * l];
      const float* Bv = p.w[3 + 2 * l];
      for (int i = tid; i < K * N; i += 256) lds[Os[l] + (i / N) * LD + (i % N)] = W[i];
      for (int i = tid; i < N; i += 256) lds[Os[l] + K * LD + i] = Bv[i];
    }
  }
  __syncthreads();
  // The weights do not change after the barrier, so the compiler is free to lift their LDS reads out of the unroll
  // loops and keep them in registers.  The narrow instances gain from that.  A wide instance has up to 40 accumulator
  // tiles and 8-slot layer inputs, the lifted reads would push it into scratch (AMD clang 22.0.0git of ROCm 7.2,
  // 256 VGPRs + 256 AGPRs each: 2412 bytes per lane at (64, 64, 63), 944 at (18, 32, 63), 316 at (18, 8, 63); with the
  // re-reads 256 + 81, 256 + 62 and 256 + 34 registers and no scratch), so it takes the base of the weights through an
  // opaque register once per step: every step re-reads what it needs from LDS, at a VGPR base plus a constant offset.
  // profiles/wide_train.txt has the figures per shape; tools/bench_train.py --wide times a narrow and a wide instance of
  // almost the same work (A = 16 / 17, E = 8) to show what the re-reads cost.
  auto weights = [&]() -> const float* {
    if constexpr (C::WIDE) {
      int z = 0;
      asm volatile("" : "+v"(z));
      return lds + z;
    } else {
      return lds;
    }
  };
  float* ck = lds + C::WEIGHT_WORDS + row * 16 * ES;  // + step * CK_WORDS_PER_STEP

  const int L = p.L;
  const int r_raw = blockIdx.x * 16 + row;
  const bool live = r_raw < p.B;
  const int r = live ? r_raw : p.B - 1;
  // rows past the batch contribute exact zeros; a row's weight (indexed by the GLOBAL row) scales its loss and, through
  // the three logit gradients, everything it back-propagates, at every unroll step; the L2 term is the reduction's
  const float scale = live ? (p.row_w ? p.loss_scale * p.row_w[r] : p.loss_scale) : 0.0f;

  // The body below spells out concat_onehot (make_x), state_fwd (sweep 1), state_bwd (next-state branch) and head_ce (the
  // three heads) of mz_train_blocks.cuh, statement for statement, and stays so on purpose: written WITH those blocks it
  // computes the same bits but not the same code (profiles/train_refactor.txt, section 2) -- head_ce for the policy head
  // moves the wide instances by 36 to 43 registers and (18, 8, 63) across an occupancy boundary, head_ce for the reward
  // head makes this compiler crash on instance (7, 40, 31), and even concat_onehot for this lambda reschedules every
  // instance.  As it stands every instance has the instruction stream it had before the blocks were shared.
  // x = [s, onehot(a)] as a row-distributed vector of X elements
  auto make_x = [&](const float (&s)[ES], int a, float (&x)[XS]) {
#pragma unroll
    for (int t = 0; t < XS; ++t) {
      const int k = j + 16 * t;
      float v = 0.0f;
      if (t < ES) v = (k < E) ? s[t] : 0.0f;
      x[t] = (k >= E && k < X) ? ((k - E == a) ? 1.0f : 0.0f) : v;
    }
  };

  // ---- sweep 1: hidden states s_0 .. s_{L-1} ----
  float u0[ES], s0mn, s0mx, s0c;  // representation pre-activation, kept for its backward
  {
#pragma unroll
    for (int t = 0; t < ES; ++t) {
      const int k = j + 16 * t;
      float acc = 0.0f;
      if (k < E) {
        for (int i = 0; i < p.obs_dim; ++i) acc = __builtin_fmaf(p.obs[(size_t)r * p.obs_dim + i], p.w[0][i * E + k], acc);
        acc = acc + p.w[1][k];
      }
      u0[t] = acc;
    }
    float s[ES];
    minmax_fwd<E>(u0, j, s, s0mn, s0mx, s0c);
#pragma unroll
    for (int t = 0; t < ES; ++t) ck[j + 16 * t] = s[t];
    for (int i = 0; i + 1 < L; ++i) {
      const float* Wl = weights();
      const float* Wdn1 = Wl + C::DN1; const float* Wdn2 = Wl + C::DN2;
      float x[XS], hn[1], u[ES], mn, mx, c;
      make_x(s, p.act[(size_t)r * L + i], x);
      lin_fwd<X, H>(x, Wdn1, j, hn);
      elu_vec(hn);
      lin_fwd<H, E>(hn, Wdn2, j, u);
      minmax_fwd<E>(u, j, s, mn, mx, c);
#pragma unroll
      for (int t = 0; t < ES; ++t) ck[(i + 1) * C::CK_WORDS_PER_STEP + j + 16 * t] = s[t];
    }
  }

  // ---- sweep 2: heads, loss and gradients, last step first ----
  f32x4 g_pv1[ES][1], g_pv2[1][FS], g_pp1[ES][1], g_pp2[1][AS], g_dr1[XS][1], g_dr2[1][FS], g_dn1[XS][1], g_dn2[1][ES];
  zero_tiles(g_pv1); zero_tiles(g_pv2); zero_tiles(g_pp1); zero_tiles(g_pp2);
  zero_tiles(g_dr1); zero_tiles(g_dr2); zero_tiles(g_dn1); zero_tiles(g_dn2);
  float b_pv1[1] = {0.0f}, b_pp1[1] = {0.0f}, b_dr1[1] = {0.0f}, b_dn1[1] = {0.0f};
  float b_pv2[FS], b_dr2[FS], b_dn2[ES], b_pp2[AS];
#pragma unroll
  for (int t = 0; t < FS; ++t) b_pv2[t] = b_dr2[t] = 0.0f;
#pragma unroll
  for (int t = 0; t < ES; ++t) b_dn2[t] = 0.0f;
#pragma unroll
  for (int t = 0; t < AS; ++t) b_pp2[t] = 0.0f;
  float loss = 0.0f;
  float ds_next[ES];
#pragma unroll
  for (int t = 0; t < ES; ++t) ds_next[t] = 0.0f;

  for (int i = L - 1; i >= 0; --i) {
    const float* Wl = weights();
    const float* Wpv1 = Wl + C::PV1; const float* Wpv2 = Wl + C::PV2;
    const float* Wpp1 = Wl + C::PP1; const float* Wpp2 = Wl + C::PP2;
    const float* Wdr1 = Wl + C::DR1; const float* Wdr2 = Wl + C::DR2;
    const float* Wdn1 = Wl + C::DN1; const float* Wdn2 = Wl + C::DN2;
    float s[ES], x[XS];
#pragma unroll
    for (int t = 0; t < ES; ++t) s[t] = ck[i * C::CK_WORDS_PER_STEP + j + 16 * t];
    const int a = p.act[(size_t)r * L + i];
    make_x(s, a, x);
    float ds[ES];
#pragma unroll
    for (int t = 0; t < ES; ++t) ds[t] = 0.0f;

    // -- dynamics: next-state branch (gradient arrives from step i + 1) and reward head --
    float dx[XS];
#pragma unroll
    for (int t = 0; t < XS; ++t) dx[t] = 0.0f;
    if (i + 1 < L) {
      float an[1], u[ES], ns[ES], mn, mx, c, du[ES], dan[1], dxn[XS];
      lin_fwd<X, H>(x, Wdn1, j, an);
      elu_vec(an);
      lin_fwd<H, E>(an, Wdn2, j, u);
      minmax_fwd<E>(u, j, ns, mn, mx, c);
      minmax_bwd<E>(ds_next, u, ns, mn, mx, c, j, du);
      grad_tiles(an, du, g_dn2);
#pragma unroll
      for (int t = 0; t < ES; ++t) b_dn2[t] = b_dn2[t] + du[t];
      lin_bwd<H, E>(du, Wdn2, j, dan);
      dan[0] = dan[0] * elu_grad(an[0]);
      grad_tiles(x, dan, g_dn1);
      b_dn1[0] = b_dn1[0] + dan[0];
      lin_bwd<X, H>(dan, Wdn1, j, dxn);
#pragma unroll
      for (int t = 0; t < XS; ++t) dx[t] = dx[t] + dxn[t];
    }
    {
      float ar[1], lr[FS], tr[FS], dlr[FS], dar[1], dxr[XS];
      lin_fwd<X, H>(x, Wdr1, j, ar);
      elu_vec(ar);
      lin_fwd<H, F>(ar, Wdr2, j, lr);
      support_target<F>(p.rew[(size_t)r * L + i], p.support, j, tr);
      loss = loss + ce_and_grad<F>(lr, tr, j, scale, dlr);
      grad_tiles(ar, dlr, g_dr2);
#pragma unroll
      for (int t = 0; t < FS; ++t) b_dr2[t] = b_dr2[t] + dlr[t];
      lin_bwd<H, F>(dlr, Wdr2, j, dar);
      dar[0] = dar[0] * elu_grad(ar[0]);
      grad_tiles(x, dar, g_dr1);
      b_dr1[0] = b_dr1[0] + dar[0];
      lin_bwd<X, H>(dar, Wdr1, j, dxr);
#pragma unroll
      for (int t = 0; t < XS; ++t) dx[t] = dx[t] + dxr[t];
    }
    // scale_gradient(s, 0.5) in front of the dynamics (muax/loss.py:60-61)
#pragma unroll
    for (int t = 0; t < ES; ++t) ds[t] = (j + 16 * t < E) ? 0.5f * dx[t] : 0.0f;

    // -- prediction heads on s_i --
    {
      float av[1], lv[FS], tv[FS], dlv[FS], dav[1], dsv[ES];
      lin_fwd<E, H>(s, Wpv1, j, av);
      elu_vec(av);
      lin_fwd<H, F>(av, Wpv2, j, lv);
      support_target<F>(p.ret[(size_t)r * L + i], p.support, j, tv);
      loss = loss + ce_and_grad<F>(lv, tv, j, scale, dlv);
      grad_tiles(av, dlv, g_pv2);
#pragma unroll
      for (int t = 0; t < FS; ++t) b_pv2[t] = b_pv2[t] + dlv[t];
      lin_bwd<H, F>(dlv, Wpv2, j, dav);
      dav[0] = dav[0] * elu_grad(av[0]);
      grad_tiles(s, dav, g_pv1);
      b_pv1[0] = b_pv1[0] + dav[0];
      lin_bwd<E, H>(dav, Wpv1, j, dsv);
#pragma unroll
      for (int t = 0; t < ES; ++t) ds[t] = ds[t] + dsv[t];
    }
    {
      float ap[1], lp[AS], tp[AS], dlp[AS], dap[1], dsp[ES];
      lin_fwd<E, H>(s, Wpp1, j, ap);
      elu_vec(ap);
      lin_fwd<H, A>(ap, Wpp2, j, lp);
#pragma unroll
      for (int t = 0; t < AS; ++t) tp[t] = (j + 16 * t < A) ? p.pi[((size_t)r * L + i) * A + j + 16 * t] : 0.0f;
      loss = loss + ce_and_grad<A>(lp, tp, j, scale, dlp);
      grad_tiles(ap, dlp, g_pp2);
#pragma unroll
      for (int t = 0; t < AS; ++t) b_pp2[t] = b_pp2[t] + dlp[t];
      lin_bwd<H, A>(dlp, Wpp2, j, dap);
      dap[0] = dap[0] * elu_grad(ap[0]);
      grad_tiles(s, dap, g_pp1);
      b_pp1[0] = b_pp1[0] + dap[0];
      lin_bwd<E, H>(dap, Wpp1, j, dsp);
#pragma unroll
      for (int t = 0; t < ES; ++t) ds[t] = ds[t] + dsp[t];
    }
#pragma unroll
    for (int t = 0; t < ES; ++t) ds_next[t] = ds[t];
  }

  // ---- representation: s_0 = minmax(obs W + b) ----
  float du0[ES];
  {
    float s[ES];
#pragma unroll
    for (int t = 0; t < ES; ++t) s[t] = ck[j + 16 * t];
    minmax_bwd<E>(ds_next, u0, s, s0mn, s0mx, s0c, j, du0);
  }

  // ---- this wavefront's partial gradient -> its workspace row ----
  float* dst = p.ws + (size_t)(blockIdx.x * 4 + (tid >> 6)) * (p.off[18] + 1);
  // obs^T du0, one tile row per 16 observation features (once per sample: the row lives only between its MFMAs and
  // its store, whatever obs_dim is)
  for (int o = 0; o < p.obs_dim; o += 16) {
    f32x4 g_rep[1][ES];
    zero_tiles(g_rep);
    float ob[1];
    ob[0] = o + j < p.obs_dim ? p.obs[(size_t)r * p.obs_dim + o + j] : 0.0f;
    grad_tiles(ob, du0, g_rep);
    store_tiles(g_rep, dst + p.off[0] + o * E, p.obs_dim - o, E, lane);
  }
  store_bias(du0, dst + p.off[1], E, lane);
  store_tiles(g_pv1, dst + p.off[2], E, H, lane);  store_bias(b_pv1, dst + p.off[3], H, lane);
  store_tiles(g_pv2, dst + p.off[4], H, F, lane);  store_bias(b_pv2, dst + p.off[5], F, lane);
  store_tiles(g_pp1, dst + p.off[6], E, H, lane);  store_bias(b_pp1, dst + p.off[7], H, lane);
  store_tiles(g_pp2, dst + p.off[8], H, A, lane);  store_bias(b_pp2, dst + p.off[9], A, lane);
  store_tiles(g_dr1, dst + p.off[10], X, H, lane); store_bias(b_dr1, dst + p.off[11], H, lane);
  store_tiles(g_dr2, dst + p.off[12], H, F, lane); store_bias(b_dr2, dst + p.off[13], F, lane);
  store_tiles(g_dn1, dst + p.off[14], X, H, lane); store_bias(b_dn1, dst + p.off[15], H, lane);
  store_tiles(g_dn2, dst + p.off[16], H, E, lane); store_bias(b_dn2, dst + p.off[17], E, lane);
  const float wl = rows_sum(loss * scale);
  if (lane == 0) dst[p.off[18]] = wl;
}

}  // namespace mz
