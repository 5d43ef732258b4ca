// mz_stoch_train.cuh -- fused forward + backward of the Stochastic MuZero loss (muax_amd/loss.py::stochastic_loss_fn) for
// the default stochastic MLP family (nn.create_stochastic_muzero_network): six modules, seven Linear(16)-elu-Linear
// stacks, the representation and the chance encoder.
//
// The mapping, the argument block, every arithmetic block and the reduction are mz_train_blocks.cuh's, shared with
// mz_train.cuh; this file is the graph of the family: StochTrainCfg (the LDS plan of an (A, C, E, F) instance), the
// encoder's forward and mz_stoch_train_kernel, whose partial rows go to mz_train_reduce_kernel<34>.
//
// Sweep 1 walks s_0 -> (after_1, c_1, s_1) -> ... through the encoder's argmax (the LOWEST index among equal maxima,
// torch.argmax on the CPU), the afterstate dynamics and the chance dynamics' next-state branch, and keeps s_i, after_i and
// c_i in LDS.  Sweep 2 goes back from transition L-1 to 1, re-evaluating each stack from the kept vectors; step 0 is the
// two prediction heads and the representation.  Only the gradient that reaches s_{i-1} through the afterstate dynamics
// is halved (scale_gradient comes after pred(s) has read the state).  The encoder's gradient is what the chance
// dynamics' two stacks leave on their code inputs (straight through) plus the commitment term's; the chance-logit cross
// entropy gives it nothing (detached target).
//
// One liberty: the chance dynamics and the chance-logit target read the EXACT one-hot of c_i (concat_onehot) where torch
// computes e + (onehot - e) in floating point; the two differ by an ulp of the input.
#pragma once
#include "mz_train_blocks.cuh"

#pragma clang fp contract(off)

namespace mz {

constexpr int STOCH_TRAIN_ARRAYS = 34;
constexpr int STOCH_TRAIN_MAX_OBS = 32;  // the listed instances' observation cap; mzs_stochastic_mlp_loss_grad names it
// repr_w, repr_b; ad, av, ac, cr, cn, pv, pp each w1, b1, w2, b2 (mzs_stochastic_mlp_weights' order); en_w1 .. en_b2
using StochTrainParams = TrainParamsT<STOCH_TRAIN_ARRAYS>;

// OB_: the observation cap of the instance -- OS = OB / 16 slots of first-layer gradient tiles for the chance encoder
// (the representation's go out 16 rows at a time), OB rows of the encoder's first layer in LDS.  32 for the listed
// instances; an instance built on demand (mz_stoch_train_jit.hip) takes obs_dim rounded up to 32 / 64 / 96 / 128.
template <int A_, int C_, int E_, int F_, int OB_ = STOCH_TRAIN_MAX_OBS>
struct StochTrainCfg {
  static constexpr int A = A_, C = C_, E = E_, F = F_, OB = OB_, H = 16, XA = E_ + A_, XC = E_ + C_;
  static constexpr int ES = (E + 15) / 16, FS = (F + 15) / 16, CS = (C + 15) / 16, AS = 1;
  static constexpr int XAS = (XA + 15) / 16, XCS = (XC + 15) / 16, OS = OB / 16;
  static constexpr int NA = STOCH_TRAIN_ARRAYS;
  static constexpr const char* DIMS = "(A, C, E, F)";
  static_assert(A <= 16, "policy head in one slot");
  static_assert(C <= 64 && E <= 64 && F <= 63, "at most four slots per vector");
  static_assert(OB == 32 || OB == 64 || OB == 96 || OB == 128, "observation cap: 32, 64, 96 or 128");
  static constexpr int ld(int n) { return 16 * ((n + 15) / 16) + 1; }
  static constexpr int blk(int k, int n) { return k * ld(n) + 16 * ((n + 15) / 16); }
  // LDS blocks in the order of the arrays 2 .. 33
  static constexpr int AD1 = 0;
  static constexpr int AD2 = AD1 + blk(XA, H);
  static constexpr int AV1 = AD2 + blk(H, E);
  static constexpr int AV2 = AV1 + blk(E, H);
  static constexpr int AC1 = AV2 + blk(H, F);
  static constexpr int AC2 = AC1 + blk(E, H);
  static constexpr int CR1 = AC2 + blk(H, C);
  static constexpr int CR2 = CR1 + blk(XC, H);
  static constexpr int CN1 = CR2 + blk(H, F);
  static constexpr int CN2 = CN1 + blk(XC, H);
  static constexpr int PV1 = CN2 + blk(H, E);
  static constexpr int PV2 = PV1 + blk(E, H);
  static constexpr int PP1 = PV2 + blk(H, F);
  static constexpr int PP2 = PP1 + blk(E, H);
  static constexpr int EN1 = PP2 + blk(H, A);  // [obs_dim][17], the bias behind row obs_dim - 1
  static constexpr int EN2 = EN1 + blk(OB, H);
  static constexpr int WEIGHT_WORDS = ((EN2 + blk(H, C) + 3) / 4) * 4;
  // per step and sample: s_i, after_i (16 ES words each); per step and workgroup 16 more words hold c_i
  static constexpr int CK_STATE = 0, CK_AFTER = 16 * 16 * ES, CK_CODE = 2 * 16 * 16 * ES;
  static constexpr int CK_WORDS_PER_STEP = CK_CODE + 16;
  static constexpr int MAX_UNROLL = (TRAIN_LDS_BYTES / 4 - WEIGHT_WORDS) / CK_WORDS_PER_STEP;
};

// the encoder: h = elu(obs W1 + b1) over the run-time obs_dim (obs read per row, a broadcast), e = h W2 + b2
template <int C>
MZ_DEV void encoder_fwd(const float* obs_row, int obs_dim, const float* W1, const float* W2, int j, float (&h)[1],
                        float (&e)[(C + 15) / 16]) {
  float acc = 0.0f;
  for (int k = 0; k < obs_dim; ++k) acc = __builtin_fmaf(obs_row[k], W1[k * 17 + j], acc);
  h[0] = elu(acc + W1[obs_dim * 17 + j]);
  lin_fwd<16, C>(h, W2, j, e);
}

template <class Cf>
__global__ __launch_bounds__(256) void mz_stoch_train_kernel(const StochTrainParams p) {
  constexpr int A = Cf::A, C = Cf::C, E = Cf::E, F = Cf::F, H = Cf::H, XA = Cf::XA, XC = Cf::XC;
  constexpr int ES = Cf::ES, FS = Cf::FS, CS = Cf::CS, XAS = Cf::XAS, XCS = Cf::XCS, OS = Cf::OS;
  constexpr int LDH = 17;  // row stride of every [K][16] block
  extern __shared__ float lds[];
  const int tid = threadIdx.x, lane = tid & 63, j = tid & 15;
  const int row = tid >> 4;
  const int L = p.L, OD = p.obs_dim;

  // ---- weights -> LDS ----
  for (int i = tid; i < Cf::WEIGHT_WORDS; i += 256) lds[i] = 0.0f;
  __syncthreads();
  {
    const int Ks[16] = {XA, H, E, H, E, H, XC, H, XC, H, E, H, E, H, OD, H};
    const int Ns[16] = {H, E, H, F, H, C, H, F, H, E, H, F, H, A, H, C};
    const int Os[16] = {Cf::AD1, Cf::AD2, Cf::AV1, Cf::AV2, Cf::AC1, Cf::AC2, Cf::CR1, Cf::CR2,
                        Cf::CN1, Cf::CN2, Cf::PV1, Cf::PV2, Cf::PP1, Cf::PP2, Cf::EN1, Cf::EN2};
    for (int l = 0; l < 16; ++l) {
      const int K = Ks[l], N = Ns[l], LD = 16 * ((N + 15) / 16) + 1;
      const float* W = p.w[2 + 2 * l];
      const float* Bv = p.w[3 + 2 * l];
      for (int i = tid; i < K * N; i += 256) lds[Os[l] + (i / N) * LD + (i % N)] = W[i];
      for (int i = tid; i < N; i += 256) lds[Os[l] + K * LD + i] = Bv[i];
    }
  }
  __syncthreads();
  // every step re-reads what it needs from LDS at an opaque base (mz_train.cuh's device for its wide instances: with
  // up to 42 accumulator tiles the reads must not be lifted out of the unroll loops into registers)
  auto weights = [&]() -> const float* {
    int z = 0;
    asm volatile("" : "+v"(z));
    return lds + z;
  };
  float* ck = lds + Cf::WEIGHT_WORDS;  // + step * CK_WORDS_PER_STEP
  const int cko = row * 16 * ES + j;   // this lane's word of its sample's kept vectors (+ 16 t)

  const int r_raw = blockIdx.x * 16 + row;
  const bool live = r_raw < p.B;
  const int r = live ? r_raw : p.B - 1;
  const float scale = live ? (p.row_w ? p.loss_scale * p.row_w[r] : p.loss_scale) : 0.0f;
  const float* obs_r = p.obs + (size_t)r * L * OD;

  // ---- sweep 1 ----
  float u0[ES], s0mn, s0mx, s0c;
  {
#pragma unroll
    for (int t = 0; t < ES; ++t) {
      const int k = j + 16 * t;
      float acc = 0.0f;
      if (k < E) {
        for (int i = 0; i < OD; ++i) acc = __builtin_fmaf(obs_r[i], p.w[0][i * E + k], acc);
        acc = acc + p.w[1][k];
      }
      u0[t] = acc;
    }
    float s[ES];
    minmax_fwd<E>(u0, j, s, s0mn, s0mx, s0c);
#pragma unroll
    for (int t = 0; t < ES; ++t) ck[Cf::CK_STATE + cko + 16 * t] = s[t];
    for (int i = 1; i < L; ++i) {
      const float* Wl = weights();
      float* cki = ck + i * Cf::CK_WORDS_PER_STEP;
      float he[1], e[CS], xa[XAS], after[ES], xc[XCS];
      encoder_fwd<C>(obs_r + (size_t)i * OD, OD, Wl + Cf::EN1, Wl + Cf::EN2, j, he, e);
      const int c = argmax_first<C>(e, j);
      concat_onehot<E, A>(s, p.act[(size_t)r * L + i - 1], j, xa);
      state_fwd<XA, E>(xa, Wl + Cf::AD1, Wl + Cf::AD2, j, after);
      concat_onehot<E, C>(after, c, j, xc);
      state_fwd<XC, E>(xc, Wl + Cf::CN1, Wl + Cf::CN2, j, s);
#pragma unroll
      for (int t = 0; t < ES; ++t) {
        cki[Cf::CK_STATE + cko + 16 * t] = s[t];
        cki[Cf::CK_AFTER + cko + 16 * t] = after[t];
      }
      cki[Cf::CK_CODE + row] = __int_as_float(c);  // (all 16 lanes of the row, the same word and value)
    }
  }
  // (each sample's kept words are written and read by its own 16 lanes of one wavefront only: no barrier)

  // ---- sweep 2 ----
  f32x4 g_ad1[XAS][1], g_ad2[1][ES], g_av1[ES][1], g_av2[1][FS], g_ac1[ES][1], g_ac2[1][CS], g_cr1[XCS][1], g_cr2[1][FS];
  f32x4 g_cn1[XCS][1], g_cn2[1][ES], g_pv1[ES][1], g_pv2[1][FS], g_pp1[ES][1], g_pp2[1][1], g_en1[OS][1], g_en2[1][CS];
  zero_tiles(g_ad1); zero_tiles(g_ad2); zero_tiles(g_av1); zero_tiles(g_av2); zero_tiles(g_ac1); zero_tiles(g_ac2);
  zero_tiles(g_cr1); zero_tiles(g_cr2); zero_tiles(g_cn1); zero_tiles(g_cn2); zero_tiles(g_pv1); zero_tiles(g_pv2);
  zero_tiles(g_pp1); zero_tiles(g_pp2); zero_tiles(g_en1); zero_tiles(g_en2);
  float b_ad1[1] = {0.0f}, b_av1[1] = {0.0f}, b_ac1[1] = {0.0f}, b_cr1[1] = {0.0f}, b_cn1[1] = {0.0f};
  float b_pv1[1] = {0.0f}, b_pp1[1] = {0.0f}, b_en1[1] = {0.0f}, b_pp2[1] = {0.0f};
  float b_ad2[ES], b_cn2[ES], b_av2[FS], b_cr2[FS], b_pv2[FS], b_ac2[CS], b_en2[CS];
#pragma unroll
  for (int t = 0; t < ES; ++t) b_ad2[t] = b_cn2[t] = 0.0f;
#pragma unroll
  for (int t = 0; t < FS; ++t) b_av2[t] = b_cr2[t] = b_pv2[t] = 0.0f;
#pragma unroll
  for (int t = 0; t < CS; ++t) b_ac2[t] = b_en2[t] = 0.0f;
  float loss = 0.0f;
  float ds[ES];  // gradient at s_i: what came back through the afterstate dynamics of transition i + 1, halved
#pragma unroll
  for (int t = 0; t < ES; ++t) ds[t] = 0.0f;

  for (int i = L - 1; i >= 0; --i) {
    const float* Wl = weights();
    const float* cki = ck + i * Cf::CK_WORDS_PER_STEP;
    // -- prediction heads on s_i --
    {
      float s[ES], tv[FS], tp[1], dh[1], dsh[ES];
#pragma unroll
      for (int t = 0; t < ES; ++t) s[t] = cki[Cf::CK_STATE + cko + 16 * t];
      support_target<F>(p.ret[(size_t)r * L + i], p.support, j, tv);
      loss = loss + head_ce<E, F>(s, Wl + Cf::PV1, Wl + Cf::PV2, tv, j, scale, g_pv1, b_pv1, g_pv2, b_pv2, dh);
      lin_bwd<E, H>(dh, Wl + Cf::PV1, j, dsh);
#pragma unroll
      for (int t = 0; t < ES; ++t) ds[t] = ds[t] + dsh[t];
      tp[0] = (j < A) ? p.pi[((size_t)r * L + i) * A + j] : 0.0f;
      loss = loss + head_ce<E, A>(s, Wl + Cf::PP1, Wl + Cf::PP2, tp, j, scale, g_pp1, b_pp1, g_pp2, b_pp2, dh);
      lin_bwd<E, H>(dh, Wl + Cf::PP1, j, dsh);
#pragma unroll
      for (int t = 0; t < ES; ++t) ds[t] = ds[t] + dsh[t];
    }
    if (i == 0) break;  // ds is now the whole gradient at s_0

    // -- transition i: s_{i-1}, a_{i-1} -> after_i; after_i, c_i -> r, s_i --
    float after[ES], dafter[ES], de[CS];
#pragma unroll
    for (int t = 0; t < ES; ++t) after[t] = cki[Cf::CK_AFTER + cko + 16 * t];
    const int c = __float_as_int(cki[Cf::CK_CODE + row]);
    {
      float xc[XCS], tr[FS], dh[1], d1[ES], d2[CS];
      concat_onehot<E, C>(after, c, j, xc);
      // chance dynamics, next-state branch: the gradient at s_i goes through the normaliser and the stack
      state_bwd<XC, E>(xc, Wl + Cf::CN1, Wl + Cf::CN2, ds, j, g_cn1, b_cn1, g_cn2, b_cn2, dh);
      lin_bwd<E, H>(dh, Wl + Cf::CN1, j, dafter);
      lin_bwd<C, H>(dh, Wl + Cf::CN1 + E * LDH, j, de);  // rows E .. E + C - 1 of W1: the code inputs
      // reward head
      support_target<F>(p.rew[(size_t)r * L + i - 1], p.support, j, tr);
      loss = loss + head_ce<XC, F>(xc, Wl + Cf::CR1, Wl + Cf::CR2, tr, j, scale, g_cr1, b_cr1, g_cr2, b_cr2, dh);
      lin_bwd<E, H>(dh, Wl + Cf::CR1, j, d1);
      lin_bwd<C, H>(dh, Wl + Cf::CR1 + E * LDH, j, d2);
#pragma unroll
      for (int t = 0; t < ES; ++t) dafter[t] = dafter[t] + d1[t];
#pragma unroll
      for (int t = 0; t < CS; ++t) de[t] = de[t] + d2[t];
    }
    // -- afterstate prediction on after_i: afterstate value against Rn_{i-1}, chance logits against onehot(c_i) --
    {
      float tv[FS], tc[CS], dh[1], d1[ES];
      support_target<F>(p.ret[(size_t)r * L + i - 1], p.support, j, tv);
      loss = loss + head_ce<E, F>(after, Wl + Cf::AV1, Wl + Cf::AV2, tv, j, scale, g_av1, b_av1, g_av2, b_av2, dh);
      lin_bwd<E, H>(dh, Wl + Cf::AV1, j, d1);
#pragma unroll
      for (int t = 0; t < ES; ++t) dafter[t] = dafter[t] + d1[t];
#pragma unroll
      for (int t = 0; t < CS; ++t) tc[t] = (j + 16 * t == c) ? 1.0f : 0.0f;
      loss = loss + head_ce<E, C>(after, Wl + Cf::AC1, Wl + Cf::AC2, tc, j, scale, g_ac1, b_ac1, g_ac2, b_ac2, dh);
      lin_bwd<E, H>(dh, Wl + Cf::AC1, j, d1);
#pragma unroll
      for (int t = 0; t < ES; ++t) dafter[t] = dafter[t] + d1[t];
    }
    // -- afterstate dynamics on [s_{i-1}, onehot(a_{i-1})]; scale_gradient(s_{i-1}, 0.5) in front of it --
    {
      float sp[ES], xa[XAS], dh[1], dsp[ES];
#pragma unroll
      for (int t = 0; t < ES; ++t) sp[t] = (cki - Cf::CK_WORDS_PER_STEP)[Cf::CK_STATE + cko + 16 * t];
      concat_onehot<E, A>(sp, p.act[(size_t)r * L + i - 1], j, xa);
      state_bwd<XA, E>(xa, Wl + Cf::AD1, Wl + Cf::AD2, dafter, j, g_ad1, b_ad1, g_ad2, b_ad2, dh);
      lin_bwd<E, H>(dh, Wl + Cf::AD1, j, dsp);
#pragma unroll
      for (int t = 0; t < ES; ++t) ds[t] = 0.5f * dsp[t];
    }
    // -- encoder on obs_i: straight-through gradient of the code + the commitment term beta * mean_C (e - onehot)^2 --
    {
      float he[1], e[CS], ob[OS], dhe[1];
      encoder_fwd<C>(obs_r + (size_t)i * OD, OD, Wl + Cf::EN1, Wl + Cf::EN2, j, he, e);
      float part = 0.0f;
#pragma unroll
      for (int t = 0; t < CS; ++t) {
        const int k = j + 16 * t;
        const float d = (k < C) ? e[t] - ((k == c) ? 1.0f : 0.0f) : 0.0f;
        part = part + d * d;
        de[t] = (k < C) ? de[t] + (2.0f * p.beta / (float)C) * scale * d : 0.0f;
      }
      loss = loss + p.beta * (row_sum(part) / (float)C);
      grad_tiles(he, de, g_en2);
#pragma unroll
      for (int t = 0; t < CS; ++t) b_en2[t] = b_en2[t] + de[t];
      lin_bwd<H, C>(de, Wl + Cf::EN2, j, dhe);
      dhe[0] = dhe[0] * elu_grad(he[0]);
#pragma unroll
      for (int t = 0; t < OS; ++t) ob[t] = (j + 16 * t < OD) ? obs_r[(size_t)i * OD + j + 16 * t] : 0.0f;
      grad_tiles(ob, dhe, g_en1);
      b_en1[0] = b_en1[0] + dhe[0];
    }
  }

  // ---- representation: s_0 = minmax(obs_0 W + b) ----
  float du0[ES];
  {
    float s[ES];
#pragma unroll
    for (int t = 0; t < ES; ++t) s[t] = ck[Cf::CK_STATE + cko + 16 * t];
    minmax_bwd<E>(ds, u0, s, s0mn, s0mx, s0c, j, du0);
  }

  // ---- this wavefront's partial gradient -> its workspace row ----
  const int* off = p.off;
  float* dst = p.ws + (size_t)(blockIdx.x * 4 + (tid >> 6)) * (off[STOCH_TRAIN_ARRAYS] + 1);
  for (int o = 0; o < OD; o += 16) {
    f32x4 g_rep[1][ES];
    zero_tiles(g_rep);
    float ob[1];
    ob[0] = o + j < OD ? obs_r[o + j] : 0.0f;
    grad_tiles(ob, du0, g_rep);
    store_tiles(g_rep, dst + off[0] + o * E, OD - o, E, lane);
  }
  store_bias(du0, dst + off[1], E, lane);
  store_tiles(g_ad1, dst + off[2], XA, H, lane);   store_bias(b_ad1, dst + off[3], H, lane);
  store_tiles(g_ad2, dst + off[4], H, E, lane);    store_bias(b_ad2, dst + off[5], E, lane);
  store_tiles(g_av1, dst + off[6], E, H, lane);    store_bias(b_av1, dst + off[7], H, lane);
  store_tiles(g_av2, dst + off[8], H, F, lane);    store_bias(b_av2, dst + off[9], F, lane);
  store_tiles(g_ac1, dst + off[10], E, H, lane);   store_bias(b_ac1, dst + off[11], H, lane);
  store_tiles(g_ac2, dst + off[12], H, C, lane);   store_bias(b_ac2, dst + off[13], C, lane);
  store_tiles(g_cr1, dst + off[14], XC, H, lane);  store_bias(b_cr1, dst + off[15], H, lane);
  store_tiles(g_cr2, dst + off[16], H, F, lane);   store_bias(b_cr2, dst + off[17], F, lane);
  store_tiles(g_cn1, dst + off[18], XC, H, lane);  store_bias(b_cn1, dst + off[19], H, lane);
  store_tiles(g_cn2, dst + off[20], H, E, lane);   store_bias(b_cn2, dst + off[21], E, lane);
  store_tiles(g_pv1, dst + off[22], E, H, lane);   store_bias(b_pv1, dst + off[23], H, lane);
  store_tiles(g_pv2, dst + off[24], H, F, lane);   store_bias(b_pv2, dst + off[25], F, lane);
  store_tiles(g_pp1, dst + off[26], E, H, lane);   store_bias(b_pp1, dst + off[27], H, lane);
  store_tiles(g_pp2, dst + off[28], H, A, lane);   store_bias(b_pp2, dst + off[29], A, lane);
  store_tiles(g_en1, dst + off[30], OD, H, lane);  store_bias(b_en1, dst + off[31], H, lane);
  store_tiles(g_en2, dst + off[32], H, C, lane);   store_bias(b_en2, dst + off[33], C, lane);
  const float wl = rows_sum(loss * scale);
  if (lane == 0) dst[off[STOCH_TRAIN_ARRAYS]] = wl;
}

}  // namespace mz
