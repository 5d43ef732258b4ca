// mz_stoch_train.hip -- training step of the default stochastic MLP family (mzs_stochastic_mlp_loss_grad): the listed
// instances of mz_stoch_train.cuh, their launcher and the host-side refusals.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "../../include/mzsearch.h"
#include "mz_host.h"
#include "mz_stoch_train.cuh"

using mzh::fail;

static const char kWho[] = "mzs_stochastic_mlp_loss_grad";

static void stoch_offsets(int obs_dim, int E, int A, int C, int F, int off[mz::STOCH_TRAIN_ARRAYS + 1]) {
  const int H = 16, XA = E + A, XC = E + C;
  const int sizes[mz::STOCH_TRAIN_ARRAYS] = {
      obs_dim * E, E,
      XA * H, H, H * E, E,  E * H, H, H * F, F,  E * H, H, H * C, C,  XC * H, H, H * F, F,  XC * H, H, H * E, E,
      E * H, H, H * F, F,  E * H, H, H * A, A,
      obs_dim * H, H, H * C, C};
  off[0] = 0;
  for (int i = 0; i < mz::STOCH_TRAIN_ARRAYS; ++i) off[i + 1] = off[i] + sizes[i];
}

// Both launches of one training step for instance Cf; the caller has validated `p` (L <= MAX_UNROLL) and selected the device.
template <class Cf>
static int launch_stoch_train(const mz::StochTrainParams& p, hipStream_t stream) {
  const size_t lds = sizeof(float) * ((size_t)Cf::WEIGHT_WORDS + (size_t)p.L * Cf::CK_WORDS_PER_STEP);
  auto kern = mz::mz_stoch_train_kernel<Cf>;
  static mzh::LdsGrant granted;
  int dev = 0;
  MZS_HIP(nullptr, hipGetDevice(&dev));
  if (!granted.covers(dev, lds)) {
    MZS_HIP(nullptr, hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    granted.note(dev, lds);
  }
  hipLaunchKernelGGL(kern, dim3(p.waves / 4), dim3(256), lds, stream, p);
  MZS_HIP(nullptr, hipGetLastError());
  hipLaunchKernelGGL(mz::mz_stoch_train_reduce_kernel, dim3((p.off[mz::STOCH_TRAIN_ARRAYS] + 31) / 32), dim3(256), 0, stream, p);
  MZS_HIP(nullptr, hipGetLastError());
  return MZS_OK;
}

// the listed instances (A, C, E, F): the three test shapes, 2048 at support 10, examples/fit_2048_stochastic.py
#define MZ_STOCH_TRAIN_INSTANCES(X) X(3, 2, 4, 17) X(4, 32, 16, 21) X(4, 17, 8, 17) X(4, 32, 32, 63)

extern "C" {

int64_t mzs_stochastic_mlp_num_params(int32_t obs_dim, int32_t embed_dim, int32_t num_actions, int32_t num_chance_outcomes,
                                      int32_t support_size) {
  int off[mz::STOCH_TRAIN_ARRAYS + 1];
  stoch_offsets(obs_dim, embed_dim, num_actions, num_chance_outcomes, 2 * support_size + 1, off);
  return off[mz::STOCH_TRAIN_ARRAYS];
}

int64_t mzs_stochastic_mlp_train_workspace_bytes(int32_t batch, int32_t obs_dim, int32_t embed_dim, int32_t num_actions,
                                                 int32_t num_chance_outcomes, int32_t support_size) {
  const int64_t waves = 4 * (int64_t)((batch + 15) / 16);
  return waves * (mzs_stochastic_mlp_num_params(obs_dim, embed_dim, num_actions, num_chance_outcomes, support_size) + 1) *
         (int64_t)sizeof(float);
}

int mzs_stochastic_mlp_loss_grad(const mzs_stochastic_train_weights* w, const mzs_stochastic_train_args* a, void* stream_) {
  if (!w || w->struct_size != (int32_t)sizeof(mzs_stochastic_train_weights))
    return fail(nullptr, MZS_E_INVALID, "%s: null weights or size mismatch (ABI)", kWho);
  if (!a || a->struct_size != (int32_t)sizeof(mzs_stochastic_train_args))
    return fail(nullptr, MZS_E_INVALID, "%s: null arguments or size mismatch (ABI)", kWho);
  const float* const* ptrs = &w->repr_w;
  for (int i = 0; i < mz::STOCH_TRAIN_ARRAYS; ++i)
    if (!ptrs[i]) return fail(nullptr, MZS_E_INVALID, "%s: null weight pointer", kWho);
  if (a->batch <= 0 || a->unroll_steps <= 0)
    return fail(nullptr, MZS_E_INVALID, "%s: batch and unroll_steps must be positive", kWho);
  if (!a->obs || !a->actions || !a->rewards || !a->returns || !a->policy || !a->loss || !a->grads || !a->workspace)
    return fail(nullptr, MZS_E_INVALID, "%s: null batch / output / workspace pointer", kWho);
  if (w->obs_dim <= 0 || w->obs_dim > mz::STOCH_TRAIN_MAX_OBS)
    return fail(nullptr, MZS_E_UNSUPPORTED, "%s: obs_dim must be 1..32", kWho);
  const int A = a->num_actions, C = a->num_chance_outcomes, E = a->embed_dim, F = 2 * w->support_size + 1;
  if (w->support_size < 8 || w->support_size > 31)
    return fail(nullptr, MZS_E_UNSUPPORTED, "%s: no kernel instance for this (A, C, E, F): support_size must be 8..31", kWho);
  int max_unroll = 0;  // of the listed instance, 0: there is none
#define MZ_X(a_, c_, e_, f_) \
  if (A == a_ && C == c_ && E == e_ && F == f_) max_unroll = mz::StochTrainCfg<a_, c_, e_, f_>::MAX_UNROLL;
  MZ_STOCH_TRAIN_INSTANCES(MZ_X)
#undef MZ_X
  if (max_unroll <= 0) return fail(nullptr, MZS_E_UNSUPPORTED, "%s: no kernel instance for this (A, C, E, F)", kWho);
  if (a->workspace_bytes < mzs_stochastic_mlp_train_workspace_bytes(a->batch, w->obs_dim, E, A, C, w->support_size))
    return fail(nullptr, MZS_E_INVALID, "%s: workspace too small", kWho);
  if (a->unroll_steps > max_unroll) {
    char msg[160];
    snprintf(msg, sizeof msg, "unroll_steps %d too large for the LDS (at most %d for this (A, C, E, F))", a->unroll_steps, max_unroll);
    return fail(nullptr, MZS_E_UNSUPPORTED, "mzs_stochastic_mlp_loss_grad: %s", msg);
  }
  if (int rc = mzh::select_device(a->device, kWho)) return rc;
  mz::StochTrainParams p;
  memset(&p, 0, sizeof p);
  p.obs = a->obs; p.act = a->actions; p.rew = a->rewards; p.ret = a->returns; p.pi = a->policy;
  for (int i = 0; i < mz::STOCH_TRAIN_ARRAYS; ++i) p.w[i] = ptrs[i];
  stoch_offsets(w->obs_dim, E, A, C, F, p.off);
  p.B = a->batch; p.L = a->unroll_steps; p.obs_dim = w->obs_dim; p.support = w->support_size;
  p.loss_scale = a->loss_scale; p.l2 = a->l2_coeff; p.beta = a->vqvae_beta;
  p.ws = static_cast<float*>(a->workspace); p.grads = a->grads; p.loss = a->loss;
  p.waves = 4 * ((a->batch + 15) / 16);
  p.row_w = a->sample_weight;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
#define MZ_X(a_, c_, e_, f_) \
  if (A == a_ && C == c_ && E == e_ && F == f_) return launch_stoch_train<mz::StochTrainCfg<a_, c_, e_, f_>>(p, stream);
  MZ_STOCH_TRAIN_INSTANCES(MZ_X)
#undef MZ_X
  return fail(nullptr, MZS_E_UNSUPPORTED, "%s: no kernel instance for this (A, C, E, F)", kWho);
}

}  // extern "C"
