// mz_unroll.hip -- translation unit of the forward value unroll (mz_unroll.cuh): argument checks and the one launch of
// mzs_mlp_unroll_values (the default trio) and of mzs_stochastic_mlp_unroll_values (the default stochastic family).
// Built like the other units of the arithmetic spec (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include "mz_host.h"
#include "mz_unroll.cuh"

using mzh::fail;

extern "C" {

int mzs_mlp_unroll_values(const mzs_mlp_weights* w, const mzs_unroll_args* a, void* stream_) {
  if (!w || w->struct_size != (int32_t)sizeof(mzs_mlp_weights))
    return fail(nullptr, MZS_E_INVALID, "mzs_mlp_unroll_values: null weights or size mismatch (ABI)");
  if (!a || a->struct_size != (int32_t)sizeof(mzs_unroll_args))
    return fail(nullptr, MZS_E_INVALID, "mzs_mlp_unroll_values: null arguments or size mismatch (ABI)");
  const float* const* ptrs = &w->repr_w;
  for (int i = 0; i < 18; ++i)
    if (!ptrs[i]) return fail(nullptr, MZS_E_INVALID, "mzs_mlp_unroll_values: null weight pointer");
  if (a->batch < 1) return fail(nullptr, MZS_E_INVALID, "mzs_mlp_unroll_values: batch must be >= 1");
  if (a->row_steps < 1 || a->k_prio < 1 || a->k_prio > a->row_steps)
    return fail(nullptr, MZS_E_INVALID, "mzs_mlp_unroll_values: k_prio must be in 1..row_steps");
  if (!a->obs || !a->actions || !a->returns)
    return fail(nullptr, MZS_E_INVALID, "mzs_mlp_unroll_values: null obs, actions or returns");
  if (!a->values && !a->prio)
    return fail(nullptr, MZS_E_INVALID, "mzs_mlp_unroll_values: at least one of values and prio must be given");
  if (w->obs_dim < 1 || w->obs_dim > 128) return fail(nullptr, MZS_E_UNSUPPORTED, "mzs_mlp_unroll_values: obs_dim must be 1..128");
  if (a->embed_dim < 1 || a->embed_dim > 64)
    return fail(nullptr, MZS_E_UNSUPPORTED, "mzs_mlp_unroll_values: embed_dim must be 1..64");
  if (a->num_actions < 1 || a->num_actions > 64)
    return fail(nullptr, MZS_E_UNSUPPORTED, "mzs_mlp_unroll_values: num_actions must be 1..64");
  if (w->support_size < 8 || w->support_size > 31)
    return fail(nullptr, MZS_E_UNSUPPORTED, "mzs_mlp_unroll_values: support_size must be 8..31");
  if (int rc = mzh::select_device(a->device, "mzs_mlp_unroll_values")) return rc;
  mz::UnrollArgs p{};
  mz::MlpGen& g = p.w;
  mzh::copy_weights(*w, g);
  g.obs_dim = w->obs_dim; g.E = a->embed_dim; g.A = a->num_actions; g.F = 2 * w->support_size + 1;
  g.support = w->support_size; g.pred_on_parent = 0; g.discount = w->discount;
  p.B = a->batch; p.L = a->row_steps; p.kp = a->k_prio;
  p.obs = a->obs; p.act = a->actions; p.Rn = a->returns; p.values = a->values; p.prio = a->prio;
  // the trio's scratch with the observation in the place of [s, onehot]: 2.2 KiB at the widest shape
  const size_t lds = sizeof(float) * (size_t)mz::gen_scratch_words(mz::gen_obs_width(g.E, g.obs_dim), g.A);
  hipLaunchKernelGGL(mz::mz_mlp_unroll_kernel, dim3(a->batch), dim3(64), lds, static_cast<hipStream_t>(stream_), p);
  MZS_HIP(nullptr, hipGetLastError());
  return MZS_OK;
}

int mzs_stochastic_mlp_unroll_values(const mzs_stochastic_train_weights* w, const mzs_stochastic_unroll_args* a, void* stream_) {
  static const char kWho[] = "mzs_stochastic_mlp_unroll_values";
  if (!w || w->struct_size != (int32_t)sizeof(mzs_stochastic_train_weights))
    return fail(nullptr, MZS_E_INVALID, "%s: null weights or size mismatch (ABI)", kWho);
  if (!a || a->struct_size != (int32_t)sizeof(mzs_stochastic_unroll_args))
    return fail(nullptr, MZS_E_INVALID, "%s: null arguments or size mismatch (ABI)", kWho);
  const float* const* ptrs = &w->repr_w;
  for (int i = 0; i < 34; ++i)
    if (!ptrs[i]) return fail(nullptr, MZS_E_INVALID, "%s: null weight pointer", kWho);
  if (a->batch < 1) return fail(nullptr, MZS_E_INVALID, "%s: batch must be >= 1", kWho);
  if (a->row_steps < 1 || a->k_prio < 1 || a->k_prio > a->row_steps)
    return fail(nullptr, MZS_E_INVALID, "%s: k_prio must be in 1..row_steps", kWho);
  if (!a->obs || !a->actions || !a->returns) return fail(nullptr, MZS_E_INVALID, "%s: null obs, actions or returns", kWho);
  if (!a->values && !a->prio && !a->codes)
    return fail(nullptr, MZS_E_INVALID, "%s: at least one of values, prio and codes must be given", kWho);
  if (w->obs_dim < 1 || w->obs_dim > 128) return fail(nullptr, MZS_E_UNSUPPORTED, "%s: obs_dim must be 1..128", kWho);
  if (a->embed_dim < 1 || a->embed_dim > 64) return fail(nullptr, MZS_E_UNSUPPORTED, "%s: embed_dim must be 1..64", kWho);
  if (a->num_actions < 1) return fail(nullptr, MZS_E_UNSUPPORTED, "%s: num_actions must be >= 1", kWho);
  if (a->num_chance_outcomes < 1) return fail(nullptr, MZS_E_UNSUPPORTED, "%s: num_chance_outcomes must be >= 1", kWho);
  // (compared one at a time first: the sum of two huge counts must not wrap)
  if (a->num_actions > 64 || a->num_chance_outcomes > 64 || a->num_actions + a->num_chance_outcomes > 64)
    return fail(nullptr, MZS_E_UNSUPPORTED, "%s: num_actions + num_chance_outcomes must be <= 64", kWho);
  if (w->support_size < 8 || w->support_size > 31)
    return fail(nullptr, MZS_E_UNSUPPORTED, "%s: support_size must be 8..31", kWho);
  if (int rc = mzh::select_device(a->device, kWho)) return rc;
  mz::StochUnrollArgs p{};
  p.repr_w = w->repr_w; p.repr_b = w->repr_b;
  p.ad = {w->ad_w1, w->ad_b1, w->ad_w2, w->ad_b2};
  p.cn = {w->cn_w1, w->cn_b1, w->cn_w2, w->cn_b2};
  p.pv = {w->pv_w1, w->pv_b1, w->pv_w2, w->pv_b2};
  p.en = {w->en_w1, w->en_b1, w->en_w2, w->en_b2};
  p.obs_dim = w->obs_dim; p.E = a->embed_dim; p.A = a->num_actions; p.C = a->num_chance_outcomes;
  p.F = 2 * w->support_size + 1; p.support = w->support_size;
  p.B = a->batch; p.L = a->row_steps; p.kp = a->k_prio;
  p.obs = a->obs; p.act = a->actions; p.Rn = a->returns; p.values = a->values; p.prio = a->prio; p.codes = a->codes;
  // the trio's scratch, G.sa wide enough for the observation row and for a one-hot of max(A, C): 2.2 KiB at the widest
  const int hot = p.A > p.C ? p.A : p.C;
  const size_t lds = sizeof(float) * (size_t)mz::gen_scratch_words(mz::gen_obs_width(p.E, p.obs_dim), hot);
  hipLaunchKernelGGL(mz::mz_stoch_unroll_kernel, dim3(a->batch), dim3(64), lds, static_cast<hipStream_t>(stream_), p);
  MZS_HIP(nullptr, hipGetLastError());
  return MZS_OK;
}

}  // extern "C"
