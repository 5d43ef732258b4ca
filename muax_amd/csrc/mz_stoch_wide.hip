// mz_stoch_wide.hip -- the one-launch stochastic search kernel (mz_stoch_wide.cuh) and its host side: the launch, the LDS
// plan and the per-call device block of the C-ABI.
#include "mz_stoch_wide.cuh"

#include <cstring>

#include "../../include/mzsearch.h"
#include "mz_host.h"
#include "mz_keys.h"

namespace mz {
namespace {

template <int MODE>
int launch_stoch_wide(int device, const StochWideParams& p, const StochWideShape& sh, size_t lds, hipStream_t stream,
                      std::string* err) {
  static mzh::LdsGrant granted;  // the kernel's dynamic-LDS limit, raised once per device
  if (!granted.covers(device, lds)) {
    const hipError_t attr_err = hipFuncSetAttribute(reinterpret_cast<const void*>(&mz_stoch_wide_kernel<MODE>),
                                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (attr_err != hipSuccess) {
      *err = std::string("hipFuncSetAttribute: ") + hipGetErrorString(attr_err);
      return MZS_E_RUNTIME;
    }
    granted.note(device, lds);
  }
  const int grid = (p.B + sh.waves - 1) / sh.waves;
  hipLaunchKernelGGL(mz_stoch_wide_kernel<MODE>, dim3(grid), dim3(64 * sh.waves), lds, stream, p, sh);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    *err = std::string("stochastic search kernel launch: ") + hipGetErrorString(e);
    return MZS_E_RUNTIME;
  }
  return MZS_OK;
}

}  // namespace

int stoch_wide_launch(bool tiebreak, int device, const StochWideParams& p, const WidePlan& pl, hipStream_t stream,
                      std::string* err) {
  const StochWideShape sh = {pl.rec_words, pl.root_words, pl.wg_words, pl.weight_words, pl.emb_lds, pl.waves};
  return tiebreak ? launch_stoch_wide<1>(device, p, sh, (size_t)pl.lds_bytes, stream, err)
                  : launch_stoch_wide<0>(device, p, sh, (size_t)pl.lds_bytes, stream, err);
}

}  // namespace mz

extern "C" int mzs_mlp_stochastic_plan(int32_t num_actions, int32_t num_chance_outcomes, int32_t embed_dim, int32_t support_size,
                                       int32_t num_simulations, int32_t out[4]) {
  mz::WidePlan pl;
  if (!out) return MZS_E_INVALID;
  if (support_size < 8 || support_size > 31) return MZS_E_UNSUPPORTED;
  if (mz::stoch_wide_plan(num_actions, num_chance_outcomes, embed_dim, 2 * support_size + 1, num_simulations, &pl))
    return MZS_E_UNSUPPORTED;
  out[0] = pl.waves;
  out[1] = pl.lds_bytes;
  out[2] = pl.roots_per_cu;
  out[3] = pl.emb_lds;
  return MZS_OK;
}

extern "C" int mzs_stochastic_search_block(const uint32_t key[2], int32_t num_simulations, float temperature,
                                           float dirichlet_fraction, uint32_t* out_words) {
  if (!out_words || num_simulations < 1) return MZS_E_INVALID;
  const uint32_t zero[2] = {0, 0};
  mzh::derive_keys(key ? key : zero, num_simulations, out_words, out_words + mz::kStochBlockHead);
  memcpy(out_words + 2, &temperature, sizeof(float));
  memcpy(out_words + 3, &dirichlet_fraction, sizeof(float));
  return MZS_OK;
}
