// mz_wide.hip -- the wide-action act() kernel (mz_wide.cuh) and its host side: the LDS plan and the launch.
#include "mz_wide.cuh"

#include "../../include/mzsearch.h"
#include "mz_host.h"

namespace mz {
namespace {

template <bool TIEBREAK>
int launch_wide(int device, const FusedParams& p, const WideShape& sh, size_t lds, hipStream_t stream, std::string* err) {
  static mzh::LdsGrant granted;  // the kernel's dynamic-LDS limit, raised once per device
  if (!granted.covers(device, lds)) {
    const hipError_t attr_err = hipFuncSetAttribute(reinterpret_cast<const void*>(&mz_act_wide_kernel<TIEBREAK>),
                                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (attr_err != hipSuccess) {
      *err = std::string("hipFuncSetAttribute: ") + hipGetErrorString(attr_err);
      return MZS_E_RUNTIME;
    }
    granted.note(device, lds);
  }
  const int grid = (p.B + sh.waves - 1) / sh.waves;
  hipLaunchKernelGGL(mz_act_wide_kernel<TIEBREAK>, dim3(grid), dim3(64 * sh.waves), lds, stream, p, sh);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    *err = std::string("wide kernel launch: ") + hipGetErrorString(e);
    return MZS_E_RUNTIME;
  }
  return MZS_OK;
}

}  // namespace

int wide_dispatch(int mode, int device, const FusedParams& p, hipStream_t stream, int A, int E, int F, std::string* err) {
  if (mode >= 2) return kNoFusedInstance;  // the Gumbel policy stays on the generic route
  WidePlan pl;
  if (!wide_plan(A, E, F, p.S, &pl)) return kNoFusedInstance;
  if (!pl.emb_lds && !p.export_tree && p.emb_scratch == nullptr) return kNeedEmbScratch;
  const WideShape sh = {A, E, F, pl.rec_words, pl.root_words, pl.wg_words, pl.weight_words, pl.emb_lds, pl.waves};
  return mode == 1 ? launch_wide<true>(device, p, sh, (size_t)pl.lds_bytes, stream, err)
                   : launch_wide<false>(device, p, sh, (size_t)pl.lds_bytes, stream, err);
}

}  // namespace mz

extern "C" int mzs_mlp_wide_plan(int32_t num_actions, int32_t embed_dim, int32_t support_size, int32_t num_simulations,
                                 int32_t out[4]) {
  mz::WidePlan pl;
  if (!out || !mz::wide_plan(num_actions, embed_dim, 2 * support_size + 1, num_simulations, &pl)) return MZS_E_UNSUPPORTED;
  out[0] = pl.waves;
  out[1] = pl.lds_bytes;
  out[2] = pl.roots_per_cu;
  out[3] = pl.emb_lds;
  return MZS_OK;
}
