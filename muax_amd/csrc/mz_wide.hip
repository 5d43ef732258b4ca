// mz_wide.hip -- the wide-action act() kernel (mz_wide.cuh) and its host side: the LDS plan and the launch.
#include "mz_wide.cuh"

#include "../../include/mzsearch.h"
#include "mz_host.h"

namespace mz {
namespace {

template <int MODE>
int launch_wide(int device, const FusedParams& p, const WideShape& sh, size_t lds, hipStream_t stream, std::string* err) {
  static mzh::LdsGrant granted;  // the kernel's dynamic-LDS limit, raised once per device
  if (!granted.covers(device, lds)) {
    const hipError_t attr_err = hipFuncSetAttribute(reinterpret_cast<const void*>(&mz_act_wide_kernel<MODE>),
                                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (attr_err != hipSuccess) {
      *err = std::string("hipFuncSetAttribute: ") + hipGetErrorString(attr_err);
      return MZS_E_RUNTIME;
    }
    granted.note(device, lds);
  }
  const int grid = (p.B + sh.waves - 1) / sh.waves;
  hipLaunchKernelGGL(mz_act_wide_kernel<MODE>, dim3(grid), dim3(64 * sh.waves), lds, stream, p, sh);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    *err = std::string("wide kernel launch: ") + hipGetErrorString(e);
    return MZS_E_RUNTIME;
  }
  return MZS_OK;
}

}  // namespace

int wide_dispatch(int mode, bool gumbel_ok, int device, const FusedParams& p, hipStream_t stream, int A, int E, int F,
                  std::string* err) {
  if (mode < 0 || mode > 3 || (mode >= 2 && !gumbel_ok)) return kNoFusedInstance;
  WidePlan pl;
  if (!wide_plan(A, E, F, p.S, mode >= 2, &pl)) return kNoFusedInstance;
  if (!pl.emb_lds && !p.export_tree && p.emb_scratch == nullptr) return kNeedEmbScratch;
  const WideShape sh = {A, E, F, pl.rec_words, pl.root_words, pl.wg_words, pl.weight_words, pl.emb_lds, pl.waves};
  const size_t lds = (size_t)pl.lds_bytes;
  switch (mode) {
    case 0: return launch_wide<0>(device, p, sh, lds, stream, err);
    case 1: return launch_wide<1>(device, p, sh, lds, stream, err);
    case 2: return launch_wide<2>(device, p, sh, lds, stream, err);
    default: return launch_wide<3>(device, p, sh, lds, stream, err);
  }
}

}  // namespace mz

extern "C" int mzs_mlp_wide_plan_policy(int32_t num_actions, int32_t embed_dim, int32_t support_size, int32_t num_simulations,
                                        int32_t policy, int32_t out[4]) {
  mz::WidePlan pl;
  if (!out || policy < 0 || policy > 1) return MZS_E_INVALID;
  if (!mz::wide_plan(num_actions, embed_dim, 2 * support_size + 1, num_simulations, policy == 1, &pl)) return MZS_E_UNSUPPORTED;
  out[0] = pl.waves;
  out[1] = pl.lds_bytes;
  out[2] = pl.roots_per_cu;
  out[3] = pl.emb_lds;
  return MZS_OK;
}
extern "C" int mzs_mlp_wide_plan(int32_t num_actions, int32_t embed_dim, int32_t support_size, int32_t num_simulations,
                                 int32_t out[4]) {
  if (!out) return MZS_E_UNSUPPORTED;
  return mzs_mlp_wide_plan_policy(num_actions, embed_dim, support_size, num_simulations, 0, out);
}
