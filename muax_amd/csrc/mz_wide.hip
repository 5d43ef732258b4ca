// mz_wide.hip -- the wide-action act() kernel (mz_wide.cuh) and its host side: the LDS plan and the launch.
#include "mz_wide.cuh"

#include "../../include/mzsearch.h"
#include "mz_host.h"

namespace mz {

int wide_dispatch(int mode, bool gumbel_ok, int device, const FusedParams& p, hipStream_t stream, int A, int E, int F,
                  std::string* err) {
  if (mode < 0 || mode > 3 || (mode >= 2 && !gumbel_ok)) return kNoFusedInstance;
  WidePlan pl;
  if (!wide_plan(A, E, F, p.S, mode >= 2, &pl)) return kNoFusedInstance;
  if (!pl.emb_lds && !p.export_tree && p.emb_scratch == nullptr) return kNeedEmbScratch;
  const WideShape sh = {A, E, F, pl.rec_words, pl.root_words, pl.wg_words, pl.weight_words, pl.emb_lds, pl.waves};
  const size_t lds = (size_t)pl.lds_bytes;
  switch (mode) {
    case 0: return launch_wave_per_root<mz_act_wide_kernel<0>>("wide kernel launch: ", device, p, sh, lds, stream, err);
    case 1: return launch_wave_per_root<mz_act_wide_kernel<1>>("wide kernel launch: ", device, p, sh, lds, stream, err);
    case 2: return launch_wave_per_root<mz_act_wide_kernel<2>>("wide kernel launch: ", device, p, sh, lds, stream, err);
    default: return launch_wave_per_root<mz_act_wide_kernel<3>>("wide kernel launch: ", device, p, sh, lds, stream, err);
  }
}

}  // namespace mz

extern "C" int mzs_mlp_wide_plan_policy(int32_t num_actions, int32_t embed_dim, int32_t support_size, int32_t num_simulations,
                                        int32_t policy, int32_t out[4]) {
  mz::WidePlan pl;
  if (!out || policy < 0 || policy > 1) return MZS_E_INVALID;
  if (!mz::wide_plan(num_actions, embed_dim, 2 * support_size + 1, num_simulations, policy == 1, &pl)) return MZS_E_UNSUPPORTED;
  mz::wide_plan_out(pl, out);
  return MZS_OK;
}
extern "C" int mzs_mlp_wide_plan(int32_t num_actions, int32_t embed_dim, int32_t support_size, int32_t num_simulations,
                                 int32_t out[4]) {
  if (!out) return MZS_E_UNSUPPORTED;
  return mzs_mlp_wide_plan_policy(num_actions, embed_dim, support_size, num_simulations, 0, out);
}
