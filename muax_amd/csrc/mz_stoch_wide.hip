// mz_stoch_wide.hip -- the one-launch stochastic search kernel (mz_stoch_wide.cuh) and its host side: the launch, the LDS
// plan and the per-call device block of the C-ABI.
#include "mz_stoch_wide.cuh"

#include <cstring>

#include "../../include/mzsearch.h"
#include "mz_host.h"
#include "mz_keys.h"

namespace mz {

// the kernel's instantiation for (tie-break mode, ROOT, DRAW)
template <bool ROOT, bool DRAW>
static int launch_instance(bool tiebreak, int device, const StochWideParams& p, const StochWideShape& sh, size_t lds,
                           hipStream_t stream, std::string* err) {
  const char* what = "stochastic search kernel launch: ";
  return tiebreak ? launch_wave_per_root<mz_stoch_wide_kernel<1, ROOT, DRAW>>(what, device, p, sh, lds, stream, err)
                  : launch_wave_per_root<mz_stoch_wide_kernel<0, ROOT, DRAW>>(what, device, p, sh, lds, stream, err);
}

int stoch_wide_launch(bool tiebreak, bool root, bool draw, int device, const StochWideParams& p, const WidePlan& pl,
                      hipStream_t stream, std::string* err) {
  const StochWideShape sh = {pl.rec_words, pl.root_words, pl.wg_words, pl.weight_words, pl.emb_lds, pl.waves};
  const size_t lds = (size_t)pl.lds_bytes;
  if (draw)
    return root ? launch_instance<true, true>(tiebreak, device, p, sh, lds, stream, err)
                : launch_instance<false, true>(tiebreak, device, p, sh, lds, stream, err);
  return root ? launch_instance<true, false>(tiebreak, device, p, sh, lds, stream, err)
              : launch_instance<false, false>(tiebreak, device, p, sh, lds, stream, err);
}

int stoch_root_launch(const StochRootParams& p, hipStream_t stream, std::string* err) {
  const int grid = (p.B + kWideMaxWaves - 1) / kWideMaxWaves;
  hipLaunchKernelGGL(mz_stoch_root_kernel, dim3(grid), dim3(64 * kWideMaxWaves), 0, stream, p);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    *err = std::string("stochastic root kernel launch: ") + hipGetErrorString(e);
    return MZS_E_RUNTIME;
  }
  return MZS_OK;
}

}  // namespace mz

extern "C" int mzs_mlp_stochastic_plan(int32_t num_actions, int32_t num_chance_outcomes, int32_t embed_dim, int32_t support_size,
                                       int32_t num_simulations, int32_t out[4]) {
  mz::WidePlan pl;
  if (!out) return MZS_E_INVALID;
  if (support_size < 8 || support_size > 31) return MZS_E_UNSUPPORTED;
  if (mz::stoch_wide_plan(num_actions, num_chance_outcomes, embed_dim, 2 * support_size + 1, num_simulations, &pl))
    return MZS_E_UNSUPPORTED;
  mz::wide_plan_out(pl, out);
  return MZS_OK;
}

static const uint32_t kZeroKey[2] = {0, 0};

extern "C" int mzs_stochastic_search_block(const uint32_t key[2], int32_t num_simulations, float temperature,
                                           float dirichlet_fraction, uint32_t* out_words) {
  if (!out_words || num_simulations < 1) return MZS_E_INVALID;
  mzh::derive_keys(key ? key : kZeroKey, num_simulations, out_words, out_words + mz::kStochBlockHead);
  memcpy(out_words + 2, &temperature, sizeof(float));
  memcpy(out_words + 3, &dirichlet_fraction, sizeof(float));
  return MZS_OK;
}

extern "C" int mzs_stochastic_search_block_draw(const uint32_t key[2], int32_t num_simulations, float temperature,
                                                float dirichlet_fraction, float dirichlet_alpha, uint32_t* out_words) {
  if (int rc = mzs_stochastic_search_block(key, num_simulations, temperature, dirichlet_fraction, out_words)) return rc;
  uint32_t* tail = out_words + mz::kStochBlockHead + 2 * (size_t)num_simulations;
  mzh::h_split(key ? key : kZeroKey, 3, 1, tail);  // mctx: rng_key, dirichlet_rng_key, search_rng_key = split(rng_key, 3)
  memcpy(tail + 2, &dirichlet_alpha, sizeof(float));
  return MZS_OK;
}
