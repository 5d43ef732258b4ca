// mz_wide_launch.h -- host interface of the wide-action act() kernel (mz_wide.cuh, compiled in mz_wide.hip).
#pragma once
#include <string>

#include "mz_fused_launch.h"
#include "mz_host.h"

namespace mz {

constexpr int kWideLdsPerCu = 160 * 1024;  // bytes of LDS of a CU; one workgroup may take all of it
constexpr int kWideMaxWaves = 4;           // roots (= wavefronts) per workgroup

// LDS budget of the wide kernel, in 4-byte words (all blocks rounded to 16 bytes):
//   workgroup: the four nets' weights (the representation's stay in HBM: read once per root) + the pUCT table [S + 2]
//   root:      (S + 1) records of 4 header words + 4 child fields x A (5 under the Gumbel policy: the prior logits as
//              well), the path [S + 1], and -- when it costs no resident root -- the embeddings [S + 1][E]
struct WidePlan {
  int waves, emb_lds, rec_words, root_words, wg_words, weight_words, roots_per_cu;
  int lds_bytes;
};
inline int wide_round4(int w) { return (w + 3) & ~3; }
inline int wide_weight_words(int A, int E, int F) {
  const int H = kHidden, X = E + A;
  return (E * H + H + H * F + F) + (E * H + H + H * A + A) + (X * H + H + H * F + F) + (X * H + H + H * E + E);
}
// The split of a CU's LDS that keeps most roots resident, for a kernel of this mapping (mz_wide.cuh, mz_stoch_wide.cuh):
// `wgt` weight words (rounded) and the pUCT table per workgroup, per root S + 1 records of `rec` words, the path and --
// when it costs no resident root -- the embeddings.  false: one root does not fit
inline bool wide_fit(int wgt, int rec, int E, int S, WidePlan* out) {
  WidePlan best{};
  const int N = S + 1, wg = wgt + wide_round4(S + 2);
  for (int emb = 1; emb >= 0; --emb)
    for (int w = 1; w <= kWideMaxWaves; ++w) {
      const int root = wide_round4(N * rec + N + (emb ? N * E : 0));
      const long bytes = 4L * (wg + (long)w * root);
      if (bytes > kWideLdsPerCu) continue;
      int roots = (int)(kWideLdsPerCu / bytes) * w;
      roots = roots > 32 ? 32 : roots;  // (a CU holds 32 wavefronts)
      if (roots > best.roots_per_cu) best = WidePlan{w, emb, rec, root, wg, wgt, roots, (int)bytes};  // ties: embeddings in LDS, fewer waves
    }
  if (best.roots_per_cu == 0) return false;
  *out = best;
  return true;
}
// false: the wide kernel declines the shape (also when one root does not fit a CU's LDS)
// gumbel: the plan of the Gumbel MuZero modes (the larger record: fewer resident roots, a smaller largest S)
inline bool wide_plan(int A, int E, int F, int S, bool gumbel, WidePlan* out) {
  if (A < 17 || A > 64 || E < 1 || E > 64 || F < 17 || F > 63 || S < 1 || S > 255) return false;
  return wide_fit(wide_round4(wide_weight_words(A, E, F)), 4 + (gumbel ? 5 : 4) * A, E, S, out);
}
// what the plan entries of the C-ABI report
inline void wide_plan_out(const WidePlan& pl, int32_t out[4]) {
  out[0] = pl.waves, out[1] = pl.lds_bytes, out[2] = pl.roots_per_cu, out[3] = pl.emb_lds;
}

// Launch of a kernel of this mapping (one root per wavefront, sh.waves roots per workgroup, `lds` bytes of dynamic LDS):
// MZS_OK, or MZS_E_RUNTIME with *err = the HIP error (`what` in front of a launch error)
template <auto Kernel, class Params, class Shape>
int launch_wave_per_root(const char* what, int device, const Params& p, const Shape& sh, size_t lds, hipStream_t stream,
                         std::string* err) {
  static mzh::LdsGrant granted;  // the kernel's dynamic-LDS limit, raised once per device
  if (!granted.covers(device, lds)) {
    const hipError_t attr_err =
        hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (attr_err != hipSuccess) {
      *err = std::string("hipFuncSetAttribute: ") + hipGetErrorString(attr_err);
      return MZS_E_RUNTIME;
    }
    granted.note(device, lds);
  }
  const int grid = (p.B + sh.waves - 1) / sh.waves;
  hipLaunchKernelGGL(Kernel, dim3(grid), dim3(64 * sh.waves), lds, stream, p, sh);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    *err = std::string(what) + hipGetErrorString(e);
    return MZS_E_RUNTIME;
  }
  return MZS_OK;
}

// mode: that of the fused dispatchers (0 / 1 MuZero policy, 2 / 3 Gumbel policy); the Gumbel modes are served only with
// `gumbel_ok` (mzs_mlp_allow_wide_gumbel).  MZS_OK after the launch, kNoFusedInstance when the kernel declines the
// shape or the policy, kNeedEmbScratch when it keeps this shape's embeddings in HBM and neither a tree export nor
// p.emb_scratch is there, or a negative MZS_E_* with *err set.
int wide_dispatch(int mode, bool gumbel_ok, int device, const FusedParams& p, hipStream_t stream, int A, int E, int F,
                  std::string* err);

}  // namespace mz
