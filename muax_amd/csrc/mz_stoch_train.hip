// mz_stoch_train.hip -- training step of the default stochastic MLP family (mzs_stochastic_mlp_loss_grad): the listed
// instances of mz_stoch_train.cuh, the hand-over to the ones built on demand (mz_stoch_train_jit.hip through
// mzs_register_stochastic_train_dispatch) and the refusals of its own; the checks it shares with mzs_mlp_loss_grad and the
// launcher are mz_train_launch.h's.
#include <hip/hip_runtime.h>

#include "mz_stoch_train.cuh"
#include "mz_train_launch.h"

using mzh::fail;
namespace th = mz::train_host;

static const char kWho[] = "mzs_stochastic_mlp_loss_grad";
constexpr int NA = mz::STOCH_TRAIN_ARRAYS;

static void stoch_offsets(int obs_dim, int E, int A, int C, int F, int (&off)[NA + 1]) {
  const int H = 16, XA = E + A, XC = E + C;
  const int sizes[NA] = {
      obs_dim * E, E,
      XA * H, H, H * E, E,  E * H, H, H * F, F,  E * H, H, H * C, C,  XC * H, H, H * F, F,  XC * H, H, H * E, E,
      E * H, H, H * F, F,  E * H, H, H * A, A,
      obs_dim * H, H, H * C, C};
  th::offsets(sizes, off);
}

extern "C" {

int64_t mzs_stochastic_mlp_num_params(int32_t obs_dim, int32_t embed_dim, int32_t num_actions, int32_t num_chance_outcomes,
                                      int32_t support_size) {
  int off[NA + 1];
  stoch_offsets(obs_dim, embed_dim, num_actions, num_chance_outcomes, 2 * support_size + 1, off);
  return off[NA];
}

int64_t mzs_stochastic_mlp_train_workspace_bytes(int32_t batch, int32_t obs_dim, int32_t embed_dim, int32_t num_actions,
                                                 int32_t num_chance_outcomes, int32_t support_size) {
  return th::workspace_bytes(
      batch, mzs_stochastic_mlp_num_params(obs_dim, embed_dim, num_actions, num_chance_outcomes, support_size));
}

int mzs_stochastic_train_jit_abi(void) { return mz::stoch_train_jit_abi(); }

int mzs_stochastic_mlp_loss_grad(const mzs_stochastic_train_weights* w, const mzs_stochastic_train_args* a, void* stream_) {
  if (int rc = th::check<NA>(w, a, kWho)) return rc;
  const int A = a->num_actions, C = a->num_chance_outcomes, E = a->embed_dim, F = 2 * w->support_size + 1;
  // the listed instances (A, C, E, F): the three test shapes, 2048 at support 10, examples/fit_2048_stochastic.py
#define MZ_STOCH_TRAIN_LISTED(X) X(3, 2, 4, 17) X(4, 32, 16, 21) X(4, 17, 8, 17) X(4, 32, 32, 63)
  const bool listed_obs = w->obs_dim > 0 && w->obs_dim <= mz::STOCH_TRAIN_MAX_OBS;
  bool listed = false;
#define MZ_STOCH_TRAIN_IS(a_, c_, e_, f_) listed = listed || (A == a_ && C == c_ && E == e_ && F == f_);
  MZ_STOCH_TRAIN_LISTED(MZ_STOCH_TRAIN_IS)
#undef MZ_STOCH_TRAIN_IS
  // an instance built on demand (mzs_register_stochastic_train_dispatch; muax_amd/_jit.py), up to its own observation
  // cap: looked up where no listed instance serves the call, and BEFORE the refusals below, which are a call's answer only
  // when nothing is registered for it
  const mzh::JitTrainLaunch jit = (listed && listed_obs) ? nullptr : mzh::jit_stochastic_train_instance(A, C, E, F, w->obs_dim);
  if (!jit) {
    if (!listed_obs) return fail(nullptr, MZS_E_UNSUPPORTED, "%s: obs_dim must be 1..32", kWho);
    if (w->support_size < 8 || w->support_size > 31)
      return fail(nullptr, MZS_E_UNSUPPORTED, "%s: no kernel instance for this (A, C, E, F): support_size must be 8..31", kWho);
  }
  if (a->workspace_bytes < mzs_stochastic_mlp_train_workspace_bytes(a->batch, w->obs_dim, E, A, C, w->support_size))
    return fail(nullptr, MZS_E_INVALID, "%s: workspace too small", kWho);
  if (int rc = mzh::select_device(a->device, kWho)) return rc;
  mz::StochTrainParams p = th::params<NA>(*w, *a, a->sample_weight);
  stoch_offsets(w->obs_dim, E, A, C, F, p.off);
  p.beta = a->vqvae_beta;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  char msg[256] = "";
  if (jit) {
    const int rc = jit(&p, stream_, msg, (int)sizeof msg);
    return rc == MZS_OK ? MZS_OK : fail(nullptr, rc, "mzs_stochastic_mlp_loss_grad (on-demand instance): %s", msg);
  }
#define MZ_STOCH_TRAIN_INST(a_, c_, e_, f_)                                                              \
  if (A == a_ && C == c_ && E == e_ && F == f_) {                                                        \
    using Cf = mz::StochTrainCfg<a_, c_, e_, f_>;                                                        \
    const int rc = mz::launch_train<Cf>(mz::mz_stoch_train_kernel<Cf>, p, stream, msg, (int)sizeof msg); \
    return rc == MZS_OK ? MZS_OK : fail(nullptr, rc, "mzs_stochastic_mlp_loss_grad: %s", msg);           \
  }
  MZ_STOCH_TRAIN_LISTED(MZ_STOCH_TRAIN_INST)
#undef MZ_STOCH_TRAIN_INST
#undef MZ_STOCH_TRAIN_LISTED
  return fail(nullptr, MZS_E_UNSUPPORTED, "%s: no kernel instance for this (A, C, E, F)", kWho);
}

}  // extern "C"
