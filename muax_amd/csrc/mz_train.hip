// mz_train.hip -- training step of the default MLP trio (mzs_mlp_loss_grad, and mzs_mlp_loss_grad_weighted with a weight
// per batch row): the instances of mz_train.cuh built into the library, and the hand-over to the ones built on demand (mz_train_jit.hip through mzs_register_train_dispatch).
#include <hip/hip_runtime.h>

#include "mz_train.cuh"
#include "mz_train_launch.h"

using mzh::fail;
namespace th = mz::train_host;

static const char kWho[] = "mzs_mlp_loss_grad";

static void mlp_offsets(int obs_dim, int E, int A, int F, int (&off)[19]) {
  const int H = mz::TrainCfg<2, 8, 21>::H, X = E + A;  // (the hidden width is the same constant in every TrainCfg)
  const int sizes[18] = {obs_dim * E, E, E * H, H, H * F, F, E * H, H, H * A, A, X * H, H, H * F, F, X * H, H, H * E, E};
  th::offsets(sizes, off);
}

extern "C" {

int mzs_train_jit_abi(void) { return mz::train_jit_abi(); }

int64_t mzs_mlp_num_params(int32_t obs_dim, int32_t embed_dim, int32_t num_actions, int32_t support_size) {
  int off[19];
  mlp_offsets(obs_dim, embed_dim, num_actions, 2 * support_size + 1, off);
  return off[18];
}

int64_t mzs_mlp_train_workspace_bytes(int32_t batch, int32_t obs_dim, int32_t embed_dim, int32_t num_actions,
                                      int32_t support_size) {
  return th::workspace_bytes(batch, mzs_mlp_num_params(obs_dim, embed_dim, num_actions, support_size));
}

}  // extern "C"

// THE training step behind mzs_mlp_loss_grad (row_w null) and mzs_mlp_loss_grad_weighted: checks, argument block, the
// instance's two launches.  Both entries report under the first one's name.
static int loss_grad(const mzs_mlp_weights* w, const mzs_train_args* a, const float* row_w, void* stream_) {
  if (int rc = th::check<18>(w, a, kWho)) return rc;
  if (w->obs_dim <= 0 || w->obs_dim > 128) return fail(nullptr, MZS_E_UNSUPPORTED, "%s: obs_dim must be 1..128", kWho);
  const int A = a->num_actions, E = a->embed_dim, F = 2 * w->support_size + 1;
  if (a->workspace_bytes < mzs_mlp_train_workspace_bytes(a->batch, w->obs_dim, E, A, w->support_size))
    return fail(nullptr, MZS_E_INVALID, "%s: workspace too small", kWho);
  if (int rc = mzh::select_device(a->device, kWho)) return rc;
  mz::TrainParams p = th::params<18>(*w, *a, row_w);
  mlp_offsets(w->obs_dim, E, A, F, p.off);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  char msg[256] = "";
  auto filed = [&](int rc, const char* fmt) { return rc == MZS_OK ? MZS_OK : fail(nullptr, rc, fmt, msg); };
#define MZ_TRAIN_INST(a_, e_, f_)    \
  if (A == a_ && E == e_ && F == f_) \
    return filed(mz::launch_train<mz::TrainCfg<a_, e_, f_>>(mz::mz_train_kernel<mz::TrainCfg<a_, e_, f_>>, p, stream, msg, (int)sizeof msg), \
                 "mzs_mlp_loss_grad: %s");
  MZ_TRAIN_INST(2, 8, 21) MZ_TRAIN_INST(4, 32, 21) MZ_TRAIN_INST(3, 8, 21) MZ_TRAIN_INST(4, 8, 21)
  MZ_TRAIN_INST(2, 16, 21) MZ_TRAIN_INST(4, 16, 21)
  MZ_TRAIN_INST(2, 10, 21) MZ_TRAIN_INST(4, 10, 21)  // the reference notebooks
  MZ_TRAIN_INST(6, 8, 21) MZ_TRAIN_INST(8, 8, 21) MZ_TRAIN_INST(2, 32, 21)
  MZ_TRAIN_INST(2, 8, 31) MZ_TRAIN_INST(2, 8, 41)  // support_size 15, 20
#undef MZ_TRAIN_INST
  // an instance built on demand (mzs_register_train_dispatch; muax_amd/_jit.py)
  if (mzh::JitTrainLaunch fn = mzh::jit_train_instance(A, E, F))
    return filed(fn(&p, stream_, msg, (int)sizeof msg), "mzs_mlp_loss_grad (on-demand instance): %s");
  if (F < 17 || F > 63)  // no instance can exist: name the limit (callers still match "no kernel instance")
    return fail(nullptr, MZS_E_UNSUPPORTED,
                "mzs_mlp_loss_grad: no kernel instance for this (A, E, F): support_size must be 8..31");
  return fail(nullptr, MZS_E_UNSUPPORTED, "mzs_mlp_loss_grad: no kernel instance for this (A, E, F)");
}

extern "C" {

int mzs_mlp_loss_grad(const mzs_mlp_weights* w, const mzs_train_args* a, void* stream_) {
  return loss_grad(w, a, nullptr, stream_);
}

int mzs_mlp_loss_grad_weighted(const mzs_mlp_weights* w, const mzs_train_args* a, const float* sample_weight,
                               void* stream_) {
  if (!sample_weight) return fail(nullptr, MZS_E_INVALID, "mzs_mlp_loss_grad_weighted: null sample_weight");
  return loss_grad(w, a, sample_weight, stream_);
}

}  // extern "C"
