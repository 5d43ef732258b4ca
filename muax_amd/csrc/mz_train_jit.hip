// mz_train_jit.hip -- ONE instance of the fused training-step kernel (mz_train.cuh), built on demand into a side library.
//
// The reference's update() (muax/model.py:181-201 through jax.value_and_grad of muax/loss.py:10-88) takes whatever
// widths its nets have; libmzsearch.so carries mz_train_kernel for the (num_actions, embedding_dim, 2 support_size + 1)
// triples listed in mzs_mlp_loss_grad.  Since round 5 act() serves other shapes of the default trio through instances
// built on demand (mz_fused_jit.hip); this is the same for the training step, so that such a model's update() does not
// drop to framework autograd (14 - 22 ms against 0.06 ms at 4096 x 10).  The host side (muax_amd/_jit.py) compiles THIS
// translation unit with -DMZ_TRAIN_A=.. -DMZ_TRAIN_E=.. -DMZ_TRAIN_F=.., loads it and hands mzs_jit_train_launch to
// mzs_register_train_dispatch(): same kernel source, same arithmetic.  With -DMZ_TRAIN_WIDE=1 on top
// (_jit.ensure_wide_train_instance) the same unit serves 17 to 64 actions: mz_train.cuh lifts its one-slot assertion.
#if !defined(MZ_TRAIN_A) || !defined(MZ_TRAIN_E) || !defined(MZ_TRAIN_F)
#error "build through muax_amd/_jit.py"
#endif
#include "mz_train.cuh"
#include "mz_train_launch.h"

// (argument block of mzs_mlp_loss_grad's own launcher; the caller has validated it and selected the device)
extern "C" int mzs_jit_train_launch(const void* params, void* stream_, char* err, int errlen) {
  using Cfg = mz::TrainCfg<MZ_TRAIN_A, MZ_TRAIN_E, MZ_TRAIN_F>;
  return mz::launch_train<Cfg>(mz::mz_train_kernel<Cfg>, *static_cast<const mz::TrainParams*>(params),
                               static_cast<hipStream_t>(stream_), err, errlen);
}
extern "C" void mzs_jit_train_shape(int32_t* A, int32_t* E, int32_t* F) {
  *A = MZ_TRAIN_A; *E = MZ_TRAIN_E; *F = MZ_TRAIN_F;
}
extern "C" int mzs_jit_train_abi(void) { return mz::train_jit_abi(); }
