// mz_stoch_train_jit.hip -- ONE instance of the Stochastic MuZero fused training-step kernel (mz_stoch_train.cuh), built
// on demand into a side library: mz_train_jit.hip's twin for the default stochastic MLP family.
//
// libmzsearch.so carries mz_stoch_train_kernel for the (A, C, E, F) tuples listed in mzs_stochastic_mlp_loss_grad, at an
// observation cap of 32.  The host side (muax_amd/_jit.py::ensure_stochastic_train_instance) compiles THIS translation
// unit with -DMZ_STOCH_A=.. -DMZ_STOCH_C=.. -DMZ_STOCH_E=.. -DMZ_STOCH_F=.. -DMZ_STOCH_OB=.., loads it and hands
// mzs_jit_stoch_train_launch to mzs_register_stochastic_train_dispatch(): same kernel source, same arithmetic.
#if !defined(MZ_STOCH_A) || !defined(MZ_STOCH_C) || !defined(MZ_STOCH_E) || !defined(MZ_STOCH_F) || !defined(MZ_STOCH_OB)
#error "build through muax_amd/_jit.py"
#endif
#include "mz_stoch_train.cuh"
#include "mz_train_launch.h"

using Cfg = mz::StochTrainCfg<MZ_STOCH_A, MZ_STOCH_C, MZ_STOCH_E, MZ_STOCH_F, MZ_STOCH_OB>;
static_assert(Cfg::MAX_UNROLL >= 2, "not even L = 2 fits in LDS (_jit.stochastic_train_plan declines such a shape)");

// (argument block of mzs_stochastic_mlp_loss_grad's own launcher; the caller has validated it, matched obs_dim against
// the cap and selected the device)
extern "C" int mzs_jit_stoch_train_launch(const void* params, void* stream_, char* err, int errlen) {
  return mz::launch_train<Cfg>(mz::mz_stoch_train_kernel<Cfg>, *static_cast<const mz::StochTrainParams*>(params),
                               static_cast<hipStream_t>(stream_), err, errlen);
}
extern "C" void mzs_jit_stoch_train_shape(int32_t* A, int32_t* C, int32_t* E, int32_t* F, int32_t* OB) {
  *A = Cfg::A; *C = Cfg::C; *E = Cfg::E; *F = Cfg::F; *OB = Cfg::OB;
}
// StochTrainCfg's LDS plan: {WEIGHT_WORDS, CK_WORDS_PER_STEP, MAX_UNROLL} (_jit.stochastic_train_plan's arithmetic)
extern "C" void mzs_jit_stoch_train_plan(int32_t out[3]) {
  out[0] = Cfg::WEIGHT_WORDS; out[1] = Cfg::CK_WORDS_PER_STEP; out[2] = Cfg::MAX_UNROLL;
}
extern "C" int mzs_jit_stoch_train_abi(void) { return mz::stoch_train_jit_abi(); }
