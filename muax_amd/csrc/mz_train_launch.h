// mz_train_launch.h -- host side of the fused training steps: THE launcher of a training kernel and its reduction
// (mz_train_blocks.cuh), shared by the instances built into libmzsearch.so (mz_train.hip, mz_stoch_train.hip) and the
// ones built on demand into side libraries (mz_train_jit.hip), and the checks and the argument-block fill that the
// library's two entries have in common.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "../../include/mzsearch.h"
#include "mz_host.h"
#include "mz_train_blocks.cuh"

namespace mz {

// what mzs_train_jit_abi() and a side library's mzs_jit_train_abi() must agree on: the layout of the argument block.
// Its size is in the number, so a field that grows TrainParamsT<18> moves it (row_w: 320 -> 328 bytes, 1320 -> 1328; beta
// took four bytes of padding in front of `ws`, every other field where it was: still 328), and a side library built
// against another block is refused at registration; a cached file from other sources is never loaded in the first place,
// since the file name carries the hash of the kernel's headers (muax_amd/_jit.py::_train_hash).
inline int train_jit_abi() { return MZS_ABI_VERSION * 1000 + (int)(sizeof(TrainParamsT<18>) % 1000); }
// ... and mzs_stochastic_train_jit_abi() with a side library's mzs_jit_stoch_train_abi() (mz_stoch_train_jit.hip): the
// block over the stochastic family's 34 arrays
inline int stoch_train_jit_abi() { return MZS_ABI_VERSION * 1000 + (int)(sizeof(TrainParamsT<34>) % 1000); }

// Both launches of one training step: `kern`, the main kernel of instance C (one kernel per C: the grant below is that
// kernel's), then the reduction over C::NA arrays.  The caller has validated `p` and selected the device.  MZS_OK, or an
// error code with its message in err[errlen], if given (a side library cannot reach the library's error slot: the caller
// files it).  An unroll beyond the instance's LDS is refused here, before any launch.
template <class C>
int launch_train(void (*kern)(const TrainParamsT<C::NA>), const TrainParamsT<C::NA>& p, hipStream_t stream, char* err,
                 int errlen) {
  auto put = [&](const char* what, hipError_t e) {
    if (err && errlen > 0) snprintf(err, (size_t)errlen, "%s: %s", what, hipGetErrorString(e));
    return (int)MZS_E_RUNTIME;
  };
  if (p.L > C::MAX_UNROLL) {
    if (err && errlen > 0)
      snprintf(err, (size_t)errlen, "unroll_steps %d too large for the LDS (at most %d for this %s)", p.L, C::MAX_UNROLL, C::DIMS);
    return MZS_E_UNSUPPORTED;
  }
  const size_t lds = sizeof(float) * ((size_t)C::WEIGHT_WORDS + (size_t)p.L * C::CK_WORDS_PER_STEP);
  static mzh::LdsGrant granted;  // (per device and instance: the attribute call is not free, update() runs every step)
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return put("hipGetDevice", e);
  if (!granted.covers(dev, lds)) {
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return put("hipFuncSetAttribute", e);
    granted.note(dev, lds);
  }
  hipLaunchKernelGGL(kern, dim3(p.waves / 4), dim3(256), lds, stream, p);
  if ((e = hipGetLastError()) != hipSuccess) return put("training kernel launch", e);
  hipLaunchKernelGGL(mz_train_reduce_kernel<C::NA>, dim3((p.off[C::NA] + 31) / 32), dim3(256), 0, stream, p);
  if ((e = hipGetLastError()) != hipSuccess) return put("reduction kernel launch", e);
  return MZS_OK;
}

// What mzs_mlp_loss_grad and mzs_stochastic_mlp_loss_grad do alike; each reports under its own name `who`.
namespace train_host {

inline int waves(int batch) { return 4 * ((batch + 15) / 16); }  // four per workgroup of 16 samples
inline int64_t workspace_bytes(int batch, int64_t num_params) {
  return (int64_t)waves(batch) * (num_params + 1) * (int64_t)sizeof(float);  // a row per wavefront: gradient + loss
}
template <int NA>
void offsets(const int (&sizes)[NA], int (&off)[NA + 1]) {
  off[0] = 0;
  for (int i = 0; i < NA; ++i) off[i + 1] = off[i] + sizes[i];
}
// the weight and argument structs (size fields, the NA weight pointers from repr_w on) and the batch's pointers
template <int NA, class W, class Args>
int check(const W* w, const Args* a, const char* who) {
  using mzh::fail;
  if (!w || w->struct_size != (int32_t)sizeof(W)) return fail(nullptr, MZS_E_INVALID, "%s: null weights or size mismatch (ABI)", who);
  if (!a || a->struct_size != (int32_t)sizeof(Args))
    return fail(nullptr, MZS_E_INVALID, "%s: null arguments or size mismatch (ABI)", who);
  const float* const* ptrs = &w->repr_w;
  for (int i = 0; i < NA; ++i)
    if (!ptrs[i]) return fail(nullptr, MZS_E_INVALID, "%s: null weight pointer", who);
  if (a->batch <= 0 || a->unroll_steps <= 0) return fail(nullptr, MZS_E_INVALID, "%s: batch and unroll_steps must be positive", who);
  if (!a->obs || !a->actions || !a->rewards || !a->returns || !a->policy || !a->loss || !a->grads || !a->workspace)
    return fail(nullptr, MZS_E_INVALID, "%s: null batch / output / workspace pointer", who);
  return MZS_OK;
}
// the argument block of checked `w` and `a`: everything but the offsets and beta, which stay zero
template <int NA, class W, class Args>
TrainParamsT<NA> params(const W& w, const Args& a, const float* row_w) {
  TrainParamsT<NA> p;
  memset(&p, 0, sizeof p);
  p.obs = a.obs; p.act = a.actions; p.rew = a.rewards; p.ret = a.returns; p.pi = a.policy;
  const float* const* ptrs = &w.repr_w;
  for (int i = 0; i < NA; ++i) p.w[i] = ptrs[i];
  p.B = a.batch; p.L = a.unroll_steps; p.obs_dim = w.obs_dim; p.support = w.support_size;
  p.loss_scale = a.loss_scale; p.l2 = a.l2_coeff;
  p.ws = static_cast<float*>(a.workspace); p.grads = a.grads; p.loss = a.loss;
  p.waves = waves(a.batch);
  p.row_w = row_w;
  return p;
}

}  // namespace train_host
}  // namespace mz
