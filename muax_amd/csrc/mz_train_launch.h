// mz_train_launch.h -- THE launcher of the fused training-step kernel (mz_train.cuh), shared by the instances built
// into libmzsearch.so (mz_train.hip) and the ones built on demand into side libraries (mz_train_jit.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>

#include "../../include/mzsearch.h"
#include "mz_host.h"
#include "mz_train.cuh"

namespace mz {

// what mzs_train_jit_abi() and a side library's mzs_jit_train_abi() must agree on: the layout of the argument block.
// Its size is in the number, so a field added to TrainParams (row_w: 320 -> 328 bytes, 1320 -> 1328) moves it, and a side
// library built against the earlier block is refused at registration; its cached file is never loaded in the first
// place, since the file name carries the hash of mz_train.cuh (muax_amd/_jit.py::_train_hash).
inline int train_jit_abi() { return MZS_ABI_VERSION * 1000 + (int)(sizeof(TrainParams) % 1000); }
// Both launches of one training step for instance C; the caller has validated `p` and selected the device.  MZS_OK, or an
// error code with its message in err[errlen], if given (a side library cannot reach the library's error slot: the caller files it)
template <class C>
int launch_train(const TrainParams& p, hipStream_t stream, char* err, int errlen) {
  auto put = [&](const char* what, hipError_t e) {
    if (err && errlen > 0) snprintf(err, (size_t)errlen, "%s: %s", what, hipGetErrorString(e));
    return (int)MZS_E_RUNTIME;
  };
  if (p.L > C::MAX_UNROLL) {
    if (err && errlen > 0)
      snprintf(err, (size_t)errlen, "unroll_steps %d too large for the LDS (at most %d for this (A, E, F))", p.L, C::MAX_UNROLL);
    return MZS_E_UNSUPPORTED;
  }
  const size_t lds = sizeof(float) * ((size_t)C::WEIGHT_WORDS + (size_t)p.L * C::CK_WORDS_PER_STEP);
  auto kern = mz_train_kernel<C>;
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
  hipLaunchKernelGGL(mz_train_reduce_kernel, dim3((p.off[18] + 31) / 32), dim3(256), 0, stream, p);
  if ((e = hipGetLastError()) != hipSuccess) return put("reduction kernel launch", e);
  return MZS_OK;
}

}  // namespace mz
