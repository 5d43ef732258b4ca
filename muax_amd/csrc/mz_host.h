// mz_host.h -- host-side helpers shared by the translation units of libmzsearch.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <string>

#include "../../include/mzsearch.h"

#define MZS_HIP(h, call)                                                                            \
  do {                                                                                              \
    hipError_t e_ = (call);                                                                         \
    if (e_ != hipSuccess) return mzh::fail(h, MZS_E_RUNTIME, #call ": %s", hipGetErrorString(e_));  \
  } while (0)

namespace mz {
struct StepArgs;
struct JumpArgs;
}  // namespace mz
namespace mzh {
// internals of a handle for the translation units that launch their own kernels on its step-wise tree (defined in
// mz_stepwise.hip): MZS_OK and the kernel argument blocks of the rooted tree with cached decisions, or an error (message
// set on the handle) when the handle has no such tree
int step_view(mzs_handle* h, mz::StepArgs* sa, mz::JumpArgs* ja, int* policy, const char* who, int* device = nullptr);
// THE error helper: formats the message onto the handle, or -- h == nullptr, an entry point without one -- into the
// thread's handle-less slot (mzs_last_error(NULL)), and returns `code`.  Defined in mz_api.hip
int fail(mzs_handle* h, int code, const char* fmt, const char* a = "");
// launcher of one training-step instance built on demand (mz_train_jit.hip; registered with mzs_register_train_dispatch,
// kept in mz_api.hip): the instance for (A, E, F = 2 support + 1), or nullptr
using JitTrainLaunch = int (*)(const void* train_params, void* stream, char* err, int errlen);
JitTrainLaunch jit_train_instance(int A, int E, int F);
// ... of the stochastic family's training step (mz_stoch_train_jit.hip; mzs_register_stochastic_train_dispatch): the
// instance for (A, C, E, F) whose observation cap is the smallest that holds obs_dim, or nullptr
JitTrainLaunch jit_stochastic_train_instance(int A, int C, int E, int F, int obs_dim);
// per-device record of what hipFuncSetAttribute(MaxDynamicSharedMemorySize) has already granted ONE kernel (one static
// LdsGrant per kernel instance).  Atomic: host threads that race can at worst both set the attribute (idempotent);
// device ordinals beyond the table are never recorded, so the attribute is then set on every call (no aliasing)
struct LdsGrant {
  std::atomic<size_t> have[64];
  bool covers(int device, size_t lds) const {
    return device >= 0 && device < 64 && have[device].load(std::memory_order_acquire) >= lds;
  }
  void note(int device, size_t lds) {
    if (device < 0 || device >= 64) return;
    size_t cur = have[device].load(std::memory_order_relaxed);
    while (cur < lds && !have[device].compare_exchange_weak(cur, lds, std::memory_order_release)) {
    }
  }
};
// `device` names a device this process can use, or the handle-less error is set: MZS_E_NODEVICE, then MZS_E_INVALID
inline int check_device(int device, const char* who) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, MZS_E_NODEVICE, "%s: no HIP device (this library has no CPU fallback)", who);
  if (device < 0 || device >= ndev) return fail(nullptr, MZS_E_INVALID, "%s: bad device ordinal", who);
  return MZS_OK;
}
// ... and makes it the calling thread's current device
inline int select_device(int device, const char* who) {
  if (int rc = check_device(device, who)) return rc;
  MZS_HIP(nullptr, hipSetDevice(device));
  return MZS_OK;
}

// the 18 weight pointers of the default MLP trio into a kernel argument block with the same member names
template <class D>
void copy_weights(const mzs_mlp_weights& w, D& d) {
  d.repr_w = w.repr_w; d.repr_b = w.repr_b;
  d.pv_w1 = w.pv_w1; d.pv_b1 = w.pv_b1; d.pv_w2 = w.pv_w2; d.pv_b2 = w.pv_b2;
  d.pp_w1 = w.pp_w1; d.pp_b1 = w.pp_b1; d.pp_w2 = w.pp_w2; d.pp_b2 = w.pp_b2;
  d.dr_w1 = w.dr_w1; d.dr_b1 = w.dr_b1; d.dr_w2 = w.dr_w2; d.dr_b2 = w.dr_b2;
  d.dn_w1 = w.dn_w1; d.dn_b1 = w.dn_b1; d.dn_w2 = w.dn_w2; d.dn_b2 = w.dn_b2;
}
}  // namespace mzh
