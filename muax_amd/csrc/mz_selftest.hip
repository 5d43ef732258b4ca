// mz_selftest.hip -- the entry points that need no handle and no tree: the device self-test of the hardware-dependent
// arithmetic identities (mzs_selftest) and the root exploration noise (mzs_dirichlet).
#include <hip/hip_runtime.h>

#include "mz_host.h"
#include "mz_dirichlet.cuh"

using mzh::fail;

extern "C" {  // (the self-test kernel too: its symbol has always been the plain selftest_kernel)

// ---- device self-test of the hardware-dependent arithmetic identities ----
namespace mz {
__global__ void selftest_kernel(unsigned long long* bad) {
  // every binary32 in [1, 4): sqrt_normal vs the IEEE sqrt; the same mantissas at 2^-9 .. 2^-2: div_two_eps vs x / 0.002f;
  // bad[2], bad[3]: see below
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;  // 2^24 threads
  const float x = __uint_as_float(0x3f800000u + i);
  unsigned long long b0 = sqrt_normal(x) != sqrtf(x);
  unsigned long long b1 = 0;
  for (int e = 118; e <= 125; ++e) {
    const float y = __uint_as_float(((uint32_t)e << 23) | (i & 0x7fffffu));
    b1 += div_two_eps(y) != y / 0.002f;
  }
  // shared-reciprocal division (rcp_newton2 / div_newton2) vs n / d: 2^24 denominators spread over [1, 64), each with
  // numerators 0, 2^-100, d itself, d's predecessor and eight pseudo-random ones in [2^-100, d]
  unsigned long long b2 = 0;
  {
    uint32_t h = i * 2654435761u + 0x9e3779b9u;
    const float d = __uint_as_float(((127u + i % 6u) << 23) | (h >> 9));
    const f32x2 dd = (f32x2){d, d};
    const f32x2 y = rcp_newton2(dd);
    float ns[12] = {0.0f, 0x1p-100f, d, __uint_as_float(__float_as_uint(d) - 1u)};
    for (int k = 4; k < 12; ++k) {
      h = h * 1664525u + 1013904223u;
      const uint32_t ex = 27u + (h >> 7) % 106u;  // 2^-100 .. 2^5
      h = h * 1664525u + 1013904223u;
      const float n = __uint_as_float((ex << 23) | (h >> 9));
      ns[k] = n <= d ? n : d * 0.37f;
    }
    for (int k = 0; k < 12; k += 2) {
      const f32x2 q = div_newton2((f32x2){ns[k], ns[k + 1]}, dd, y);
      b2 += (q.x != ns[k] / d) + (q.y != ns[k + 1] / d);
    }
  }
  // the same for the value scores' range: denominators (the span) spread over 2^-27 .. 2^41, numerators 0, the span
  // itself and pseudo-random ones in [2^-100, span]
  unsigned long long b3 = 0;
  {
    uint32_t h = i * 2246822519u + 0x85ebca6bu;
    const float d = __uint_as_float(((100u + i % 68u) << 23) | (h >> 9));
    const f32x2 dd = (f32x2){d, d};
    const f32x2 y = rcp_newton2(dd);
    float ns[8] = {0.0f, d};
    for (int k = 2; k < 8; ++k) {
      h = h * 1664525u + 1013904223u;
      const uint32_t ex = 27u + (h >> 7) % 142u;  // 2^-100 .. 2^41
      h = h * 1664525u + 1013904223u;
      const float n = __uint_as_float((ex << 23) | (h >> 9));
      ns[k] = n <= d ? n : d * 0.61f;
      ns[k] = ns[k] < 0x1p-100f ? 0x1p-100f : ns[k];
    }
    for (int k = 0; k < 8; k += 2) {
      const f32x2 q = div_newton2((f32x2){ns[k], ns[k + 1]}, dd, y);
      b3 += (q.x != ns[k] / d) + (q.y != ns[k + 1] / d);
    }
  }
  if (b0) atomicAdd(&bad[0], b0);
  if (b1) atomicAdd(&bad[1], b1);
  if (b2) atomicAdd(&bad[2], b2);
  if (b3) atomicAdd(&bad[3], b3);
}
}  // namespace mz

int mzs_selftest(int32_t device, int64_t* mismatches) {
  if (!mismatches) return fail(nullptr, MZS_E_INVALID, "mzs_selftest: null argument");
  if (int rc = mzh::select_device(device, "mzs_selftest")) return rc;
  unsigned long long* d = nullptr;
  MZS_HIP(nullptr, hipMalloc(reinterpret_cast<void**>(&d), 32));
  MZS_HIP(nullptr, hipMemset(d, 0, 32));
  hipLaunchKernelGGL(mz::selftest_kernel, dim3((1u << 24) / 256), dim3(256), 0, nullptr, d);
  unsigned long long h2[4] = {0, 0, 0, 0};
  hipError_t e = hipMemcpy(h2, d, 32, hipMemcpyDeviceToHost);
  hipFree(d);
  if (e != hipSuccess) return fail(nullptr, MZS_E_RUNTIME, "mzs_selftest: %s", hipGetErrorString(e));
  for (int i = 0; i < 4; ++i) mismatches[i] = (int64_t)h2[i];
  return MZS_OK;
}

// ---- root exploration noise ----
int mzs_dirichlet(int32_t device, const uint32_t key[2], float alpha, int32_t batch, int32_t num_actions,
                  int64_t global_batch, int64_t root_offset, float* out, void* stream_) {
  if (!key || !out) return fail(nullptr, MZS_E_INVALID, "mzs_dirichlet: null argument");
  if (batch <= 0 || num_actions <= 0 || num_actions > 64) return fail(nullptr, MZS_E_INVALID, "mzs_dirichlet: batch / num_actions (1..64)");
  if (!(alpha > 0.0f)) return fail(nullptr, MZS_E_INVALID, "mzs_dirichlet: alpha must be positive");
  if (global_batch <= 0) global_batch = batch;
  if (root_offset < 0 || root_offset + batch > global_batch)
    return fail(nullptr, MZS_E_INVALID, "mzs_dirichlet: root_offset + batch exceeds global_batch");
  if (int rc = mzh::select_device(device, "mzs_dirichlet")) return rc;
  const int R = (256 / mz::kSpec) / num_actions;  // roots per workgroup
  hipLaunchKernelGGL(mz::dirichlet_kernel, dim3((batch + R - 1) / R), dim3(256), sizeof(float) * (size_t)R * num_actions,
                     static_cast<hipStream_t>(stream_), key[0], key[1], alpha, batch, num_actions, (uint64_t)global_batch,
                     (uint64_t)root_offset, out);
  MZS_HIP(nullptr, hipGetLastError());
  return MZS_OK;
}

}  // extern "C"
