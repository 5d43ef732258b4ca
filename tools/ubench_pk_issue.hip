// ubench_pk_issue.hip -- what does ONE wave per SIMD pay for a packed f32 op on gfx950, against the two scalar ops
// that do the same work?  (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 against 2 x v_fma_f32 / v_mul_f32 / v_add_f32;
// a dependent stream -- each op reads the result of the one before on its chain -- and an independent one of four
// packed / eight scalar chains.)  The instructions are inline assembly, so the compiler can neither pack nor unpack.
// Build: hipcc --offload-arch=gfx950 -O3 tools/ubench_pk_issue.hip -o tools/bin/ubench_pk_issue
#include <hip/hip_runtime.h>
#include <cstdio>
typedef float f32x2 __attribute__((ext_vector_type(2)));
enum { FMA = 0, MUL = 1, ADD = 2 };
constexpr int kUnroll = 16;

// NP packed chains: per round NP packed instructions = 2 NP scalar results
template <int OP, int NP>
__global__ __launch_bounds__(256) void k_packed(float* out, int iters, float a, float b) {
  f32x2 x[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) x[i] = (f32x2){threadIdx.x * 0.001f + i, threadIdx.x * 0.002f + i};
  const f32x2 a2 = (f32x2){a, a}, b2 = (f32x2){b, b};
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int r = 0; r < kUnroll; ++r) {
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        if constexpr (OP == FMA) asm volatile("v_pk_fma_f32 %0, %0, %1, %2" : "+v"(x[i]) : "v"(a2), "v"(b2));
        if constexpr (OP == MUL) asm volatile("v_pk_mul_f32 %0, %0, %1" : "+v"(x[i]) : "v"(a2));
        if constexpr (OP == ADD) asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(x[i]) : "v"(b2));
      }
    }
  }
  float s = 0;
#pragma unroll
  for (int i = 0; i < NP; ++i) s += x[i].x + x[i].y;
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}
// the same work in scalar form: 2 NP chains, per round 2 NP scalar instructions
template <int OP, int NP>
__global__ __launch_bounds__(256) void k_scalar(float* out, int iters, float a, float b) {
  float x[2 * NP];
#pragma unroll
  for (int i = 0; i < 2 * NP; ++i) x[i] = threadIdx.x * 0.001f * (1 + (i & 1)) + (i >> 1);
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int r = 0; r < kUnroll; ++r) {
#pragma unroll
      for (int i = 0; i < 2 * NP; ++i) {
        if constexpr (OP == FMA) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(x[i]) : "v"(a), "v"(b));
        if constexpr (OP == MUL) asm volatile("v_mul_f32 %0, %0, %1" : "+v"(x[i]) : "v"(a));
        if constexpr (OP == ADD) asm volatile("v_add_f32 %0, %0, %1" : "+v"(x[i]) : "v"(b));
      }
    }
  }
  float s = 0;
#pragma unroll
  for (int i = 0; i < 2 * NP; ++i) s += x[i];
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}
template <class F>
float time_it(F f) {
  hipEvent_t a, b;
  hipEventCreate(&a); hipEventCreate(&b);
  f();
  hipDeviceSynchronize();
  float best = 1e30f;
  for (int rep = 0; rep < 3; ++rep) {  // best of three: the first timed launch may still see the clocks ramp
    hipEventRecord(a);
    f();
    hipEventRecord(b);
    hipEventSynchronize(b);
    float ms;
    hipEventElapsedTime(&ms, a, b);
    best = ms < best ? ms : best;
  }
  hipEventDestroy(a); hipEventDestroy(b);
  return best;
}
template <int OP, int NP>
void run_pair(const char* op, const char* stream, float* out, int blocks) {
  const int iters = 20000;
  const double ghz = 2.4;
  const float pk = time_it([&] { hipLaunchKernelGGL((k_packed<OP, NP>), dim3(blocks), dim3(256), 0, 0, out, iters, 1.0001f, 0.5f); });
  const float sc = time_it([&] { hipLaunchKernelGGL((k_scalar<OP, NP>), dim3(blocks), dim3(256), 0, 0, out, iters, 1.0001f, 0.5f); });
  const double per = 1e-3 * ghz * 1e9 / ((double)iters * kUnroll * NP);  // cycles per (one packed op | two scalar ops)
  printf("%-4s %-12s  v_pk_*: %8.3f ms %6.2f cyc/op    2 x scalar: %8.3f ms %6.2f cyc/pair    packed / scalar pair = %.3f\n",
         op, stream, pk, pk * per, sc, sc * per, pk / sc);
}
int main() {
  int dev = 0;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) { printf("no device\n"); return 1; }
  const int blocks = prop.multiProcessorCount;  // 256 threads per block: one wave on each of a CU's four SIMDs
  float* out;
  if (hipMalloc(&out, (size_t)blocks * 256 * sizeof(float)) != hipSuccess) { printf("hipMalloc failed\n"); return 1; }
  printf("%s, %d CUs, one wave per SIMD, cycles at an assumed 2.4 GHz\n", prop.gcnArchName, blocks);
  run_pair<FMA, 1>("fma", "dependent", out, blocks);
  run_pair<FMA, 4>("fma", "independent", out, blocks);
  run_pair<MUL, 1>("mul", "dependent", out, blocks);
  run_pair<MUL, 4>("mul", "independent", out, blocks);
  run_pair<ADD, 1>("add", "dependent", out, blocks);
  run_pair<ADD, 4>("add", "independent", out, blocks);
  if (hipDeviceSynchronize() != hipSuccess) { printf("device error\n"); return 1; }
  hipFree(out);
  return 0;
}
