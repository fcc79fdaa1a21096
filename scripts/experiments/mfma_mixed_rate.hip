// Issue rate of v_mfma_scale_f32_16x16x128_f8f6f4 per operand-format pair: fp8 x fp8, fp4 x fp8
// (the pair gemm_fp4.hip issues: fp4 weights as A, e4m3 activations as B), fp8 x fp4 and
// fp4 x fp4.  One wave per SIMD, 4 independent accumulators, back-to-back issue.
//   pass 1: one workgroup, s_memtime ticks and wall ns (s_memrealtime, 100 MHz) per MFMA;
//   pass 2: one workgroup per CU, event-timed: dense TFLOP/s the whole chip sustains in this loop.
//   hipcc --offload-arch=gfx950 -O3 scripts/experiments/mfma_mixed_rate.hip -o tools_bin/mfma_mixed_rate
#include <hip/hip_runtime.h>
#include <cstdio>

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kAcc = 4, kInner = 4;   // 16 MFMAs per loop iteration

template <int CBSZ, int BLGP>
__global__ void __launch_bounds__(256) rate(float* out, unsigned long long* cyc, int iters) {
  const int lane = threadIdx.x & 63;
  i32x8 a, b;
  for (int j = 0; j < 8; ++j) {   // finite e4m3 bytes / any nibbles
    a[j] = (int)((0x9e3779b9u * (unsigned)(lane * 8 + j + 1)) & 0x77777777u);
    b[j] = (int)((0x85ebca6bu * (unsigned)(lane * 8 + j + 3)) & 0x77777777u);
  }
  f32x4 c[kAcc];
  for (int i = 0; i < kAcc; ++i) c[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();   // 100 MHz
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
#pragma unroll 1
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int r = 0; r < kInner; ++r)
#pragma unroll
      for (int i = 0; i < kAcc; ++i)
        c[i] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c[i], CBSZ, BLGP, 0, 120, 0, 120);
  }
  asm volatile("s_nop 0" : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]));
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  const unsigned long long r1 = __builtin_amdgcn_s_memrealtime();
  float s = 0.f;
  for (int i = 0; i < kAcc; ++i) s += c[i][0] + c[i][1] + c[i][2] + c[i][3];
  out[blockIdx.x * 256 + threadIdx.x] = s;
  if (lane == 0) {
    cyc[blockIdx.x * 8 + (threadIdx.x >> 6)] = t1 - t0;
    cyc[blockIdx.x * 8 + 4 + (threadIdx.x >> 6)] = r1 - r0;
  }
}

template <int CBSZ, int BLGP>
static void run(const char* name, float* out, unsigned long long* cyc, int cus) {
  const int iters = 20000;
  const double mfmas = (double)iters * kAcc * kInner;
  rate<CBSZ, BLGP><<<1, 256>>>(out, cyc, 1000);   // warm-up
  rate<CBSZ, BLGP><<<1, 256>>>(out, cyc, iters);
  unsigned long long h[8];
  hipMemcpy(h, cyc, sizeof(h), hipMemcpyDeviceToHost);
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  rate<CBSZ, BLGP><<<cus, 256>>>(out, cyc, 1000);
  float best = 1e30f;
  for (int rep = 0; rep < 5; ++rep) {
    hipEventRecord(e0);
    rate<CBSZ, BLGP><<<cus, 256>>>(out, cyc, iters);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms;
    hipEventElapsedTime(&ms, e0, e1);
    if (ms < best) best = ms;
  }
  const double flop = 2.0 * 16 * 16 * 128 * mfmas * 4 * cus;
  printf("{\"pair\": \"%s\", \"memtime_ticks_per_mfma\": %.2f, \"ns_per_mfma\": %.2f, "
         "\"chip_tflops\": %.0f, \"chip_ms\": %.3f}\n",
         name, (double)h[0] / mfmas, (double)h[4] * 10.0 / mfmas, flop / (best * 1e-3) / 1e12, best);
}

int main() {
  int cus = 0;
  hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0);
  float* out;
  unsigned long long* cyc;
  hipMalloc(&out, (size_t)cus * 256 * 4);
  hipMalloc(&cyc, (size_t)cus * 8 * 8);
  printf("{\"cus\": %d, \"loop\": \"1 wave / SIMD, 4 accumulators, 16 MFMAs per iteration\"}\n", cus);
  run<0, 0>("fp8(A) x fp8(B)", out, cyc, cus);
  run<4, 0>("fp4(A) x fp8(B)", out, cyc, cus);
  run<0, 4>("fp8(A) x fp4(B)", out, cyc, cus);
  run<4, 4>("fp4(A) x fp4(B)", out, cyc, cus);
  return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
