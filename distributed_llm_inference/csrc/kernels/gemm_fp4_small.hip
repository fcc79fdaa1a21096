// Weight-streaming MFMA GEMM for MXFP4 weights and 3-32 bf16 activation rows:
//   y[M, N] = x[M, K] . dequant(W, bscale)[N, K]^T (+ bias), fp32 accumulation, one bf16 rounding.
// The regime between the fp4 GEMV (gemv.hip, 1-2 rows) and the 256 x 256 tile GEMM (gemm_fp4.hip).
// The product is wstream_core.h's (WF = kWsFp4: the operand layout, x through LDS, the K split
// over the waves and the load pipeline are described there): every weight byte is read once, at
// 17/32 byte per weight, as the GEMV reads it, and the activations stay bf16.  The result is the
// dequantise path's product up to summation order.
//
//   * rows.  MT = 1 / 2 B tiles cover M <= 16 / 32; rows past M (and weight rows past N, when
//     N % 32 == 16) are clamped on load and never stored.
//   * parallelism.  kUnroll = 4 steps = 2 x kUnroll 16-byte weight loads in flight per lane.
//   * epilogues.  C/D: lane (c, g) holds D[n = 4 g + e][m = c], e = 0..3 -- four consecutive
//     output columns of activation row c.  Plain: + bias in fp32, one rounding, one 8-byte store.
//     SwiGLU (swiglu_interleave'd weight rows: rows 32 b .. 32 b + 15 are the gates and
//     32 b + 16 .. 32 b + 31 the ups of output columns 16 b .. 16 b + 15): the two A tiles of the
//     workgroup hold gate and up of one output column in the same lane and register; both are
//     rounded to bf16 first, then silu(gate) * up -- ops.swiglu_interleaved on the bf16 product,
//     bit for bit.
#include "wstream_core.h"

namespace dli {

namespace {

constexpr int kUnroll = 4;             // k-steps of weight loads in flight per lane

enum SmallEp { kSmallPlain = 0, kSmallSwiGLU = 1 };

template <int MT, int EPI>
__global__ void __launch_bounds__(kWsThreads)
small_gemm_fp4_kernel(const bf16* __restrict__ x, const uint8_t* __restrict__ W,
                      const uint8_t* __restrict__ bscale, const bf16* __restrict__ bias,
                      bf16* __restrict__ y, int M, int N, int K) {
  __shared__ __attribute__((aligned(1024))) char smem[kWsSmem<MT>];
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * kWsRowsWg;

  f32x4 acc[2][MT];
  if (!ws_accumulate<MT, kWsFp4, kUnroll>(
          smem, x, reinterpret_cast<const char*>(W), bscale, n0, K,
          [&](int n) { return min(n, N - 1); },          // weight rows past N: clamped into W
          [&](int row) { return min(row, M - 1); },      // image rows past M: clamped into x
          acc))
    return;

  // ---- epilogue: acc[a][b][e] = y[m = 16 b + r][n = n0 + 16 a + 4 g + e] ----
  if constexpr (EPI == kSmallSwiGLU) {
    const int I = N >> 1;
    const int col = 16 * (int)blockIdx.x + 4 * g;   // N % 32 == 0: both tiles are whole
#pragma unroll
    for (int b = 0; b < MT; ++b) {
      const int m = 16 * b + r;
      if (m >= M) continue;
      bf16x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float gt = (float)(bf16)acc[0][b][e];
        const float up = (float)(bf16)acc[1][b][e];
        o[e] = (bf16)(silu(gt) * up);
      }
      *reinterpret_cast<bf16x4*>(y + (size_t)m * I + col) = o;
    }
  } else {
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int n = n0 + 16 * a + 4 * g;
      if (n >= N) continue;   // N % 16 == 0: a tile is whole or absent
#pragma unroll
      for (int b = 0; b < MT; ++b) {
        const int m = 16 * b + r;
        if (m >= M) continue;
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          o[e] = (bf16)(acc[a][b][e] + (bias ? (float)bias[n + e] : 0.f));
        *reinterpret_cast<bf16x4*>(y + (size_t)m * N + n) = o;
      }
    }
  }
}

template <int MT>
void launch_t(bf16* y, const bf16* x, const uint8_t* W, const uint8_t* bscale, const bf16* bias,
              int M, int N, int K, bool swiglu, hipStream_t stream) {
  const int grid = (N + kWsRowsWg - 1) / kWsRowsWg;
  if (swiglu)
    small_gemm_fp4_kernel<MT, kSmallSwiGLU><<<grid, kWsThreads, 0, stream>>>(x, W, bscale, bias, y,
                                                                         M, N, K);
  else
    small_gemm_fp4_kernel<MT, kSmallPlain><<<grid, kWsThreads, 0, stream>>>(x, W, bscale, bias, y,
                                                                        M, N, K);
}

}  // namespace

int launch_small_gemm_fp4(bf16* y, const bf16* x, const uint8_t* W, const uint8_t* bscale,
                          const bf16* bias, int M, int N, int K, bool swiglu,
                          hipStream_t stream) {
  if (M < 3 || M > 32 || N <= 0 || N % 16 != 0 || K <= 0 || K % 128 != 0) return -1;
  if (swiglu && (N % 32 != 0 || bias != nullptr)) return -4;
  if (y == nullptr || x == nullptr || W == nullptr || bscale == nullptr) return -5;
  if (M <= 16) launch_t<1>(y, x, W, bscale, bias, M, N, K, swiglu, stream);
  else launch_t<2>(y, x, W, bscale, bias, M, N, K, swiglu, stream);
  return 0;
}

}  // namespace dli
