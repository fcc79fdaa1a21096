// Weight-streaming MFMA GEMM for a dense block-scaled fp8 (e4m3fn) weight and 1-32 bf16 rows:
//   y[M, N] = x[M, K] . (W8[N, K] (.) scale)^T (+ bias), fp32 accumulation, one bf16 rounding,
// scale [N / 16, K / 128] fp32: one factor per 16 consecutive weight rows and 128 consecutive k
// (the 16 x 128 expansion of a 128 x 128 FP8 checkpoint's weight_scale_inv; Linear's
// "fp8_block" state).  The decode kernel of that format: gemm_fp8_small.hip's shape on
// wstream_core.h's product with WF = kWsFp8Block -- the operand layout, x through LDS, the K split
// over the 8 waves and the load pipeline are described there.
//
//   * the scale.  A workgroup's 32 weight rows are two 16-row A tiles = two scale groups, and a
//     k-step is 128 k = one scale block: per step and A tile the four MFMAs run into a zeroed step
//     accumulator and acc += scale * step follows on the vector ALU (4 MT fused multiply-adds per
//     A tile and step).  The result is the fp32 sum over the blocks of scale * (exact block sum);
//     the activations are never quantised and no dequantised weight exists anywhere.  This file
//     is compiled without packed fp32 instructions: the rescale stays scalar v_fma_f32, which the
//     CPU oracle mirrors (moe_fp8_block.hip).
//   * rows.  MT = 1 / 2 B tiles cover M <= 16 / 32; rows past M are clamped on load and never
//     stored.  M = 1 and 2 run here as well (15 / 14 of the 16 MFMA columns repeat row M - 1): the
//     1-2-row GEMV and its fused norm / RoPE prologues do not know this format.  N % 128 == 0
//     (the format's), so both A tiles of every workgroup are whole; the row clamp stays as the
//     sibling has it.
//   * parallelism.  kUnroll = 2 steps: 4 x kUnroll 16-byte weight loads and 2 x kUnroll scale
//     dwords in flight per lane, the sibling's bytes in flight.  From the ISA (no scratch, the
//     step accumulators add 4 MT registers per A tile); unmeasured against kUnroll = 4.  Against
//     bf16 (profiles/fp8_block/dense.json): 0.4-0.5 of its time at 8-32 rows of qkv / o shapes,
//     level at one row, slower on N = 4096, K = 12288 (128 workgroups, K split 8 ways only).
//   * epilogues.  C/D: lane (c, g) holds D[n = 4 g + e][m = c], e = 0..3.  Nothing is left but
//     the bias.  Plain: (+ bias) in fp32, one rounding, one 8-byte store.  SwiGLU
//     (swiglu_interleave'd weight rows: rows 32 b .. 32 b + 15 are the gates and 32 b + 16 ..
//     32 b + 31 the ups of output columns 16 b .. 16 b + 15): the two A tiles of the workgroup
//     hold gate and up of one output column in the same lane and register; each rounded to bf16
//     first, then silu(gate) * up -- ops.swiglu_interleaved on the bf16 product, bit for bit.
#include "wstream_core.h"

namespace dli {

namespace {

constexpr int kUnroll = 2;             // k-steps of weight loads in flight per lane

enum SmallEp { kSmallPlain = 0, kSmallSwiGLU = 1 };

template <int MT, int EPI>
__global__ void __launch_bounds__(kWsThreads)
small_gemm_fp8_block_kernel(const bf16* __restrict__ x, const uint8_t* __restrict__ W,
                            const float* __restrict__ bscale, const bf16* __restrict__ bias,
                            bf16* __restrict__ y, int M, int N, int K) {
  __shared__ __attribute__((aligned(1024))) char smem[kWsSmem<MT>];
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * kWsRowsWg;

  f32x4 acc[2][MT];
  if (!ws_accumulate<MT, kWsFp8Block, kUnroll>(
          smem, x, reinterpret_cast<const char*>(W), reinterpret_cast<const uint8_t*>(bscale), n0,
          K, [&](int n) { return min(n, N - 1); },       // weight rows past N: clamped into W
          [&](int row) { return min(row, M - 1); },      // image rows past M: clamped into x
          acc))
    return;

  // ---- epilogue: acc[a][b][e] = y[m = 16 b + r][n = n0 + 16 a + 4 g + e] ----
  if constexpr (EPI == kSmallSwiGLU) {
    const int I = N >> 1;
    const int col = 16 * (int)blockIdx.x + 4 * g;
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
        for (int e = 0; e < 4; ++e) {
          float v = acc[a][b][e];
          if (bias) v += (float)bias[n + e];
          o[e] = (bf16)v;
        }
        *reinterpret_cast<bf16x4*>(y + (size_t)m * N + n) = o;
      }
    }
  }
}

template <int MT>
void launch_t(bf16* y, const bf16* x, const uint8_t* W, const float* bscale, const bf16* bias,
              int M, int N, int K, bool swiglu, hipStream_t stream) {
  const int grid = N / kWsRowsWg;
  if (swiglu)
    small_gemm_fp8_block_kernel<MT, kSmallSwiGLU><<<grid, kWsThreads, 0, stream>>>(
        x, W, bscale, bias, y, M, N, K);
  else
    small_gemm_fp8_block_kernel<MT, kSmallPlain><<<grid, kWsThreads, 0, stream>>>(
        x, W, bscale, bias, y, M, N, K);
}

}  // namespace

int launch_small_gemm_fp8_block(bf16* y, const bf16* x, const uint8_t* W, const float* bscale,
                                const bf16* bias, int M, int N, int K, bool swiglu,
                                hipStream_t stream) {
  if (M < 1 || M > 32 || N <= 0 || N % 128 != 0 || K <= 0 || K % 128 != 0) return -1;
  if (swiglu && bias != nullptr) return -4;
  if (y == nullptr || x == nullptr || W == nullptr || bscale == nullptr) return -5;
  if (M <= 16) launch_t<1>(y, x, W, bscale, bias, M, N, K, swiglu, stream);
  else launch_t<2>(y, x, W, bscale, bias, M, N, K, swiglu, stream);
  return 0;
}

}  // namespace dli
