// The grouped weight-streaming MFMA GEMM of the sparse-MoE MLP (described in moe.hip): the kernel
// template and its launcher, shared by moe.hip (bf16, per-row fp8 and MXFP4 experts) and
// moe_fp8_block.hip (block-scaled fp8 experts, whose in-loop rescale is fp32 vector arithmetic and
// is compiled without packed fp32 instructions: a translation unit of its own, so that the other
// three formats keep the code they have).
#pragma once
#include "wstream_core.h"

namespace dli {

// launch_moe_grouped_gemm for W.format == kExpertFp8Block (moe_fp8_block.hip); `wscale` is the
// [E, N / 16, K / 128] fp32 table
int launch_moe_grouped_fp8_block(bf16* out, const bf16* x, const void* W, const void* wscale,
                                 const int* sorted_pairs, const int* tile_expert,
                                 const int* tile_start, const int* tile_rows, const int* n_tiles,
                                 int cap, int T, int E, int k, int N, int K, int epilogue,
                                 hipStream_t stream);

namespace {

constexpr int kMaxExperts = 256;
constexpr int kMaxTopK = 8;

// ------------------------------------------------------------------------------------- grouped GEMM
constexpr int kTileRows = 32;          // activation rows per tile: two 16-column B tiles

enum MoeEp { kMoeGateUp = 0, kMoeDown = 1 };
enum MoeWf { kMoeBf16 = kWsBf16, kMoeFp8 = kWsFp8, kMoeFp4 = kWsFp4, kMoeFp8Block = kWsFp8Block };

// k-steps of weight loads in flight per lane: 8 (bf16) / 4 (fp8) 16-byte loads per step, 16
// loads in flight either way (fp8 with 2 measured 0-4 % slower: docs/kernels.md); fp4 has 2
// 16-byte loads and 2 scale bytes per step: 4 + 4 in flight with 2, which measured 0-7 % faster
// than 4 and 8 at 1-16 rows and 4-5 % slower than 4 at Mixtral's 128 / 512 rows (docs/kernels.md).
// Block-scaled fp8 takes fp8's 4 (16 weight loads and 8 scale dwords in flight): chosen from the
// ISA (registers, no scratch: docs/kernels.md), not measured against 2
template <int WF> constexpr int kUnrollOf = (WF == kMoeFp8 || WF == kMoeFp8Block) ? 4 : 2;

__device__ __forceinline__ int clamp_pair(int p, int P) { return min(max(p, 0), P - 1); }

// One tile: `rows` (1 .. 16 MT) activation rows x the 32 weight rows n0 .. n0 + 31 of W [N, K].
// pairs = sorted_pairs + start.  W is the expert's [N, K] bf16 (WF = kMoeBf16), e4m3 bytes with
// its N row scales `wscale` (fp32, kMoeFp8) or its [N / 16, K / 128] block scales `wscale` (fp32,
// kMoeFp8Block), or [N, K / 2] MXFP4 bytes with its [N, K / 32] e8m0 block scales `wscale`
// (bytes, kMoeFp4).
template <int MT, int EPI, int WF>
__device__ __forceinline__ void moe_tile(char* smem, const bf16* __restrict__ x,
                                         const char* __restrict__ W,
                                         const void* __restrict__ wscale, bf16* __restrict__ out,
                                         const int* __restrict__ pairs, int start, int rows,
                                         int nb, int topk, int P, int N, int K) {
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  const int n0 = nb * kWsRowsWg;

  // N % 32 == 0: both A tiles are whole.  Image rows past `rows` repeat the tile's last row.
  f32x4 acc[2][MT];
  if (!ws_accumulate<MT, WF, kUnrollOf<WF>>(
          smem, x, W, static_cast<const uint8_t*>(wscale), n0, K, [](int n) { return n; },
          [&](int row) {
            const int tr = min(row, rows - 1);
            if constexpr (EPI == kMoeGateUp)
              return (size_t)(clamp_pair(pairs[tr], P) / topk);   // token
            else
              return (size_t)(start + tr);   // h row
          },
          acc))
    return;

  // ---- epilogue: acc[a][b][e] = y[m = 16 b + r][n = n0 + 16 a + 4 g + e] ----
  if constexpr (WF == kMoeFp8) {   // the scales of the lane's four weight rows per A tile
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const f32x4 ws = *reinterpret_cast<const f32x4*>(static_cast<const float*>(wscale) + n0 +
                                                       16 * a + 4 * g);
#pragma unroll
      for (int b = 0; b < MT; ++b)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[a][b][e] *= ws[e];
    }
  }
  if constexpr (EPI == kMoeGateUp) {
    const int I = N >> 1;
    const int col = 16 * nb + 4 * g;
#pragma unroll
    for (int b = 0; b < MT; ++b) {
      const int m = 16 * b + r;
      if (m >= rows) continue;
      bf16x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float gt = (float)(bf16)acc[0][b][e];
        const float up = (float)(bf16)acc[1][b][e];
        o[e] = (bf16)(silu(gt) * up);
      }
      *reinterpret_cast<bf16x4*>(out + (size_t)(start + m) * I + col) = o;
    }
  } else {
#pragma unroll
    for (int b = 0; b < MT; ++b) {
      const int m = 16 * b + r;
      if (m >= rows) continue;
      const size_t dst = (size_t)clamp_pair(pairs[m], P);
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (bf16)acc[a][b][e];
        *reinterpret_cast<bf16x4*>(out + dst * N + n0 + 16 * a + 4 * g) = o;
      }
    }
  }
}

template <int EPI, int WF>
__global__ void __launch_bounds__(kWsThreads)
moe_grouped_gemm_kernel(const bf16* __restrict__ x, const void* __restrict__ W,
                        const void* __restrict__ wscale, bf16* __restrict__ out,
                        const int* __restrict__ sorted_pairs,
                        const int* __restrict__ tile_expert, const int* __restrict__ tile_start,
                        const int* __restrict__ tile_rows, const int* __restrict__ n_tiles,
                        int E, int topk, int P, int N, int K) {
  __shared__ __attribute__((aligned(1024))) char smem[kWsSmem<kTileRows / 16>];
  const int tile = blockIdx.y, nb = blockIdx.x;
  if (tile >= n_tiles[0]) return;   // before any DMA or barrier
  const int e = min(max(tile_expert[tile], 0), E - 1);
  const int rows = min(max(tile_rows[tile], 1), min(kTileRows, P));
  const int start = min(max(tile_start[tile], 0), P - rows);
  // expert e's weights and scales: N rows of 2 K (bf16), K (fp8) or K / 2 (fp4) bytes; N fp32
  // row scales (fp8), N / 16 x K / 128 fp32 block scales (block-scaled fp8) or N K / 32
  // block-scale bytes (fp4)
  const size_t wrow =
      WF == kMoeFp4 ? (size_t)(K >> 1) : (size_t)K * (WF == kMoeBf16 ? 2 : 1);
  const char* We = static_cast<const char*>(W) + (size_t)e * N * wrow;
  const void* se = nullptr;
  if constexpr (WF == kMoeFp8) se = static_cast<const float*>(wscale) + (size_t)e * N;
  if constexpr (WF == kMoeFp8Block)
    se = static_cast<const float*>(wscale) + (size_t)e * (N >> 4) * (size_t)(K >> 7);
  if constexpr (WF == kMoeFp4)
    se = static_cast<const uint8_t*>(wscale) + (size_t)e * N * (size_t)(K >> 5);
  const int* pairs = sorted_pairs + start;
  if (rows <= 16)
    moe_tile<1, EPI, WF>(smem, x, We, se, out, pairs, start, rows, nb, topk, P, N, K);
  else
    moe_tile<2, EPI, WF>(smem, x, We, se, out, pairs, start, rows, nb, topk, P, N, K);
}

template <int WF>
int launch_grouped(bf16* out, const bf16* x, const void* W, const void* wscale,
                   const int* sorted_pairs, const int* tile_expert, const int* tile_start,
                   const int* tile_rows, const int* n_tiles, int cap, int T, int E, int k, int N,
                   int K, int epilogue, hipStream_t stream) {
  if (T <= 0 || E <= 0 || E > kMaxExperts || k <= 0 || k > kMaxTopK) return -1;
  if (N <= 0 || N % 32 != 0 || K <= 0 || K % 128 != 0) return -2;
  if (cap <= 0 || cap > 65535 || (long)T * k > (1L << 30)) return -3;
  if (out == nullptr || x == nullptr || W == nullptr) return -5;
  if (WF != kMoeBf16 && wscale == nullptr) return -5;
  const dim3 grid(N / kWsRowsWg, cap);
  const int P = T * k;
  if (epilogue == kMoeGateUp)
    moe_grouped_gemm_kernel<kMoeGateUp, WF><<<grid, kWsThreads, 0, stream>>>(
        x, W, wscale, out, sorted_pairs, tile_expert, tile_start, tile_rows, n_tiles, E, k, P, N,
        K);
  else if (epilogue == kMoeDown)
    moe_grouped_gemm_kernel<kMoeDown, WF><<<grid, kWsThreads, 0, stream>>>(
        x, W, wscale, out, sorted_pairs, tile_expert, tile_start, tile_rows, n_tiles, E, k, P, N,
        K);
  else
    return -4;
  return 0;
}

}  // namespace
}  // namespace dli
