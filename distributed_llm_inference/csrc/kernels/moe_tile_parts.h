// What the two grouped tile-GEMM families of the sparse-MoE MLP have in common -- moe_tile_core.h
// (bf16 MFMAs, quantised weights widened in registers) and moe_tile_scaled.hip (the block-scaled
// MFMA on fp8 activations): the tile geometry, the prologue that finds a workgroup's tile, the two
// epilogues over the finished accumulators and the launchers' argument checks.  moe_tile.hip
// describes the design.
#pragma once
#include "kernels.h"

namespace dli {
namespace {

constexpr int kMaxExperts = 256;
constexpr int kMaxTopK = 8;
constexpr int kTM = 128;          // activation rows per tile
constexpr int kTN = 128;          // weight rows per workgroup
constexpr int kThreads = 256;

enum MoeEp { kMoeGateUp = 0, kMoeDown = 1 };

// Which expert, which rows: the wave's prefix sum over ceil(count / 128), lane l holding experts
// 4 l .. 4 l + 3.  False for a tile index past the sum, the same in every wave: the caller returns
// before any DMA, LDS write or barrier.  Every value is clamped before it forms an address: counts
// into [0, P], the expert into [0, E), rows into [1, 128], start + rows <= P
__device__ __forceinline__ bool moe_tile_locate(const int* __restrict__ expert_count,
                                                const int* __restrict__ expert_offset, int E,
                                                int P, int tile, int lane, int& e, int& rows,
                                                int& start) {
  int cnt[4], nt[4], mine_tiles = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = 4 * lane + q;
    cnt[q] = j < E ? min(max(expert_count[j], 0), P) : 0;
    nt[q] = (cnt[q] + kTM - 1) / kTM;
    mine_tiles += nt[q];
  }
  int incl = mine_tiles;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  if (tile >= __shfl(incl, 63, 64)) return false;
  int rem = tile - (incl - mine_tiles), e_l = 4 * lane, c_l = cnt[0];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    if (e_l == 4 * lane + q && rem >= nt[q]) {
      rem -= nt[q];
      e_l = 4 * lane + q + 1;
      c_l = cnt[q + 1];
    }
  }
  const unsigned long long own = __ballot(incl - mine_tiles <= tile && tile < incl);
  const int owner = own ? __builtin_ctzll(own) : 0;   // exactly one lane (tile < the sum)
  e = min(max(__builtin_amdgcn_readlane(e_l, owner), 0), E - 1);
  const int ti = max(__builtin_amdgcn_readlane(rem, owner), 0);
  const int ce = __builtin_amdgcn_readlane(c_l, owner);
  rows = min(max(ce - kTM * ti, 1), min(kTM, P));
  start = min(max(expert_offset[e] + kTM * ti, 0), P - rows);
  return true;
}

// acc[a][b][i] = y[m = 64 wc + 16 b + fr][n = n0 + 64 wr + 16 a + 4 g + i] of the tile whose rows
// are sorted pairs start .. start + rows - 1 (pairs = sorted_pairs + start), finished in fp32.
// Gate|up: gate and up of an output column are A fragments 2 p and 2 p + 1, each rounded to bf16,
// silu(gate) * up in fp32, rounded, to h[start + m, N / 2].  Down: one rounding, to row pairs[m]
// (clamped below P) of y[P, N].  Image rows m >= rows are not stored
template <int EPI>
__device__ __forceinline__ void moe_tile_epilogue(const f32x4 (&acc)[4][4], bf16* __restrict__ out,
                                                  const int* __restrict__ pairs, int rows,
                                                  int start, int P, int N, int n0, int wr, int wc,
                                                  int fr, int g) {
  if constexpr (EPI == kMoeGateUp) {
    const int I = N >> 1;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int m = 64 * wc + 16 * b + fr;
      if (m >= rows) continue;
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        bf16x4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float gt = (float)(bf16)acc[2 * p][b][i];
          const float up = (float)(bf16)acc[2 * p + 1][b][i];
          o[i] = (bf16)(silu(gt) * up);
        }
        // weight rows 32 q .. 32 q + 31 are gate | up of output columns 16 q .. 16 q + 15
        const int col = ((n0 + 64 * wr + 32 * p) >> 1) + 4 * g;
        *reinterpret_cast<bf16x4*>(out + (size_t)(start + m) * I + col) = o;
      }
    }
  } else {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int m = 64 * wc + 16 * b + fr;
      if (m >= rows) continue;
      const size_t dst = (size_t)min(max(pairs[m], 0), P - 1);
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        bf16x4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (bf16)acc[a][b][i];
        *reinterpret_cast<bf16x4*>(out + dst * N + n0 + 64 * wr + 16 * a + 4 * g) = o;
      }
    }
  }
}

// The launchers' checks, with kernels.h's codes: -1 (T, E, k), -2 (N % 128, K a multiple of
// `k_mult` and at most `k_max`), -3 (more pairs or tiles than one launch takes), -4 (epilogue),
// -5 (a null pointer: `pointers` is false)
inline int moe_tile_check_args(int T, int E, int k, int N, int K, int k_mult, int k_max,
                               int epilogue, bool pointers) {
  if (T <= 0 || E <= 0 || E > kMaxExperts || k <= 0 || k > kMaxTopK) return -1;
  if (N <= 0 || N % kTN != 0 || K <= 0 || K % k_mult != 0 || K > k_max) return -2;
  if ((long)T * k > (1L << 30)) return -3;
  const int cap = moe_tile_gemm_capacity(T, E, k);
  if (cap <= 0 || cap > 65535) return -3;
  if (epilogue != kMoeGateUp && epilogue != kMoeDown) return -4;
  return pointers ? 0 : -5;
}

}  // namespace
}  // namespace dli
