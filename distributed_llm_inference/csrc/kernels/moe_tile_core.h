// The grouped MFMA tile GEMM of the sparse-MoE MLP (described in moe_tile.hip): the kernel
// template and its launcher, shared by moe_tile.hip (bf16, per-row fp8 and MXFP4 experts) and
// moe_tile_fp8_block.hip (block-scaled fp8 experts, whose in-loop rescale is fp32 vector
// arithmetic and is compiled without packed fp32 instructions: a translation unit of its own, so
// that the other three formats keep the code they have).  The tile geometry, the prologue that
// finds the tile, the epilogues and the launcher's checks are moe_tile_parts.h's.
#pragma once
#include <climits>

#include "moe_tile_parts.h"

namespace dli {

// launch_moe_tile_gemm for W.format == kExpertFp8Block (moe_tile_fp8_block.hip); `wscale` is the
// [E, N / 16, K / 128] fp32 table
int launch_moe_tile_fp8_block(bf16* out, const bf16* x, const void* W, const void* wscale,
                              const int* sorted_pairs, const int* expert_count,
                              const int* expert_offset, int T, int E, int k, int N, int K,
                              int epilogue, hipStream_t stream);

namespace {

constexpr int kBK = 64;           // k per step
constexpr int kOp = 128 * 128;    // bytes of one staged operand tile

enum TileWf { kTileBf16 = 0, kTileFp8 = 1, kTileFp4 = 2, kTileFp8Block = 3 };

// fp8 bytes in LDS, whichever scales go with them
template <int WF> constexpr bool kTileF8Bytes = WF == kTileFp8 || WF == kTileFp8Block;
// bytes of one staged weight tile (128 rows of one k-step) and of one buffer (weight | activation)
template <int WF>
constexpr int kWOp = WF == kTileBf16 ? kOp : kTileF8Bytes<WF> ? kOp / 2 : kOp / 4;
template <int WF> constexpr int kBufOf = kWOp<WF> + kOp;

// W: the experts' [E, N, K] bf16, [E, N, K] e4m3 bytes (wscale: [E, N] fp32 row scales, or
// [E, N / 16, K / 128] fp32 block scales for kTileFp8Block) or [E, N, K / 2] MXFP4 bytes (wscale:
// [E, N, K / 32] e8m0 block scales)
template <int EPI, int WF>
__global__ void __launch_bounds__(kThreads, 2)
moe_tile_gemm_kernel(const bf16* __restrict__ x, const void* __restrict__ Wv,
                     bf16* __restrict__ out, const int* __restrict__ sorted_pairs,
                     const int* __restrict__ expert_count, const int* __restrict__ expert_offset,
                     int E, int topk, int P, int N, int K, const void* __restrict__ wscale) {
  constexpr int kBuf = kBufOf<WF>;
  __shared__ __attribute__((aligned(1024))) char smem[2 * kBuf];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nb = blockIdx.x;

  int e, rows, start;
  if (!moe_tile_locate(expert_count, expert_offset, E, P, blockIdx.y, lane, e, rows, start)) return;
  const int* pairs = sorted_pairs + start;
  const bf16* We = static_cast<const bf16*>(Wv) + (size_t)e * N * K;   // the bf16 experts only
  const int n0 = nb * kTN;
  const int kt = K / kBK;

  // ---- staging: DMA round j fills image rows 32 j .. 32 j + 31 of an operand tile (thread: row
  // 32 j + (tid >> 3), slot tid & 7); the chunk that belongs in that slot is the same every round
  const int srow = tid >> 3;
  const int chunk = (tid & 7) ^ ((srow >> 1) & 7);
  // the weight tile: bf16 as above; fp8 two rounds of 64 rows of 64 B (thread: row 64 j +
  // (tid >> 2), slot tid & 3); MXFP4 one round of 128 rows of 32 B (row tid >> 1, slot tid & 1)
  const bf16* wsrc = nullptr;
  const char* qsrc = nullptr;
  if constexpr (WF == kTileBf16) {
    wsrc = We + (size_t)(n0 + srow) * K + chunk * 8;
  } else if constexpr (kTileF8Bytes<WF>) {
    const int qrow = tid >> 2;
    qsrc = static_cast<const char*>(Wv) + ((size_t)e * N + n0 + qrow) * K +
           (((tid & 3) ^ ((qrow >> 2) & 3) ^ ((qrow >> 4) & 3)) << 4);
  } else {
    const int qrow = tid >> 1;
    qsrc = static_cast<const char*>(Wv) + ((size_t)e * N + n0 + qrow) * (size_t)(K >> 1) +
           (((tid & 1) ^ ((qrow >> 2) & 1)) << 4);
  }
  const bf16* xsrc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int tr = min(32 * j + srow, rows - 1);
    size_t src;
    if constexpr (EPI == kMoeGateUp) src = (size_t)(min(max(pairs[tr], 0), P - 1) / topk);   // token
    else src = (size_t)(start + tr);                                                        // h row
    xsrc[j] = x + src * K + chunk * 8;
  }
  auto stage = [&](int t, int buf) {
    char* dst = smem + buf * kBuf + wave * 1024;
    if constexpr (WF == kTileBf16) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        glds16(wsrc + (size_t)j * 32 * K + (size_t)t * kBK, dst + j * 4096);
    } else if constexpr (kTileF8Bytes<WF>) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
        glds16(qsrc + (size_t)j * 64 * K + (size_t)t * kBK, dst + j * 4096);
    } else {
      glds16(qsrc + (size_t)t * (kBK / 2), dst);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) glds16(xsrc[j] + (size_t)t * kBK, dst + kWOp<WF> + j * 4096);
  };

  // ---- fragments: lane (fr, g) reads chunk 4 kk + g of row 16 f + fr of its wave's 64 rows ----
  const int wr = wave >> 1, wc = wave & 1, fr = lane & 15, g = lane >> 4;
  int foff[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) foff[kk] = fr * 128 + (((4 * kk + g) ^ ((fr >> 1) & 7)) << 4);
  // quantised weight rows: bytes 32 kk + 8 g .. + 7 of a 64-byte row (fp8), dword 4 kk + g of a
  // 32-byte row (MXFP4), behind the slot swizzles of the staging
  int qoff[4][2] = {};
#pragma unroll
  for (int f = 0; f < 4; ++f)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      if constexpr (kTileF8Bytes<WF>)
        qoff[f][kk] = f * 1024 + fr * 64 + (((2 * kk + (g >> 1)) ^ ((fr >> 2) & 3) ^ f) << 4) +
                      ((g & 1) << 3);
      if constexpr (WF == kTileFp4)
        qoff[f][kk] = f * 512 + fr * 32 + ((kk ^ ((fr >> 2) & 1)) << 4) + (g << 2);
    }
  const int aoff = wr * 64 * (kWOp<WF> / 128), boff = kWOp<WF> + wc * 64 * 128;

  // MXFP4: the e8m0 bytes of a pair of k-steps of the lane's four fragment rows, a pair ahead
  const uint8_t* ssrc = nullptr;
  int srstride = 0;
  unsigned sc[4] = {0u, 0u, 0u, 0u}, scn[4] = {0u, 0u, 0u, 0u};
  if constexpr (WF == kTileFp4) {
    srstride = 16 * (K >> 5);
    ssrc = static_cast<const uint8_t*>(wscale) +
           ((size_t)e * N + n0 + 64 * wr + fr) * (size_t)(K >> 5);
  }
  auto load_scales = [&](int u) {   // the four bytes of k-steps 2 u and 2 u + 1 (K % 128 == 0)
#pragma unroll
    for (int f = 0; f < 4; ++f)
      scn[f] = *reinterpret_cast<const unsigned*>(ssrc + (size_t)f * srstride + 4 * u);
  };
  // block-scaled fp8: the wave's four A fragments are four 16-row scale groups, (n0 + 64 wr) / 16
  // + a, a = 0 .. 3; a group's fp32 scales of the K / 128 blocks are consecutive.  A scale block
  // is a pair of k-steps (2 u, 2 u + 1; K % 128 == 0): the pair's products meet in `blk`, and the
  // odd step adds scale * blk to the running sum.  The four scales of a pair are wave-uniform
  // loads issued at its even step
  const float* bsrc = nullptr;
  int bstride = 0;
  float bs[4] = {0.f, 0.f, 0.f, 0.f};
  if constexpr (WF == kTileFp8Block) {
    bstride = K >> 7;
    bsrc = static_cast<const float*>(wscale) +
           ((size_t)e * (N >> 4) + ((n0 + 64 * wr) >> 4)) * (size_t)bstride;
  }

  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  // kTileFp8Block: the sum over the current 128-k block, before its scale
  f32x4 blk[kTileFp8Block == WF ? 4 : 1][4];
  if constexpr (WF == kTileFp8Block) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) blk[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  stage(0, 0);
  if constexpr (WF == kTileFp4) load_scales(0);
  for (int t = 0; t < kt; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();   // k-step t has landed for every wave; nobody still reads the other buffer
    if constexpr (WF == kTileFp4) {
      if (!(t & 1)) {
#pragma unroll
        for (int f = 0; f < 4; ++f) sc[f] = scn[f];
      }
    }
    if (t + 1 < kt) {
      stage(t + 1, (t + 1) & 1);
      if constexpr (WF == kTileFp4) {   // an even k-step fetches the next pair's scales
        if (!(t & 1) && t + 2 < kt) load_scales((t >> 1) + 1);
      }
    }
    if constexpr (WF == kTileFp8Block) {
      if (!(t & 1)) {
#pragma unroll
        for (int a = 0; a < 4; ++a) bs[a] = bsrc[(size_t)a * bstride + (t >> 1)];
      }
    }
    asm volatile("" ::: "memory");
    const char* buf = smem + (t & 1) * kBuf;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        if constexpr (WF == kTileBf16) {
          af[f] = *reinterpret_cast<const bf16x8*>(buf + aoff + f * 2048 + foff[kk]);
        } else if constexpr (kTileF8Bytes<WF>) {
          // a clang vector, not HIP's uint2: read through that struct the ds_read_b64 may alias
          // anything for the compiler, which then waits vmcnt(0) for the DMA it has just sent
          typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
          const u32x2 v = *reinterpret_cast<const u32x2*>(buf + aoff + qoff[f][kk]);
          af[f] = fp8x8_to_bf16x8(uint2{v[0], v[1]});
        } else {
          const float s =   // 2^(byte - 127), byte 2 (t & 1) + kk of the pair's four
              __uint_as_float(((sc[f] >> (16 * (t & 1) + 8 * kk)) & 0xffu) << 23);
          af[f] = fp4x8_to_bf16x8(
              *reinterpret_cast<const unsigned*>(buf + aoff + qoff[f][kk]), s);
        }
        bfr[f] = *reinterpret_cast<const bf16x8*>(buf + boff + f * 2048 + foff[kk]);
      }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          if constexpr (WF == kTileFp8Block)
            blk[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[a], bfr[b], blk[a][b], 0, 0, 0);
          else
            acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[a], bfr[b], acc[a][b], 0, 0, 0);
        }
    }
    if constexpr (WF == kTileFp8Block) {
      if (t & 1) {   // the 128-k block is complete: its scale, then a fresh block sum
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) {
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[a][b][i] += bs[a] * blk[a][b][i];
            blk[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
          }
      }
    }
    asm volatile("" ::: "memory");   // the next DMA into this buffer stays behind its reads
  }

  // fp8: the scales of the lane's four weight rows per A fragment, n0 + 64 wr + 16 a + 4 g + i < N
  if constexpr (WF == kTileFp8) {
    const float* se = static_cast<const float*>(wscale) + (size_t)e * N + n0 + 64 * wr + 4 * g;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const f32x4 ws = *reinterpret_cast<const f32x4*>(se + 16 * a);
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[a][b][i] *= ws[i];
    }
  }

  moe_tile_epilogue<EPI>(acc, out, pairs, rows, start, P, N, n0, wr, wc, fr, g);
}

template <int WF>
int launch_tile(bf16* out, const bf16* x, const void* W, const void* wscale,
                const int* sorted_pairs, const int* expert_count, const int* expert_offset, int T,
                int E, int k, int N, int K, int epilogue, hipStream_t stream) {
  const int rc = moe_tile_check_args(
      T, E, k, N, K, WF == kTileFp4 || WF == kTileFp8Block ? 128 : kBK, INT_MAX, epilogue,
      out != nullptr && x != nullptr && W != nullptr && sorted_pairs != nullptr &&
          expert_count != nullptr && expert_offset != nullptr &&
          (WF == kTileBf16 || wscale != nullptr));
  if (rc != 0) return rc;
  const dim3 grid(N / kTN, moe_tile_gemm_capacity(T, E, k));
  const int P = T * k;
  if (epilogue == kMoeGateUp)
    moe_tile_gemm_kernel<kMoeGateUp, WF><<<grid, kThreads, 0, stream>>>(
        x, W, out, sorted_pairs, expert_count, expert_offset, E, k, P, N, K, wscale);
  else
    moe_tile_gemm_kernel<kMoeDown, WF><<<grid, kThreads, 0, stream>>>(
        x, W, out, sorted_pairs, expert_count, expert_offset, E, k, P, N, K, wscale);
  return 0;
}

}  // namespace
}  // namespace dli
