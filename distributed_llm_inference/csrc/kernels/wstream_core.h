// The weight-streaming MFMA core shared by the small-M GEMMs (gemm_fp4_small.hip,
// gemm_fp8_small.hip: 3-32 bf16 activation rows) and the grouped sparse-MoE GEMM (moe.hip: tiles of
// 1-32 rows): acc = x[rows, K] . W[32 weight rows, K]^T in fp32 for bf16, fp8 (e4m3fn) or MXFP4
// weights.  All activation rows fit the 16 columns of one (MT = 1) or two (MT = 2) MFMA B tiles,
// so the product is a pure weight stream -- every weight byte is read once -- and the activations
// stay bf16: the weight is widened to bf16 in registers (exact, below) and multiplied on
// v_mfma_f32_16x16x32_bf16.  The callers own the kernel signature, the LDS buffer, which rows are
// loaded (ws_accumulate's two functors) and everything after the K-split sum: row scales, bias,
// SwiGLU, scatter.
//
//   * operands.  The weight is the MFMA's A operand (lane l = (r = l & 15, g = l >> 4) holds
//     A[row r][k = 8 g + j], j = 0..7), the activations its B operand (B[k = 8 g + j][col r]).
//     The k order inside a step is free as long as A and B agree, so a 128-k step t is four
//     MFMAs whose "k = 8 g + j" is really k = 128 t + 32 g + 8 i + j for MFMA i = 0..3:
//       - lane (r, g) loads W[n0 + 16 a + r][128 t + 32 g .. + 31] of A tile a, non-temporal:
//           kWsBf16: 64 bytes, four 16-byte loads; load i is the lane's A fragment of MFMA i;
//           kWsFp8:  32 bytes, two 16-byte loads; dwords 2 i and 2 i + 1 of the 8, widened
//             e4m3 -> bf16 (v_cvt_scalef32_pk_bf16_fp8, scale 1.0, 4 converts; exact, every e4m3
//             value is a bf16 value), are the A fragment of MFMA i.  No scale in the loop: a
//             per-row scale is the caller's, on the fp32 accumulator;
//           kWsFp4:  16 bytes, one load (a row is K / 2 bytes, element 2 j in the low nibble of
//             byte j): exactly one scale block, so one scale byte bscale[n0 + 16 a + r][4 t + g];
//             dword i of the load, widened e2m1 -> bf16 with the block's 2^(byte - 127)
//             (v_cvt_scalef32_pk_bf16_fp4, 4 converts, exact), is the A fragment of MFMA i.  The
//             scale is spent in the widening: nothing is left for the epilogue;
//       - the B fragment of MFMA i at lane (c, g) is the 16 bytes x[c][128 t + 32 g + 8 i .. + 7]:
//         64 consecutive bytes of x per lane and step.
//     4 MFMAs per A tile, B tile and step; 16 converts per 32 fp8 / fp4 weights; no lane
//     movement.  The k order, the wave's steps and the order of the MFMAs are the same for the
//     three formats, so fp8 / fp4 give the bf16 result on the widened weights bit for bit.
//   * x through LDS.  Read straight from global, those fragments are four 16-byte loads at a
//     64-byte lane stride over 16 rows -- 32 cache lines per instruction, each fetched four
//     times -- and the kernel was bound by them, not by the weights (fp4, M = 32: 0.9-1.4 TB/s of
//     weights).  So each wave stages the x of its own k-step (16 MT rows x 256 B) in a private
//     LDS buffer by LDS-DMA, whole 256-byte row pieces per 16 lanes, one step ahead of the MFMAs
//     (two buffers per wave, no workgroup barrier), and reads the fragments back with
//     ds_read_b128.  The image is lane-linear (DMA), so the bank swizzle sits on the source
//     address: slot p of row c holds chunk p ^ swz(c), swz(c) = c ^ ((c & 4) << 1).  A
//     ds_read_b128 lane group holds all 16 rows c and two neighbouring g (chunks 4 g + i):
//     plain c would collide for rows 4 apart across the two g; swz keeps the 16 slots distinct.
//     The source row of an image row is the caller's (xrow): clamped, gathered or offset, the
//     LDS-DMA source address is per lane already.
//   * rows.  A workgroup owns kWsRowsWg = 32 consecutive weight rows = two A tiles, so every x
//     fragment feeds two MFMAs (x traffic is what bounded the GEMV).  MT = 1 / 2 B tiles cover
//     <= 16 / 32 activation rows; image rows past the caller's count repeat a row the caller
//     names and are never stored.
//   * parallelism.  The kWsWaves waves of the workgroup split K: wave w takes the steps t = w,
//     w + kWsWaves, ... (at any moment the workgroup reads kWsWaves x 256 / 128 / 64 consecutive
//     bytes of each of its bf16 / fp8 / fp4 rows), with kUnroll steps of weight loads in flight
//     per lane: 4 / 2 / 1 16-byte loads (fp4: and one scale byte) per A tile and step.  kUnroll
//     is each caller's, by its own measurements.  The partial accumulators meet in LDS and wave 0
//     adds them in wave order: deterministic, no atomics, no cross-workgroup hand-off.
//   * the pipeline.  A wave's steps are t = wave + i kWsWaves, i < nsteps.  On entering a group
//     of kUnroll steps the x of its first step is the only memory operation in flight; the
//     group's weight loads follow it, and every step first sends the next step's x into the other
//     buffer, then waits for all but those 4 MT newest operations (vmcnt counts in issue order).
//     kWsFp4: the scale bytes are vector memory loads too, issued with the weight loads, i.e.
//     before the next x -- so "all but the 4 MT newest" still covers them.
//   * result.  C/D: lane (c, g) holds D[n = 4 g + e][m = c], e = 0..3 -- four consecutive output
//     columns of activation row c: acc[a][b][e] = y[m = 16 b + r][n = n0 + 16 a + 4 g + e].
#pragma once
#include "kernels.h"

namespace dli {
namespace {

constexpr int kWsWaves = 8;              // K-split ways = waves per workgroup
constexpr int kWsThreads = kWsWaves * 64;
constexpr int kWsRowsWg = 32;            // weight rows per workgroup: two 16-row A tiles

enum WsFormat { kWsBf16 = 0, kWsFp8 = 1, kWsFp4 = 2 };

typedef unsigned u32x4w __attribute__((ext_vector_type(4)));   // nontemporal-loadable 16 B

template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// the 16-byte slot of chunk ch of x row c in the staged image is ch ^ swz(c)
__device__ __forceinline__ int swz(int c) { return c ^ ((c & 4) << 1); }

// LDS bytes of a workgroup: two x buffers (one k-step of x: 16 MT rows x 128 bf16) per wave
template <int MT> constexpr int kWsSmem = kWsWaves * 2 * (MT * 16 * 256);

// The K-split product of one workgroup: activation image rows 0 .. 16 MT - 1 (image row i is row
// xrow(i) of x [*, K]) times the weight rows wrow(n0) .. wrow(n0 + 31) of W (rows of 2 K (kWsBf16),
// K (kWsFp8) or K / 2 (kWsFp4) bytes; bscale: the [*, K / 32] e8m0 block scales, kWsFp4 only).
// K % 128 == 0; smem holds kWsSmem<MT> bytes, 1024-aligned.  Every wave of the workgroup must
// call it (it holds a barrier); it returns true in wave 0, with the sum over K in `sum`, and false
// in the others, which are done.
template <int MT, int WF, int kUnroll, class WRow, class XRow>
__device__ __forceinline__ bool ws_accumulate(char* smem, const bf16* __restrict__ x,
                                              const char* __restrict__ W,
                                              const uint8_t* __restrict__ bscale, int n0, int K,
                                              WRow wrow, XRow xrow, f32x4 (&sum)[2][MT]) {
  static_assert(kUnroll % 2 == 0, "a group starts on x buffer 0");
  // the accumulators are a local array, handed over at the end: accumulating through the
  // caller's reference made the compiler schedule the k-loop differently from the kernels that
  // carried this loop themselves (fp4 gate|up 0.5-1 % slower: docs/kernels.md)
  f32x4 acc[2][MT];
  constexpr int kWB = WF == kWsBf16 ? 2 : 1;   // bytes per weight (kWsFp4: half a byte, below)
  constexpr int kWL = WF == kWsFp4 ? 1 : 2 * kWB;   // 16-byte loads per A tile and k-step
  constexpr int kStepB = 16 * 4 * kWL;         // bytes of a weight row per k-step: 4 lanes' loads
  constexpr int kXBuf = MT * 16 * 256;   // one k-step of x: 16 MT rows x 128 bf16
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int kt = K >> 7;
  char* xw = smem + wave * (2 * kXBuf);   // this wave's two x buffers; nobody else touches them

  // this lane's weight rows (A tiles 0 / 1) at its 32-k block of step 0
  // (kWsFp4: a row is K / 2 bytes, and the lane's scale byte of step 0 is block g of its row)
  const char* wp[2];
  const uint8_t* sp[2];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const size_t n = (size_t)wrow(n0 + 16 * a + r);
    if constexpr (WF == kWsFp4) {
      wp[a] = W + n * (size_t)(K >> 1) + 16 * g;
      sp[a] = bscale + n * (size_t)(K >> 5) + g;
    } else {
      wp[a] = W + (n * K + 32 * g) * kWB;
      sp[a] = nullptr;
    }
  }
  // x staging: DMA instruction q fills image rows 4 q .. 4 q + 3 (lane l: row 4 q + (l >> 4),
  // slot l & 15) with whole 256-byte row pieces; the slot permutation is on the source address.
  const bf16* xsrc[4 * MT];
#pragma unroll
  for (int q = 0; q < 4 * MT; ++q) {
    const int row = 4 * q + g;
    const size_t src = (size_t)xrow(row);
    xsrc[q] = x + src * K + ((r ^ swz(row & 15)) << 3);
  }
  // ... and the fragment reads: B fragment i of lane (c = r, g) is chunk 4 g + i of row 16 b + c
  int xoff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) xoff[i] = r * 256 + (((4 * g + i) ^ swz(r)) << 4);

#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < MT; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  // k-step t < kt: every address below stays inside its row (K % 128 == 0)
  // kWsFp4: the scale bytes are vector memory loads too, issued here with the weight loads,
  // i.e. before the next stage_x -- so "all but the 4 MT newest" below still covers them
  auto load_w = [&](int t, u32x4w (&wv)[2][kWL], unsigned (&sc)[2]) {
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
      for (int i = 0; i < kWL; ++i)
        wv[a][i] = __builtin_nontemporal_load(
            reinterpret_cast<const u32x4w*>(wp[a] + (size_t)t * kStepB + 16 * i));
      if constexpr (WF == kWsFp4) sc[a] = sp[a][(size_t)t * 4];
    }
  };
  auto stage_x = [&](int t, int buf) {
#pragma unroll
    for (int q = 0; q < 4 * MT; ++q)
      glds16(xsrc[q] + (size_t)t * 128, xw + buf * kXBuf + q * 1024);
  };
  auto step = [&](int buf, const u32x4w (&wv)[2][kWL], const unsigned (&sc)[2]) {
    bf16x8 xb[MT][4];
#pragma unroll
    for (int b = 0; b < MT; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        xb[b][i] = *reinterpret_cast<const bf16x8*>(xw + buf * kXBuf + b * 4096 + xoff[i]);
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      float s = 0.f;   // kWsFp4: 2^(byte - 127), byte in [1, 254]
      if constexpr (WF == kWsFp4) s = __uint_as_float(sc[a] << 23);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        bf16x8 wf;
        if constexpr (WF == kWsFp4)   // dword i of the lane's 4: exact widening
          wf = fp4x8_to_bf16x8(wv[a][0][i], s);
        else if constexpr (WF == kWsFp8)   // dwords 2 i, 2 i + 1 of the lane's 8: exact widening
          wf = fp8x8_to_bf16x8(uint2{wv[a][i >> 1][2 * (i & 1)], wv[a][i >> 1][2 * (i & 1) + 1]});
        else
          wf = __builtin_bit_cast(bf16x8, wv[a][i]);
#pragma unroll
        for (int b = 0; b < MT; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xb[b][i], acc[a][b], 0, 0, 0);
      }
    }
  };

  // This wave's steps are t = wave + i kWsWaves, i < nsteps.  On entering a group of kUnroll steps
  // the x of its first step is the only memory operation in flight; the group's weight loads
  // follow it, and every step first sends the next step's x into the other buffer, then waits
  // for all but those 4 MT newest operations (vmcnt counts in issue order).
  const int nsteps = wave < kt ? (kt - wave + kWsWaves - 1) / kWsWaves : 0;
  if (nsteps > 0) stage_x(wave, 0);
  int i = 0;
  for (; i + kUnroll <= nsteps; i += kUnroll) {   // whole groups; kUnroll is even: buffer u & 1
    u32x4w wv[kUnroll][2][kWL];
    unsigned sc[kUnroll][2];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) load_w(wave + (i + u) * kWsWaves, wv[u], sc[u]);
    asm volatile("" ::: "memory");
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      if (u + 1 < kUnroll || i + kUnroll < nsteps) {
        stage_x(wave + (i + u + 1) * kWsWaves, (u + 1) & 1);
        wait_vm<4 * MT>();
      } else {
        wait_vm<0>();
      }
      step(u & 1, wv[u], sc[u]);
      asm volatile("" ::: "memory");   // the next DMA into this buffer stays behind its reads
    }
  }
  for (; i < nsteps; ++i) {   // fewer than kUnroll steps left
    u32x4w wv[2][kWL];
    unsigned sc[2];
    load_w(wave + i * kWsWaves, wv, sc);
    asm volatile("" ::: "memory");
    if (i + 1 < nsteps) {
      stage_x(wave + (i + 1) * kWsWaves, (i + 1) & 1);
      wait_vm<4 * MT>();
    } else {
      wait_vm<0>();
    }
    step(i & 1, wv, sc);
    asm volatile("" ::: "memory");
  }

  // ---- K-split sum: waves 1.. park their partials, wave 0 adds them in wave order ----
  // (into its own x buffers: every DMA into them has landed and been read)
  if (wave > 0) {
    float* red = reinterpret_cast<float*>(xw);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < MT; ++b)
#pragma unroll
        for (int e = 0; e < 4; ++e) red[((a * MT + b) * 4 + e) * 64 + lane] = acc[a][b][e];
  }
  __syncthreads();
  if (wave > 0) return false;
#pragma unroll
  for (int w = 1; w < kWsWaves; ++w) {
    const float* red = reinterpret_cast<const float*>(smem + w * (2 * kXBuf));
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < MT; ++b)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[a][b][e] += red[((a * MT + b) * 4 + e) * 64 + lane];
  }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < MT; ++b) sum[a][b] = acc[a][b];
  return true;
}

}  // namespace
}  // namespace dli
