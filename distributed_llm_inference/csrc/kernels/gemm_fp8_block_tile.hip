// Dense LDS-staged MFMA tile GEMM for a block-scaled fp8 (e4m3fn) weight and 33 bf16 rows and more:
//   y[M, N] = x[M, K] . (W8[N, K] (.) scale)^T (+ bias), fp32 accumulation, one bf16 rounding,
// scale [N / 16, K / 128] fp32 (Linear's "fp8_block" state; gemm_fp8_block_small.hip is the 1-32
// row kernel).  Prefill chunks and large decode batches of a 128 x 128 FP8 checkpoint run their
// linears on the stored bytes: a weight byte is read once per 128 activation rows, widened to bf16
// (exact: every e4m3 value is a bf16 value) when a lane reads its MFMA fragment from LDS, and
// never exists dequantised in memory.  The activations are never quantised.
//
//   * work split.  One workgroup per 128 (weight rows) x 128 (activation rows) output tile, a 1-D
//     grid of tiles_n * tiles_m workgroups (tiles_n = N / 128, tiles_m = ceil(M / 128)) in
//     gemm_tile.hip's grouped order: groups of 8 M tiles x all N panels, M fastest inside a group,
//     so the workgroups that run at once share 8 activation panels and a few weight panels
//     through L2, and a weight panel's M tiles stay neighbours.  No expert tables, no gather, no
//     scatter, no split-K and no partials: the kernel writes the finished bf16 tensor and the
//     launcher allocates nothing (graph-safe on the current stream).
//   * 4 waves as 2 (weight rows) x 2 (activation rows), 64 x 64 per wave = 4 x 4 fragments of
//     v_mfma_f32_16x16x32_bf16 with the weight as the A operand: a lane owns 4 consecutive output
//     columns of one row (8-byte stores), and each of a wave's four 16-row A fragments is exactly
//     one scale group -- the scale is uniform over an MFMA operand tile, one fp32 per fragment.
//   * staging.  k-step of 64.  Per step the workgroup stages W8 [128 rows][64 B] (two LDS-DMA
//     rounds; thread: row 64 j + (tid >> 2), 16-byte slot tid & 3) and x [128 rows][128 B] (four
//     rounds; thread: row 32 j + (tid >> 3), slot tid & 7) by 16-byte LDS-DMA (glds16).  The images
//     are lane-linear, so the bank swizzles sit on the per-lane source address:
//       - x: chunk c of row r in slot c ^ ((r >> 1) & 7); a fragment ds_read_b128 (16 rows x one
//         chunk per g) then touches every bank group once (gemm_tile.hip's swizzle);
//       - W8: the fragment is 8 bytes (k = 32 kk + 8 g .. + 7), one ds_read_b64, served in halves
//         of 32 lanes over four 64-byte rows; chunk c of row r in slot c ^ ((r >> 2) & 3) ^
//         ((r >> 4) & 3): rows fr, fr + 4, fr + 8, fr + 12 take the four slots and the two g of a
//         half the two halves of a slot -- every bank once.  (moe_tile.hip's fp8 image: the
//         second term also keeps two fragments' reads from fusing into ds_read2st64_b64.)
//     The activation rows are contiguous: row m0 + r, clamped to M - 1 in a partial M tile (loaded
//     in bounds, multiplied, never stored).
//   * pipeline.  Two LDS buffers; per k-step: wait for step t's DMA, one barrier (which also says
//     everybody is done reading the other buffer), send step t + 1 into the other buffer, multiply
//     step t -- the next step's DMA is in flight under this step's 32 MFMAs per wave.
//   * scale granularity.  A scale block is 128 k = two k-steps (K % 128 == 0, so steps come in
//     pairs and a scale change falls on a step boundary).  The MFMAs of steps 2 u and 2 u + 1 run
//     into a second accumulator set `blk`; the odd step adds scale[group][u] * blk to the running
//     sum on the vector ALU (64 fused multiply-adds per lane and pair, next to 64 MFMAs per wave)
//     and clears it.  The four scales of a pair are wave-uniform loads issued at its even step.
//     The result is the fp32 sum over the blocks of scale * (block sum): the small kernel's and
//     the CPU oracle's arithmetic up to the order inside a block.  This file is compiled without
//     packed fp32 instructions, so the flush stays scalar v_fma_f32.
//     Why not a 128-deep step: it needs 2 x (16 + 32) KB = 96 KB of LDS, one workgroup per CU, and
//     still the zeroed step accumulator; the 64-deep step costs the same registers and keeps two.
//   * LDS.  2 buffers x (8 KB W8 + 16 KB x) = 48 KB per workgroup: three workgroups per CU out of
//     160 KB; the 128 + 128 accumulator registers hold it to two (__launch_bounds__(256, 2)),
//     which overlap one's barrier wait with the other's MFMAs.
//   * epilogues.  acc[a][b][i] = y[m = m0 + 64 wc + 16 b + fr][n = n0 + 64 wr + 16 a + 4 g + i];
//     rows m >= M are not stored.  Plain: (+ bias) in fp32, one rounding, one 8-byte store.
//     SwiGLU (swiglu_interleave'd rows: gate and up of an output column are A fragments 2 p and
//     2 p + 1 of a wave, in the same lane and register): each rounded to bf16, silu(gate) * up in
//     fp32, one rounding -- ops.swiglu_interleaved on the plain output, bit for bit.
//   * measured (profiles/fp8_block/dense.json, docs/kernels.md "Dense block-scaled fp8 weights"):
//     slower than the bf16 path on the dequantised weight at most shapes, 1.2-3.2 x -- few
//     workgroups at 128 rows of a 4096-wide output, and 1.45-1.7 x with a full grid at 4096 rows.
#include "kernels.h"

namespace dli {

namespace {

constexpr int kTM = 128;          // activation rows per tile
constexpr int kTN = 128;          // weight rows per tile
constexpr int kBK = 64;           // k per step
constexpr int kThreads = 256;
constexpr int kWOp = kTN * kBK;           // bytes of a staged weight tile: 8 KB
constexpr int kXOp = kTM * kBK * 2;       // bytes of a staged activation tile: 16 KB
constexpr int kBuf = kWOp + kXOp;
constexpr int kGroupM = 8;        // M tiles per group of the grouped tile order

enum TileEp { kTilePlain = 0, kTileSwiGLU = 1 };

template <int EPI>
__global__ void __launch_bounds__(kThreads, 2)
fp8_block_tile_kernel(const bf16* __restrict__ x, const uint8_t* __restrict__ W,
                      const float* __restrict__ bscale, const bf16* __restrict__ bias,
                      bf16* __restrict__ y, int M, int N, int K, int tiles_m, int tiles_n) {
  __shared__ __attribute__((aligned(1024))) char smem[2 * kBuf];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // ---- grouped tile order: groups of (up to) 8 M tiles x all N panels, M fastest in a group ----
  const int tile = blockIdx.x;
  const int gper = kGroupM * tiles_n, grp = tile / gper, grem = tile % gper;
  const int gm = min(kGroupM, tiles_m - grp * kGroupM);
  const int m0 = (grp * kGroupM + grem % gm) * kTM;
  const int n0 = (grem / gm) * kTN;
  const int kt = K / kBK;   // even: K % 128 == 0

  // ---- staging sources (the slot swizzles are on the source address) ----
  const int qrow = tid >> 2;   // weight: round j fills rows 64 j + qrow, slot tid & 3
  const char* qsrc = reinterpret_cast<const char*>(W) + (size_t)(n0 + qrow) * K +
                     (((tid & 3) ^ ((qrow >> 2) & 3) ^ ((qrow >> 4) & 3)) << 4);
  const int srow = tid >> 3;   // activations: round j fills rows 32 j + srow, slot tid & 7
  const int chunk = (tid & 7) ^ ((srow >> 1) & 7);
  const bf16* xsrc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)   // rows past M repeat row M - 1
    xsrc[j] = x + (size_t)min(m0 + 32 * j + srow, M - 1) * K + chunk * 8;
  auto stage = [&](int t, int buf) {
    char* dst = smem + buf * kBuf + wave * 1024;
#pragma unroll
    for (int j = 0; j < 2; ++j) glds16(qsrc + (size_t)j * 64 * K + (size_t)t * kBK, dst + j * 4096);
#pragma unroll
    for (int j = 0; j < 4; ++j) glds16(xsrc[j] + (size_t)t * kBK, dst + kWOp + j * 4096);
  };

  // ---- fragments: wave (wr, wc) owns weight rows 64 wr .. + 63, activation rows 64 wc .. + 63 ----
  const int wr = wave >> 1, wc = wave & 1, fr = lane & 15, g = lane >> 4;
  int foff[2], qoff[4][2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    // x: chunk 4 kk + g of row 16 f + fr (16 f is a multiple of 16: the swizzle sees fr alone)
    foff[kk] = fr * 128 + (((4 * kk + g) ^ ((fr >> 1) & 7)) << 4);
    // W8: bytes 32 kk + 8 g .. + 7 of row 16 f + fr of the wave's 64 ((row >> 4) & 3 == f)
#pragma unroll
    for (int f = 0; f < 4; ++f)
      qoff[f][kk] = f * 1024 + fr * 64 + (((2 * kk + (g >> 1)) ^ ((fr >> 2) & 3) ^ f) << 4) +
                    ((g & 1) << 3);
  }
  const int aoff = wr * 64 * kBK, boff = kWOp + wc * 64 * 128;

  // the wave's four scale groups (n0 + 64 wr) / 16 + a; a group's K / 128 scales are consecutive
  const int bstride = K >> 7;
  const float* bsrc = bscale + (size_t)((n0 + 64 * wr) >> 4) * bstride;
  float bs[4] = {0.f, 0.f, 0.f, 0.f};

  f32x4 acc[4][4], blk[4][4];   // the running sum; the current 128-k block before its scale
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
      blk[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

  stage(0, 0);
  for (int t = 0; t < kt; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();   // k-step t has landed for every wave; nobody still reads the other buffer
    if (t + 1 < kt) stage(t + 1, (t + 1) & 1);
    if (!(t & 1)) {
#pragma unroll
      for (int a = 0; a < 4; ++a) bs[a] = bsrc[(size_t)a * bstride + (t >> 1)];
    }
    asm volatile("" ::: "memory");
    const char* buf = smem + (t & 1) * kBuf;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        // a clang vector, not HIP's uint2: read through that struct the ds_read_b64 may alias
        // anything for the compiler, which then waits vmcnt(0) for the DMA it has just sent
        typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
        const u32x2 v = *reinterpret_cast<const u32x2*>(buf + aoff + qoff[f][kk]);
        af[f] = fp8x8_to_bf16x8(uint2{v[0], v[1]});
        bfr[f] = *reinterpret_cast<const bf16x8*>(buf + boff + f * 2048 + foff[kk]);
      }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
          blk[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[a], bfr[b], blk[a][b], 0, 0, 0);
    }
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
    asm volatile("" ::: "memory");   // the next DMA into this buffer stays behind its reads
  }

  // ---- epilogue ----
  if constexpr (EPI == kTileSwiGLU) {
    const int I = N >> 1;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int m = m0 + 64 * wc + 16 * b + fr;
      if (m >= M) continue;
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
        *reinterpret_cast<bf16x4*>(y + (size_t)m * I + col) = o;
      }
    }
  } else {
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int n = n0 + 64 * wr + 16 * a + 4 * g;
      float bv[4] = {0.f, 0.f, 0.f, 0.f};
      if (bias) {
#pragma unroll
        for (int i = 0; i < 4; ++i) bv[i] = (float)bias[n + i];
      }
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int m = m0 + 64 * wc + 16 * b + fr;
        if (m >= M) continue;
        bf16x4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (bf16)(acc[a][b][i] + bv[i]);
        *reinterpret_cast<bf16x4*>(y + (size_t)m * N + n) = o;
      }
    }
  }
}

}  // namespace

int launch_gemm_fp8_block_tile(bf16* y, const bf16* x, const uint8_t* W, const float* bscale,
                               const bf16* bias, int M, int N, int K, bool swiglu,
                               hipStream_t stream) {
  if (M < 1 || N <= 0 || N % kTN != 0 || K <= 0 || K % 128 != 0) return -1;
  if (swiglu && bias != nullptr) return -4;
  if (y == nullptr || x == nullptr || W == nullptr || bscale == nullptr) return -5;
  const int tiles_m = (M + kTM - 1) / kTM, tiles_n = N / kTN;
  if ((long)tiles_m * tiles_n > (1L << 30)) return -3;
  const int grid = tiles_m * tiles_n;
  if (swiglu)
    fp8_block_tile_kernel<kTileSwiGLU><<<grid, kThreads, 0, stream>>>(x, W, bscale, bias, y, M, N,
                                                                     K, tiles_m, tiles_n);
  else
    fp8_block_tile_kernel<kTilePlain><<<grid, kThreads, 0, stream>>>(x, W, bscale, bias, y, M, N,
                                                                    K, tiles_m, tiles_n);
  return 0;
}

}  // namespace dli
