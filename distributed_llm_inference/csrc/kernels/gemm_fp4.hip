// MXFP4-weight tile GEMM for CDNA4:  C[M, N] = A[M, K] . W[N, K]^T on the mixed-format block-scaled
// MFMA (v_mfma_scale_f32_16x16x128_f8f6f4, fp4 x fp8), for the batches the fp4 GEMV (gemv.hip,
// 1-2 rows) does not take.
//
//   A = MX fp8 activations: e4m3 bytes [M, K] + one e8m0 byte per (row, 128 columns) in common.h's
//       mx_off layout (quant.hip launch_quant_mx / ops.mx_quantize);
//   W = MXFP4 weights as the GEMV reads them: e2m1 nibbles [N, K / 2] (element 2j in the low nibble
//       of byte j) + one e8m0 byte per (row, 32 k) [N, K / 32].
//
// Both scale sets go to the MFMA's per-lane scale operands, so the accumulator holds the scaled
// product in fp32: no epilogue scaling, no dequantised copy of either operand.
//
// Structure: gemm_tile.hip's 256 x 256 workgroup tile (8 waves as 2 (M) x 4 (N), wave tile
// 128 x 64, LDS-DMA staging, two wave groups one barrier apart, XCD remap, weight as the MFMA's A
// operand so a lane owns 4 consecutive output columns), with a k-tile of 128 k = one MFMA k-step:
//
//   * k order (measured with one-hot operands, pinned by test_gemm_fp4_layout_bit_exact).  The two
//     formats sit differently in the k-step.  The fp4 operand's lane group g = lane >> 4 holds
//     k = 32 g .. 32 g + 31 in its four dwords, and lane (row, g)'s scale byte scales exactly
//     those 32: one real 32-block of the weight = the 16-byte chunk g of the k-tile's 64-byte
//     row.  The fp8 operand's lane group g holds k = 16 g .. 16 g + 15 in dwords 0-3 and
//     k = 64 + 16 g .. 64 + 16 g + 15 in dwords 4-7: the 16-byte chunks g and g + 4 of the
//     128-byte activation row -- gemm_tile.hip's fp8 fragment read, unchanged.  (Its scale byte
//     covers those two half-blocks; the activation scale is per 128 k, so that is immaterial.)
//   * staging.  Activations: two 128-row half-tiles of 128-byte rows, as gemm_tile.hip (swizzle
//     chunk ^ ((row >> 1) & 7)).  Weight: two 128-row half-tiles of 64-BYTE rows = 8 KB = one
//     `global_load_lds_dwordx4` per thread; LDS unit u = tid -> local row u >> 2, slot u & 3,
//     global chunk slot ^ ((row >> 2) & 3).  The 16 lanes of one fragment read (same g, rows
//     r .. r + 15) sit at byte (row & 3) * 64 + (g ^ ((row >> 2) & 3)) * 16 of four consecutive
//     256-byte bank lines: 16 distinct 16-byte slots, every bank once.
//     A buffer is 2 x 16 KB + 2 x 8 KB = 48 KB, double-buffered 96 KB.
//   * weight scales.  The 4 bytes of one (row, k-tile) are one aligned dword of the block-scale
//     row, and lane group g needs byte g (op_sel is an immediate).  Each wave stages the dwords of
//     its own 64 weight rows with one 4-byte LDS-DMA per k-tile, next to the weight halves, into
//     a slot only it reads; in phase 0 a lane reads byte g of its 4 rows (2 halves x 2 fragments)
//     with ds_read_u8.  (Loaded into registers a k-tile ahead instead, the compiler drains the
//     whole DMA queue -- vmcnt(0) -- before their first use in every k-tile.)
//   * activation scales.  As gemm_tile.hip kFp8Mx: the split's scales sit in LDS ([k-tile][256
//     rows]); a lane's dword holds the 4 rows (r, r + 16, r + 32, r + 48) it multiplies and the
//     MFMA's op_sel immediate picks the byte.
//   * per k-tile, 4 phases of one output quadrant (64 x 32 = 8 MFMAs of K = 128) each; the DMA
//     schedule is gemm_tile.hip's with the weight halves one instruction each, so the steady-state
//     wait is vmcnt(5): activation half 0 (2), both weight halves (1 + 1) and the weight scales
//     (1) of tile t + 2 in flight.
//   * epilogues: bf16 store, fp32 split-K slab (summed by launch_splitk_reduce or the consumer),
//     fused SwiGLU on swiglu_interleave'd weight rows (gemm_tile.hip kSwiGLU's pairing).
#include "kernels.h"

namespace dli {

namespace {

constexpr int kTM = 256, kTN = 256, kThreads = 512;
constexpr int kHalfA = 128 * 128;               // 128 rows x 128 fp8
constexpr int kHalfW = 128 * 64;                // 128 rows x 128 fp4
constexpr int kBuf = 2 * kHalfA + 2 * kHalfW;   // A0 A1 W0 W1: 48 KB
constexpr int kLds = 2 * kBuf;                  // double buffer: 96 KB
constexpr int kWsBuf = 8 * 256;                 // weight scales: [wave][64 rows] dwords, per buffer
constexpr int kMaxKt = 128;                     // k-tiles of activation scales a workgroup keeps
constexpr int kScLds = kMaxKt * 256;            // [k-tile][256 tile rows] bytes: 32 KB

enum Epilogue { kStoreBf16 = 0, kStoreF32 = 1, kSwiGLU = 2 };

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

// glds16 (common.h) with the non-temporal cache policy (NT): the weight stream, read by at most
// two M-tiles
__device__ __forceinline__ void dma16_nt(const void* g, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((gbl_void*)g, (lds_void*)lds_wave_base, 16, 0, 2);
}

__device__ __forceinline__ void barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// e2m1 (A operand, cbsz = 4: the first four operand dwords) x e4m3 (B operand, blgp = 0), K = 128.
// Lane l's byte 0 of `wsc` scales the weight's 32 k-values it holds (row l & 15, k-block l >> 4);
// byte SEL of `asc` scales its 32 activation values likewise.
template <int SEL>
__device__ __forceinline__ f32x4 mfma_w4(const i32x4& w, int wsc, const i32x4& a0, const i32x4& a1,
                                         const f32x4& c, int asc) {
  const i32x8 a = {w[0], w[1], w[2], w[3], 0, 0, 0, 0};
  const i32x8 b = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 4, 0, 0, wsc, SEL, asc);
}

// NT: weight half-tiles loaded non-temporal (launches with <= 2 M-tiles, as gemm_tile.hip VAR 1)
template <int EPI, bool NT>
__global__ void __launch_bounds__(kThreads, 1)
gemm_fp4_kernel(const uint8_t* __restrict__ A, const uint8_t* __restrict__ a_sc,
                const uint8_t* __restrict__ W, const uint8_t* __restrict__ w_sc,
                void* __restrict__ C, int M, int N, int K, int nb, int tiles_m, int tiles_n,
                int k_tiles_per_split) {
  const size_t Ka = (size_t)K;        // activation row stride in bytes
  const size_t Kw = (size_t)K >> 1;   // weight row stride in bytes
  const size_t Ks = (size_t)K >> 5;   // weight scale row stride in bytes
  const int kt_all = K >> 7;
  __shared__ __attribute__((aligned(1024))) char smem[kLds + 2 * kWsBuf + kScLds];

  // ---- XCD-aware, bijective block remap (consecutive logical ids share an XCD / its L2) ----
  const int nblk = (int)gridDim.x;
  const int bx = (int)blockIdx.x;
  const int xq = nblk >> 3, xr = nblk & 7, xx = bx & 7;
  const int lid = (xx < xr ? xx * (xq + 1) : xr * (xq + 1) + (xx - xr) * xq) + (bx >> 3);

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6, wr = wave >> 2, wc = wave & 3, fr = lane & 15;
  const int g = lane >> 4;
  const int tiles = tiles_m * tiles_n;
  const int tile = lid % tiles, split = lid / tiles;
  const int kt0 = split * k_tiles_per_split;
  const int T = min(k_tiles_per_split, kt_all - kt0);
  // M fastest: the M-tiles of one weight panel are neighbours (share it through the XCD's L2)
  const int tm = tile % tiles_m, tn = tile / tiles_m;
  const int m0 = tm * kTM, n0 = tn * kTN;

  // fragment read offsets: activation chunks g, g + 4 (swizzle (row >> 1) & 7), weight chunk g
  // (swizzle (row >> 2) & 3); the row multiples of 16 added per fragment leave both swizzles alone
  int sch[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) sch[kk] = ((kk * 4 + g) ^ (fr >> 1)) << 4;
  const int a_lane = (wr * 64 + fr) * 128;
  const int w_lane = (wc * 32 + fr) * 64 + ((g ^ ((fr >> 2) & 3)) << 4);

  // ---- DMA sources ----
  // activations: LDS units u = j*512 + tid (j = 0, 1) of each half; unit u -> local row u >> 3,
  // slot u & 7, global chunk slot ^ ((row >> 1) & 7)
  const uint8_t* srcA[2][2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int u = j * kThreads + tid;
    const int lr = u >> 3, ch = (u & 7) ^ ((lr >> 1) & 7);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int ga = (lr >> 6) * 128 + h * 64 + (lr & 63);
      const int ra = min(m0 + ga, M - 1);   // rows past M are computed, never stored
      srcA[h][j] = A + (size_t)ra * Ka + (size_t)kt0 * 128 + ch * 16;
    }
  }
  // weight: LDS unit u = tid of each half; local row u >> 2, slot u & 3
  const uint8_t* srcW[2];
  {
    const int lr = tid >> 2, ch = (tid & 3) ^ ((lr >> 2) & 3);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int gb = (lr >> 5) * 64 + h * 32 + (lr & 31);
      srcW[h] = W + (size_t)(n0 + gb) * Kw + (size_t)kt0 * 64 + ch * 16;
    }
  }
  // stage half `which` (0 = A0, 1 = A1, 2 = W0, 3 = W1) of k-tile t into buffer t & 1
  auto stage = [&](int which, int t) {
    char* buf = smem + (t & 1) * kBuf;
    if (which < 2) {
      char* dst = buf + which * kHalfA + wave * 1024;
#pragma unroll
      for (int j = 0; j < 2; ++j) glds16(srcA[which][j] + (size_t)t * 128, dst + j * 8192);
    } else {
      char* dst = buf + 2 * kHalfA + (which - 2) * kHalfW + wave * 1024;
      if (NT)
        dma16_nt(srcW[which - 2] + (size_t)t * 64, dst);
      else
        glds16(srcW[which - 2] + (size_t)t * 64, dst);
    }
  };
  // weight scales: every wave stages the k-tile's scale dwords of its own 64 weight rows (lane l:
  // row n0 + 64 wc + l) with one 4-byte LDS-DMA into its private slot of buffer t & 1, and is the
  // only reader of that slot (byte g of rows 32 h + 16 j + fr)
  const uint8_t* srcS = w_sc + (size_t)(n0 + wc * 64 + lane) * Ks + (size_t)kt0 * 4;
  auto stage_ws = [&](int t) {
    __builtin_amdgcn_global_load_lds((gbl_void*)(srcS + (size_t)t * 4),
                                     (lds_void*)(smem + kLds + (t & 1) * kWsBuf + wave * 256), 4,
                                     0, 0);
  };

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  i32x4 af[4][2], w0[2], w1[2];
  int s_mx[2] = {0, 0};    // this lane's 4 activation row scales of A-half 0 / 1, current k-tile
  int wsc[2][2];           // weight scales [half][fragment] of the current k-tile
  const char* sls = smem + kLds + 2 * kWsBuf;
  auto read_a = [&](const char* buf, int h, int t) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
        af[i][kk] = *reinterpret_cast<const i32x4*>(buf + h * kHalfA + a_lane + i * 16 * 128 + sch[kk]);
    s_mx[h] = *reinterpret_cast<const int*>(sls + t * 256 + wr * 128 + h * 64 + fr * 4);
  };
  auto read_ws = [&](int t) {
    const char* p = smem + kLds + (t & 1) * kWsBuf + wave * 256 + fr * 4 + g;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int j = 0; j < 2; ++j) wsc[h][j] = *reinterpret_cast<const uint8_t*>(p + (h * 32 + j * 16) * 4);
  };
  auto read_w = [&](const char* buf, int h, i32x4 (&wf)[2]) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
      wf[j] = *reinterpret_cast<const i32x4*>(buf + 2 * kHalfA + h * kHalfW + w_lane + j * 16 * 64);
  };
  auto quadrant = [&](int mq, int nq, const i32x4 (&wf)[2]) {
    __builtin_amdgcn_s_setprio(1);
    const int sc = s_mx[mq];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ws = wsc[nq][j];
      acc[mq * 4 + 0][nq * 2 + j] = mfma_w4<0>(wf[j], ws, af[0][0], af[0][1], acc[mq * 4 + 0][nq * 2 + j], sc);
      acc[mq * 4 + 1][nq * 2 + j] = mfma_w4<1>(wf[j], ws, af[1][0], af[1][1], acc[mq * 4 + 1][nq * 2 + j], sc);
      acc[mq * 4 + 2][nq * 2 + j] = mfma_w4<2>(wf[j], ws, af[2][0], af[2][1], acc[mq * 4 + 2][nq * 2 + j], sc);
      acc[mq * 4 + 3][nq * 2 + j] = mfma_w4<3>(wf[j], ws, af[3][0], af[3][1], acc[mq * 4 + 3][nq * 2 + j], sc);
    }
    // pin the segment here (gemm_tile.hip: without a use the compiler sinks the MFMAs of the
    // k-tile past the phase barriers)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) asm volatile("" : "+v"(acc[mq * 4 + i][nq * 2 + j]));
    __builtin_amdgcn_s_setprio(0);
  };

  // this split's activation scales -> LDS, before any LDS-DMA is in flight (plain loads):
  // k-tile t, 64-row block w >> 2 of the tile (clamped: rows past M are never stored)
  for (int u = tid; u < T * 16; u += kThreads) {
    const int t = u >> 4, w = u & 15;
    const int blk = min((m0 >> 6) + (w >> 2), nb - 1);
    const uint4 v = *reinterpret_cast<const uint4*>(a_sc + ((size_t)(kt0 + t) * nb + blk) * 64 +
                                                    (w & 3) * 16);
    *reinterpret_cast<uint4*>(smem + kLds + 2 * kWsBuf + t * 256 + w * 16) = v;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  // ---- prologue: tile 0 complete; A-half 0, both weight halves and the scales of tile 1 in flight
  if (T > 0) {
    stage(0, 0); stage(2, 0); stage(3, 0); stage_ws(0); stage(1, 0);
    if (T > 1) {
      stage(0, 1); stage(2, 1); stage(3, 1); stage_ws(1);
      asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  barrier();

  // the two wave groups (wr = 0 / 1, one wave of each per SIMD) run one barrier apart
  if (wr == 1) barrier();
  for (int t = 0; t < T; ++t) {
    const char* buf = smem + (t & 1) * kBuf;
    const bool more1 = t + 1 < T, more2 = t + 2 < T;
    // phase 0: quadrant (0, 0)
    read_a(buf, 0, t);
    read_w(buf, 0, w0);
    read_ws(t);
    if (more1) stage(1, t + 1);
    barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    quadrant(0, 0, w0);
    barrier();
    // phase 1: quadrant (0, 1)
    read_w(buf, 1, w1);
    barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    quadrant(0, 1, w1);
    barrier();
    // phase 2: quadrant (1, 1); A-half 0 was last read two phases ago
    read_a(buf, 1, t);
    if (more2) stage(0, t + 2);
    barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    quadrant(1, 1, w1);
    barrier();
    // phase 3: quadrant (1, 0); restage both weight halves and the weight scales; retire tile
    // t + 1 (all but the 5 newest DMA instructions: A-half 0, both weight halves and the scales
    // of tile t + 2)
    if (more2) {
      stage(2, t + 2);
      stage(3, t + 2);
      stage_ws(t + 2);
      asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    barrier();
    quadrant(1, 0, w0);
    barrier();
  }
  if (wr == 0) barrier();

  // ---- epilogue ----
  // The MFMAs compute the transposed tile (A operand = weight rows): fragment (i, j) element e of
  // lane l is C[row = 16 i + (l & 15)][col = 16 j + 4 (l >> 4) + e].
  const int crow = m0 + wr * 128 + fr;
  const int cq = 4 * g;
  if constexpr (EPI == kSwiGLU) {
    // n-fragments (2p, 2p+1) = (gate, up) of output columns n0/2 + wc*32 + p*16 + cq + e
    bf16* out = reinterpret_cast<bf16*>(C);
    const int I = N >> 1;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = crow + i * 16;
      if (row >= M) continue;
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          // round gate and up to bf16 first: matches the unfused GEMM -> silu_mul path
          const float gt = (float)(bf16)acc[i][2 * p][e];
          const float up = (float)(bf16)acc[i][2 * p + 1][e];
          o[e] = (bf16)(silu(gt) * up);
        }
        *reinterpret_cast<bf16x4*>(out + (size_t)row * I + (n0 >> 1) + wc * 32 + p * 16 + cq) = o;
      }
    }
  } else if constexpr (EPI == kStoreF32) {
    float* out = reinterpret_cast<float*>(C) + (size_t)split * M * N;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = crow + i * 16;
      if (row >= M) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        *reinterpret_cast<f32x4*>(out + (size_t)row * N + n0 + wc * 64 + j * 16 + cq) = acc[i][j];
    }
  } else {
    bf16* out = reinterpret_cast<bf16*>(C);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = crow + i * 16;
      if (row >= M) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (bf16)acc[i][j][e];
        *reinterpret_cast<bf16x4*>(out + (size_t)row * N + n0 + wc * 64 + j * 16 + cq) = o;
      }
    }
  }
}

template <bool NT>
int launch_impl(void* C, const uint8_t* a_q, const uint8_t* a_mx, const uint8_t* W,
                const uint8_t* bscale, float* workspace, int M, int N, int K, int splits, int kps,
                int epilogue, int tiles_m, int tiles_n, hipStream_t stream) {
  const int nb = (M + 63) / 64;
  const int grid = tiles_m * tiles_n * splits;
  if (splits > 1) {
    gemm_fp4_kernel<kStoreF32, NT><<<grid, kThreads, 0, stream>>>(
        a_q, a_mx, W, bscale, workspace, M, N, K, nb, tiles_m, tiles_n, kps);
    if (epilogue == kStoreF32) return 0;
    return launch_splitk_reduce(reinterpret_cast<bf16*>(C), workspace, splits, (size_t)M * N, stream);
  }
  if (epilogue == kSwiGLU)
    gemm_fp4_kernel<kSwiGLU, NT><<<grid, kThreads, 0, stream>>>(a_q, a_mx, W, bscale, C, M, N, K, nb,
                                                               tiles_m, tiles_n, kps);
  else
    gemm_fp4_kernel<kStoreBf16, NT><<<grid, kThreads, 0, stream>>>(a_q, a_mx, W, bscale, C, M, N, K,
                                                                  nb, tiles_m, tiles_n, kps);
  return 0;
}

}  // namespace

int gemm_fp4_max_ktiles() { return kMaxKt; }

int launch_gemm_fp4(void* C, const uint8_t* a_q, const uint8_t* a_mx, const uint8_t* W,
                    const uint8_t* bscale, float* workspace, int M, int N, int K, int splits,
                    int epilogue, hipStream_t stream) {
  if (M <= 0 || N <= 0 || K <= 0 || N % kTN != 0 || K % 128 != 0) return -1;
  if (a_q == nullptr || a_mx == nullptr || W == nullptr || bscale == nullptr) return -5;
  const int kt = K / 128;
  if (splits < 1 || splits > kt) return -2;
  const int kps = (kt + splits - 1) / splits;
  if ((splits - 1) * kps >= kt) return -2;   // every split owns at least one k-tile
  if (kps > kMaxKt) return -15;              // its activation scales must fit the LDS slot
  if (epilogue != kStoreBf16 && epilogue != kStoreF32 && epilogue != kSwiGLU) return -4;
  // split-K: fp32 slabs in the workspace, reduced here (epilogue 0) or by the consumer (1)
  if (splits > 1 && (workspace == nullptr || epilogue == kSwiGLU)) return -3;
  if (splits == 1 && epilogue == kStoreF32) return -3;
  if (epilogue != kStoreF32 && C == nullptr) return -3;
  const int tiles_m = (M + kTM - 1) / kTM, tiles_n = N / kTN;
  if ((long long)tiles_m * tiles_n * splits > 0x7fffffffLL) return -1;
  if (tiles_m <= 2)
    return launch_impl<true>(C, a_q, a_mx, W, bscale, workspace, M, N, K, splits, kps, epilogue,
                             tiles_m, tiles_n, stream);
  return launch_impl<false>(C, a_q, a_mx, W, bscale, workspace, M, N, K, splits, kps, epilogue,
                            tiles_m, tiles_n, stream);
}

}  // namespace dli
