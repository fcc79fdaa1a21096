// Weight-streaming MFMA GEMM for fp8 (e4m3fn) weights and 3-32 bf16 activation rows:
//   y[M, N] = (x[M, K] . W8[N, K]^T) * w_scale[n] (+ bias), fp32 accumulation, one bf16 rounding.
// The regime between the fp8 GEMV (gemv.hip, 1-2 rows) and the block-scaled tile GEMM
// (gemm_tile.hip, 16 rows and more): gemm_fp4_small.hip's design on 1-byte weights.  All
// activation rows fit the 16 columns of one (M <= 16) or two (M <= 32) MFMA B tiles, so the
// product is a pure weight stream -- every weight byte is read once -- and the activations are
// never quantised: the weight is widened e4m3 -> bf16 in registers (v_cvt_scalef32_pk_bf16_fp8,
// scale 1.0; exact, every e4m3 value is a bf16 value) and multiplied on
// v_mfma_f32_16x16x32_bf16.  These are the fp8 GEMV's numerics for bf16 rows
// (skinny_gemm_fp8 without x_scale) up to summation order.
//
//   * operands.  The weight is the MFMA's A operand (lane l = (r = l & 15, g = l >> 4) holds
//     A[row r][k = 8 g + j], j = 0..7), the activations its B operand (B[k = 8 g + j][col r]).
//     The k order inside a step is free as long as A and B agree, so a 128-k step t is four
//     MFMAs whose "k = 8 g + j" is really k = 128 t + 32 g + 8 i + j for MFMA i = 0..3:
//       - lane (r, g) loads the 32 bytes W8[n0 + r][128 t + 32 g .. + 31] as two non-temporal
//         16-byte loads; dwords 2 i and 2 i + 1 of the 8, widened (4 converts), are the lane's
//         A fragment of MFMA i;
//       - the B fragment of MFMA i at lane (c, g) is the 16 bytes x[c][128 t + 32 g + 8 i .. + 7]:
//         64 consecutive bytes of x per lane and step.
//     4 MFMAs and 16 converts per 32 weights, as in the fp4 kernel; no lane movement, and no
//     scale in the loop: the per-row scale multiplies the fp32 accumulator in the epilogue.
//   * x through LDS.  As in the fp4 kernel: each wave stages the x of its own k-step (16 MT rows
//     x 256 B) in a private LDS buffer by LDS-DMA, whole 256-byte row pieces per 16 lanes, one
//     step ahead of the MFMAs (two buffers per wave, no workgroup barrier), and reads the
//     fragments back with ds_read_b128.  The image is lane-linear (DMA), so the bank swizzle sits
//     on the source address: slot p of row c holds chunk p ^ swz(c), swz(c) = c ^ ((c & 4) << 1).
//   * rows.  A workgroup owns kRowsWg = 32 consecutive weight rows = two A tiles, so every x
//     fragment feeds two MFMAs.  MT = 1 / 2 B tiles cover M <= 16 / 32; rows past M (and weight
//     rows past N, when N % 32 == 16) are clamped on load and never stored.
//   * parallelism.  The kWaves waves of the workgroup split K: wave w takes the steps t = w,
//     w + kWaves, ... (at any moment the workgroup reads kWaves x 128 consecutive bytes of each of
//     its rows), kUnroll steps = 4 x kUnroll 16-byte weight loads in flight per lane -- the fp4
//     kernel's bytes in flight at half its kUnroll.  The partial accumulators meet in LDS and
//     wave 0 adds them in wave order: deterministic, no atomics, no cross-workgroup hand-off.
//   * epilogues.  C/D: lane (c, g) holds D[n = 4 g + e][m = c], e = 0..3 -- four consecutive
//     output columns of activation row c, so four row scales per tile.  Plain: acc * scale
//     (+ bias) in fp32, one rounding, one 8-byte store.  SwiGLU (swiglu_interleave'd weight rows:
//     rows 32 b .. 32 b + 15 are the gates and 32 b + 16 .. 32 b + 31 the ups of output columns
//     16 b .. 16 b + 15): the two A tiles of the workgroup hold gate and up of one output column
//     in the same lane and register; each is scaled by its own row's scale and rounded to bf16
//     first, then silu(gate) * up -- ops.swiglu_interleaved on the bf16 product, bit for bit.
#include "kernels.h"

namespace dli {

namespace {

constexpr int kWaves = 8;              // K-split ways = waves per workgroup
constexpr int kThreads = kWaves * 64;
constexpr int kRowsWg = 32;            // weight rows per workgroup: two 16-row A tiles
constexpr int kUnroll = 2;             // k-steps of weight loads in flight per lane
static_assert(kUnroll % 2 == 0, "a group starts on x buffer 0");

enum SmallEp { kSmallPlain = 0, kSmallSwiGLU = 1 };

typedef unsigned u32x4s __attribute__((ext_vector_type(4)));   // nontemporal-loadable 16 B

// two dwords = 8 e4m3 bytes -> 8 bf16 (exact), in byte order
__device__ __forceinline__ bf16x8 widen8(unsigned lo, unsigned hi) {
  return fp8x8_to_bf16x8(uint2{lo, hi});
}

typedef __attribute__((address_space(3))) void lds_void_s;
typedef __attribute__((address_space(1))) void gbl_void_s;

// 16 bytes per lane global -> LDS (LDS-DMA): the wave's 64 lanes fill 1 KB at `lds_wave_base`
__device__ __forceinline__ void glds16(const void* g, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((gbl_void_s*)g, (lds_void_s*)lds_wave_base, 16, 0, 0);
}
template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// the 16-byte slot of chunk ch of x row c in the staged image is ch ^ swz(c)
__device__ __forceinline__ int swz(int c) { return c ^ ((c & 4) << 1); }

template <int MT, int EPI>
__global__ void __launch_bounds__(kThreads)
small_gemm_fp8_kernel(const bf16* __restrict__ x, const uint8_t* __restrict__ W,
                      const float* __restrict__ wscale, const bf16* __restrict__ bias,
                      bf16* __restrict__ y, int M, int N, int K) {
  constexpr int kXBuf = MT * 16 * 256;   // one k-step of x: 16 MT rows x 128 bf16
  __shared__ __attribute__((aligned(1024))) char smem[kWaves * 2 * kXBuf];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * kRowsWg;
  const int kt = K >> 7;
  char* xw = smem + wave * (2 * kXBuf);   // this wave's two x buffers; nobody else touches them

  // this lane's weight rows (A tiles 0 / 1), clamped into W, at its 32-k block of step 0
  const uint8_t* wp[2];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const size_t n = (size_t)min(n0 + 16 * a + r, N - 1);
    wp[a] = W + n * (size_t)K + 32 * g;
  }
  // x staging: DMA instruction q fills image rows 4 q .. 4 q + 3 (lane l: row 4 q + (l >> 4),
  // slot l & 15) with whole 256-byte row pieces; the slot permutation is on the source address.
  // Rows past M are clamped into x.
  const bf16* xsrc[4 * MT];
#pragma unroll
  for (int q = 0; q < 4 * MT; ++q) {
    const int row = 4 * q + g;
    xsrc[q] = x + (size_t)min(row, M - 1) * K + ((r ^ swz(row & 15)) << 3);
  }
  // ... and the fragment reads: B fragment i of lane (c = r, g) is chunk 4 g + i of row 16 b + c
  int xoff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) xoff[i] = r * 256 + (((4 * g + i) ^ swz(r)) << 4);

  f32x4 acc[2][MT];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < MT; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  // k-step t < kt: every address below stays inside its row (K % 128 == 0)
  auto load_w = [&](int t, u32x4s (&wv)[2][2]) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int h = 0; h < 2; ++h)
        wv[a][h] = __builtin_nontemporal_load(
            reinterpret_cast<const u32x4s*>(wp[a] + (size_t)t * 128 + 16 * h));
  };
  auto stage_x = [&](int t, int buf) {
#pragma unroll
    for (int q = 0; q < 4 * MT; ++q)
      glds16(xsrc[q] + (size_t)t * 128, xw + buf * kXBuf + q * 1024);
  };
  auto step = [&](int buf, const u32x4s (&wv)[2][2]) {
    bf16x8 xb[MT][4];
#pragma unroll
    for (int b = 0; b < MT; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        xb[b][i] = *reinterpret_cast<const bf16x8*>(xw + buf * kXBuf + b * 4096 + xoff[i]);
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bf16x8 wf = widen8(wv[a][i >> 1][2 * (i & 1)], wv[a][i >> 1][2 * (i & 1) + 1]);
#pragma unroll
        for (int b = 0; b < MT; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xb[b][i], acc[a][b], 0, 0, 0);
      }
    }
  };

  // This wave's steps are t = wave + i kWaves, i < nsteps.  On entering a group of kUnroll steps
  // the x of its first step is the only memory operation in flight; the group's weight loads
  // follow it, and every step first sends the next step's x into the other buffer, then waits
  // for all but those 4 MT newest operations (vmcnt counts in issue order).
  const int nsteps = wave < kt ? (kt - wave + kWaves - 1) / kWaves : 0;
  if (nsteps > 0) stage_x(wave, 0);
  int i = 0;
  for (; i + kUnroll <= nsteps; i += kUnroll) {   // whole groups; kUnroll is even: buffer u & 1
    u32x4s wv[kUnroll][2][2];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) load_w(wave + (i + u) * kWaves, wv[u]);
    asm volatile("" ::: "memory");
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      if (u + 1 < kUnroll || i + kUnroll < nsteps) {
        stage_x(wave + (i + u + 1) * kWaves, (u + 1) & 1);
        wait_vm<4 * MT>();
      } else {
        wait_vm<0>();
      }
      step(u & 1, wv[u]);
      asm volatile("" ::: "memory");   // the next DMA into this buffer stays behind its reads
    }
  }
  for (; i < nsteps; ++i) {   // fewer than kUnroll steps left
    u32x4s wv[2][2];
    load_w(wave + i * kWaves, wv);
    asm volatile("" ::: "memory");
    if (i + 1 < nsteps) {
      stage_x(wave + (i + 1) * kWaves, (i + 1) & 1);
      wait_vm<4 * MT>();
    } else {
      wait_vm<0>();
    }
    step(i & 1, wv);
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
  if (wave > 0) return;
#pragma unroll
  for (int w = 1; w < kWaves; ++w) {
    const float* red = reinterpret_cast<const float*>(smem + w * (2 * kXBuf));
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < MT; ++b)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[a][b][e] += red[((a * MT + b) * 4 + e) * 64 + lane];
  }

  // ---- epilogue: acc[a][b][e] = y[m = 16 b + r][n = n0 + 16 a + 4 g + e] ----
  // the scales of the lane's four weight rows per tile (clamped: an absent tile is never stored)
  float ws[2][4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int e = 0; e < 4; ++e) ws[a][e] = wscale[min(n0 + 16 * a + 4 * g + e, N - 1)];
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
        const float gt = (float)(bf16)(acc[0][b][e] * ws[0][e]);
        const float up = (float)(bf16)(acc[1][b][e] * ws[1][e]);
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
          float v = acc[a][b][e] * ws[a][e];
          if (bias) v += (float)bias[n + e];
          o[e] = (bf16)v;
        }
        *reinterpret_cast<bf16x4*>(y + (size_t)m * N + n) = o;
      }
    }
  }
}

template <int MT>
void launch_t(bf16* y, const bf16* x, const uint8_t* W, const float* wscale, const bf16* bias,
              int M, int N, int K, bool swiglu, hipStream_t stream) {
  const int grid = (N + kRowsWg - 1) / kRowsWg;
  if (swiglu)
    small_gemm_fp8_kernel<MT, kSmallSwiGLU><<<grid, kThreads, 0, stream>>>(x, W, wscale, bias, y,
                                                                         M, N, K);
  else
    small_gemm_fp8_kernel<MT, kSmallPlain><<<grid, kThreads, 0, stream>>>(x, W, wscale, bias, y,
                                                                        M, N, K);
}

}  // namespace

int launch_small_gemm_fp8(bf16* y, const bf16* x, const uint8_t* W, const float* wscale,
                          const bf16* bias, int M, int N, int K, bool swiglu,
                          hipStream_t stream) {
  if (M < 3 || M > 32 || N <= 0 || N % 16 != 0 || K <= 0 || K % 128 != 0) return -1;
  if (swiglu && (N % 32 != 0 || bias != nullptr)) return -4;
  if (y == nullptr || x == nullptr || W == nullptr || wscale == nullptr) return -5;
  if (M <= 16) launch_t<1>(y, x, W, wscale, bias, M, N, K, swiglu, stream);
  else launch_t<2>(y, x, W, wscale, bias, M, N, K, swiglu, stream);
  return 0;
}

}  // namespace dli
