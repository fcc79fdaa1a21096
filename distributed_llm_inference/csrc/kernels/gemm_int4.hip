// Int4 group-quantised weights (AWQ / GPTQ checkpoints, ops.quantize_int4): unsigned nibbles
// q[n, k] in 0..15, one fp16 scale s and one zero point z in 0..15 per weight row and 128 k,
//   w[n, k] = (q[n, k] - z[k / 128, n]) * s[k / 128, n],
// W [N, K / 2] bytes, scale [K / 128, N] fp16, zero [K / 128, N] bytes (the checkpoints' own
// layout of the two tables).  N % 32 == 0, K % 128 == 0.  Two kernels:
//
// (a) small_gemm_int4_kernel: y[M, N] = x[M, K] . w^T (+ bias) for 1-32 bf16 rows, fp32
//     accumulation, one bf16 rounding.  The geometry of gemm_fp8_block_small.hip -- 32 weight rows
//     per workgroup = two 16-row A tiles, the 8 waves split K in 128-k steps, x staged per wave
//     through LDS by LDS-DMA with wstream_core.h's swizzle, the wave-order K-split sum, MT = 1 / 2
//     B tiles for <= 16 / 32 rows, v_mfma_f32_16x16x32_bf16 -- with a k-loop of its own
//     (ws_accumulate is not touched: its four formats are pinned bit for bit).
//
//   * nibble order.  Eight consecutive k of a row are one 32-bit word whose nibble p (bits 4 p ..
//     4 p + 3) holds k = 8 w + [0, 2, 4, 6, 1, 3, 5, 7][p] (ops.reference.pack_int4).  Elements
//     2 m and 2 m + 1 -- one dword of the MFMA's bf16 A fragment -- sit 16 bits apart, so
//     (word >> 4 m) & 0x000F000F is the pair in place.
//   * loads.  Lane (r, g) of A tile a loads, per step t (= one scale group), the 16 bytes
//     W[n0 + 16 a + r][64 t + 16 g ..] (32 nibbles; dword i is its A fragment of MFMA i, k =
//     128 t + 32 g + 8 i + j), non-temporal; the four fp16 scales (8 bytes) and the four zero
//     bytes (4 bytes) of its OUTPUT rows n0 + 16 a + 4 g + e, e = 0..3 (the C/D layout: lane
//     (c, g) holds D[n = 4 g + e][m = c]).  All three are issued together, before the next x
//     stage, so wstream_core.h's counted vmcnt waits ("all but the 4 MT newest") cover them.
//   * the zero point: the offset form.  gfx950 has no int4 -> bf16 convert and no packed bf16
//     add, and s, z belong to (row, group), not to a 16-row tile, so the zero point cannot be
//     spent in the widening.  The pair is widened as (bits & 0x000F000F) | 0x43004300: bf16
//     128 + q, exact (128 has an ulp of 1 in bf16) -- 7 vector ALU operations per 8 weights.  The
//     step's four MFMAs per A and B tile run into a zeroed accumulator, step = sum_k (128 + q) x.
//     Four more MFMAs per B tile and step (shared by both A tiles) with an all-ones A operand
//     give sumx = sum_k x[k, m] of the step in all four registers of lane (c, g), and
//       acc[e] += s[e] * (step[e] - (128 + z[e]) * sumx)
//     follows in fp32 on the vector ALU as two explicit fused multiply-adds per value (the same
//     value from v_fma_f32 or v_pk_fma_f32: the file needs no special flags).  The alternative,
//     exact q - z in fp32 then v_cvt_pk_bf16_f32, costs about twice the vector ALU work per
//     weight; it was not built or measured.  The price of the offset form is cancellation: the
//     step sum carries magnitudes up to 143 |x| instead of 15 |x| into the fp32 accumulator (the
//     tests' bound says so).  No dequantised weight is written anywhere; the activations stay bf16.
//   * kUnroll = 4 steps of loads in flight per lane: 8 16-byte weight loads, the bytes in flight
//     of the fp8 siblings' kUnroll = 2.  Chosen from the ISA (no scratch, below); not measured
//     against kUnroll = 2.
//   * epilogues: gemm_fp8_block_small.hip's.  Plain (+ bias) in fp32, one rounding, one 8-byte
//     store per lane; SwiGLU on swiglu_interleave'd rows: gate and up each rounded to bf16, then
//     silu(gate) * up -- ops.swiglu_interleaved of the plain output, bit for bit.
//
// (b) dequant_int4_kernel: out[N, K] = bf16((q - z) * s), the product in fp32 (exact: 5 x 11
//     significant bits), one rounding.  For products of more than 32 rows, which run the bf16 GEMM
//     path on the dequantised weight (ops.linear_int4); a tile GEMM on the int4 bytes is not
//     built.  One workgroup = 64 weight rows x 128 k (one scale group): the 64 scales and zeros
//     go through LDS, every thread loads 16 bytes (32 nibbles) and stores 4 x 16 bytes.
#include "wstream_core.h"

#include <hip/hip_fp16.h>

namespace dli {

namespace {

constexpr int kUnroll = 4;             // k-steps of weight / scale / zero loads in flight per lane
constexpr unsigned kBf16x2_128 = 0x43004300u;   // bf16 pair (128.0, 128.0)
constexpr unsigned kBf16x2_1 = 0x3F803F80u;     // bf16 pair (1.0, 1.0)

enum SmallEp { kSmallPlain = 0, kSmallSwiGLU = 1 };

// the 8 nibbles of `d` (pack_int4 order) as the bf16 values 128 + q, elements 0..7
__device__ __forceinline__ bf16x8 int4x8_to_bf16x8_off(unsigned d) {
  u32x4w v;
#pragma unroll
  for (int m = 0; m < 4; ++m) v[m] = ((d >> (4 * m)) & 0x000F000Fu) | kBf16x2_128;
  return __builtin_bit_cast(bf16x8, v);
}

template <int MT, int EPI>
__global__ void __launch_bounds__(kWsThreads)
small_gemm_int4_kernel(const bf16* __restrict__ x, const uint8_t* __restrict__ W,
                       const uint16_t* __restrict__ scale, const uint8_t* __restrict__ zero,
                       const bf16* __restrict__ bias, bf16* __restrict__ y, int M, int N, int K) {
  __shared__ __attribute__((aligned(1024))) char smem[kWsSmem<MT>];
  constexpr int kXBuf = MT * 16 * 256;   // one k-step of x: 16 MT rows x 128 bf16
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * kWsRowsWg;   // N % 32 == 0: both A tiles are whole
  const int kt = K >> 7;
  char* xw = smem + wave * (2 * kXBuf);   // this wave's two x buffers; nobody else touches them

  // lane (r, g): the weight row of A tile a at its 32-k block of step 0, and the scale / zero
  // entries of its four output rows n0 + 16 a + 4 g + e at group 0
  const uint8_t* wp[2];
  const uint16_t* sp[2];
  const uint8_t* zp[2];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    wp[a] = W + (size_t)(n0 + 16 * a + r) * (size_t)(K >> 1) + 16 * g;
    sp[a] = scale + n0 + 16 * a + 4 * g;
    zp[a] = zero + n0 + 16 * a + 4 * g;
  }
  // x staging and fragment reads: wstream_core.h's image (rows past M repeat row M - 1)
  const bf16* xsrc[4 * MT];
#pragma unroll
  for (int q = 0; q < 4 * MT; ++q) {
    const int row = 4 * q + g;
    xsrc[q] = x + (size_t)min(row, M - 1) * K + ((r ^ swz(row & 15)) << 3);
  }
  int xoff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) xoff[i] = r * 256 + (((4 * g + i) ^ swz(r)) << 4);

  f32x4 acc[2][MT];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < MT; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bf16x8 ones = __builtin_bit_cast(bf16x8, u32x4w{kBf16x2_1, kBf16x2_1, kBf16x2_1, kBf16x2_1});

  // k-step t < kt: every address stays inside its row / table (K % 128 == 0, N % 32 == 0)
  auto load_w = [&](int t, u32x4w (&wv)[2], uint2 (&sc)[2], unsigned (&zr)[2]) {
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      wv[a] = __builtin_nontemporal_load(reinterpret_cast<const u32x4w*>(wp[a] + (size_t)t * 64));
      sc[a] = *reinterpret_cast<const uint2*>(sp[a] + (size_t)t * N);
      zr[a] = *reinterpret_cast<const unsigned*>(zp[a] + (size_t)t * N);
    }
  };
  auto stage_x = [&](int t, int buf) {
#pragma unroll
    for (int q = 0; q < 4 * MT; ++q)
      glds16(xsrc[q] + (size_t)t * 128, xw + buf * kXBuf + q * 1024);
  };
  auto step = [&](int buf, const u32x4w (&wv)[2], const uint2 (&sc)[2], const unsigned (&zr)[2]) {
    bf16x8 xb[MT][4];
#pragma unroll
    for (int b = 0; b < MT; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        xb[b][i] = *reinterpret_cast<const bf16x8*>(xw + buf * kXBuf + b * 4096 + xoff[i]);
    // sum_k x[k, m] of the step: an all-ones A operand, so every register of lane (c, g) holds it
    f32x4 sx[MT];
#pragma unroll
    for (int b = 0; b < MT; ++b) {
      sx[b] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 4; ++i)
        sx[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, xb[b][i], sx[b], 0, 0, 0);
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      f32x4 part[MT];   // this step's sum_k (128 + q) x, before zero point and scale
#pragma unroll
      for (int b = 0; b < MT; ++b) part[b] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bf16x8 wf = int4x8_to_bf16x8_off(wv[a][i]);
#pragma unroll
        for (int b = 0; b < MT; ++b)
          part[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xb[b][i], part[b], 0, 0, 0);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned sbits = e < 2 ? sc[a].x : sc[a].y;
        const float s = __half2float(__ushort_as_half((unsigned short)(sbits >> (16 * (e & 1)))));
        const float nz = -(128.f + (float)((zr[a] >> (8 * e)) & 0xFFu));   // exact: <= 143
#pragma unroll
        for (int b = 0; b < MT; ++b)
          acc[a][b][e] = __builtin_fmaf(s, __builtin_fmaf(nz, sx[b][e], part[b][e]), acc[a][b][e]);
      }
    }
  };

  // wstream_core.h's pipeline: this wave's steps are t = wave + i kWsWaves, i < nsteps.  On
  // entering a group of kUnroll steps the x of its first step is the only memory operation in
  // flight; the group's weight, scale and zero loads follow it, and every step first sends the
  // next step's x into the other buffer, then waits for all but those 4 MT newest operations.
  static_assert(kUnroll % 2 == 0, "a group starts on x buffer 0");
  const int nsteps = wave < kt ? (kt - wave + kWsWaves - 1) / kWsWaves : 0;
  if (nsteps > 0) stage_x(wave, 0);
  int i = 0;
  for (; i + kUnroll <= nsteps; i += kUnroll) {
    u32x4w wv[kUnroll][2];
    uint2 sc[kUnroll][2];
    unsigned zr[kUnroll][2];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) load_w(wave + (i + u) * kWsWaves, wv[u], sc[u], zr[u]);
    asm volatile("" ::: "memory");
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      if (u + 1 < kUnroll || i + kUnroll < nsteps) {
        stage_x(wave + (i + u + 1) * kWsWaves, (u + 1) & 1);
        wait_vm<4 * MT>();
      } else {
        wait_vm<0>();
      }
      step(u & 1, wv[u], sc[u], zr[u]);
      asm volatile("" ::: "memory");   // the next DMA into this buffer stays behind its reads
    }
  }
  for (; i < nsteps; ++i) {   // fewer than kUnroll steps left
    u32x4w wv[2];
    uint2 sc[2];
    unsigned zr[2];
    load_w(wave + i * kWsWaves, wv, sc, zr);
    asm volatile("" ::: "memory");
    if (i + 1 < nsteps) {
      stage_x(wave + (i + 1) * kWsWaves, (i + 1) & 1);
      wait_vm<4 * MT>();
    } else {
      wait_vm<0>();
    }
    step(i & 1, wv, sc, zr);
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
  for (int w = 1; w < kWsWaves; ++w) {
    const float* red = reinterpret_cast<const float*>(smem + w * (2 * kXBuf));
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < MT; ++b)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[a][b][e] += red[((a * MT + b) * 4 + e) * 64 + lane];
  }

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
void launch_t(bf16* y, const bf16* x, const uint8_t* W, const uint16_t* scale, const uint8_t* zero,
              const bf16* bias, int M, int N, int K, bool swiglu, hipStream_t stream) {
  const int grid = N / kWsRowsWg;
  if (swiglu)
    small_gemm_int4_kernel<MT, kSmallSwiGLU><<<grid, kWsThreads, 0, stream>>>(
        x, W, scale, zero, bias, y, M, N, K);
  else
    small_gemm_int4_kernel<MT, kSmallPlain><<<grid, kWsThreads, 0, stream>>>(
        x, W, scale, zero, bias, y, M, N, K);
}

// ---------------------------------------------------------------------------------- dequantiser
constexpr int kDqRows = 64;       // weight rows per workgroup
constexpr int kDqThreads = 256;   // 4 threads per row: 32 k (16 bytes in, 64 bytes out) each

__global__ void __launch_bounds__(kDqThreads)
dequant_int4_kernel(const uint8_t* __restrict__ W, const uint16_t* __restrict__ scale,
                    const uint8_t* __restrict__ zero, bf16* __restrict__ out, int N, int K) {
  __shared__ float s_sh[kDqRows];
  __shared__ float z_sh[kDqRows];
  const int t = blockIdx.x;                 // scale group: k = 128 t .. 128 t + 127
  const int n0 = blockIdx.y * kDqRows;
  const int tid = threadIdx.x;
  if (tid < kDqRows && n0 + tid < N) {
    s_sh[tid] = __half2float(__ushort_as_half(scale[(size_t)t * N + n0 + tid]));
    z_sh[tid] = (float)zero[(size_t)t * N + n0 + tid];
  }
  __syncthreads();
  const int row = tid >> 2, ch = tid & 3;
  const int n = n0 + row;
  if (n >= N) return;
  const float s = s_sh[row], z = z_sh[row];
  const u32x4w v = *reinterpret_cast<const u32x4w*>(W + (size_t)n * (size_t)(K >> 1) + 64 * t +
                                                    16 * ch);
  bf16* o = out + (size_t)n * K + 128 * t + 32 * ch;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    bf16x8 ov;
#pragma unroll
    for (int j = 0; j < 8; ++j) {   // element j is nibble j / 2 + 4 (j & 1) of the word
      const float q = (float)((v[w] >> (4 * ((j >> 1) + 4 * (j & 1)))) & 0xFu);
      ov[j] = (bf16)((q - z) * s);
    }
    *reinterpret_cast<bf16x8*>(o + 8 * w) = ov;
  }
}

}  // namespace

int launch_small_gemm_int4(bf16* y, const bf16* x, const uint8_t* W, const uint16_t* scale,
                           const uint8_t* zero, const bf16* bias, int M, int N, int K, bool swiglu,
                           hipStream_t stream) {
  if (M < 1 || M > 32 || N <= 0 || N % 32 != 0 || K <= 0 || K % 128 != 0) return -1;
  if (swiglu && bias != nullptr) return -4;
  if (y == nullptr || x == nullptr || W == nullptr || scale == nullptr || zero == nullptr)
    return -5;
  if (M <= 16) launch_t<1>(y, x, W, scale, zero, bias, M, N, K, swiglu, stream);
  else launch_t<2>(y, x, W, scale, zero, bias, M, N, K, swiglu, stream);
  return 0;
}

int launch_dequant_int4(bf16* out, const uint8_t* W, const uint16_t* scale, const uint8_t* zero,
                        int N, int K, hipStream_t stream) {
  if (N <= 0 || N % 32 != 0 || K <= 0 || K % 128 != 0) return -1;
  if (out == nullptr || W == nullptr || scale == nullptr || zero == nullptr) return -5;
  const dim3 grid(K / 128, (N + kDqRows - 1) / kDqRows);
  dequant_int4_kernel<<<grid, kDqThreads, 0, stream>>>(W, scale, zero, out, N, K);
  return 0;
}

}  // namespace dli
