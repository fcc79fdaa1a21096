// Sparse mixture-of-experts MLP, quantised experts with many rows, on the block-scaled MFMA: the two
// products of moe_tile.hip (gate|up + SwiGLU, down + scatter) with the stored weight bytes and MX
// fp8 activations multiplied by v_mfma_scale_f32_16x16x128_f8f6f4 as they are stored.  Nothing is
// widened to bf16 and no operand is dequantised: a k-step of 128 is one MFMA per fragment pair, 16
// per wave, where moe_tile.hip's loop issues 64 bf16 MFMAs for the same k.  One kernel template,
// moe_tile_scaled_kernel<EPI, WF>, for three weight formats:
//
//   W  = MXFP4 (kExpertFp4): nibbles [E, N, K / 2] (element 2 j in the low nibble of byte j),
//        scale [E, N, K / 32] e8m0 bytes, as moe_tile.hip's MXFP4 kernel reads them;
//        fp8 (kExpertFp8): e4m3fn bytes [E, N, K], scale [E, N] fp32, one per weight row;
//        block-scaled fp8 (kExpertFp8Block): e4m3fn bytes [E, N, K] in stored row order, scale
//        [E, N / 16, K / 128] fp32, one per 16 stored rows and 128 k, as moe_tile_fp8_block.hip
//        reads them, neither tensor re-laid-out;
//   A  = e4m3 bytes [R, K] with ROW-MAJOR e8m0 scales [R, K / 128] (quant.hip
//        launch_quant_mx_rows).  The rows of a tile are gathered (gate|up: token
//        sorted_pairs[start + r] / k of x quantised once per token; down: row start + r of h
//        quantised in its sorted order), so mx_off's packing of four contiguous rows per dword
//        does not apply; row-major lets a gathered row bring its scales with it.
//
// Shared by the three formats:
//   * grid, prologue, clamps: moe_tile.hip's (moe_tile_parts.h).  Grid (N / 128, min(E, P) +
//     P / 128), fixed by (T, E, k, N); every wave derives its tile from expert_count /
//     expert_offset (lane l holds experts 4 l .. 4 l + 3, wave prefix sum over ceil(count / 128));
//     a tile index past the sum returns before any DMA, LDS write or barrier.  Counts are clamped
//     into [0, P], the expert into [0, E), rows into [1, 128], start + rows <= P, pair < P hence
//     token < T.  Image rows past the tile's count repeat its last row (bytes and scales; loaded
//     in bounds, computed, never stored).  No atomics, no host sync; a row's result depends on
//     that row and its expert only.
//   * 4 waves as 2 (weight rows) x 2 (activation rows), 64 x 64 per wave = 4 x 4 fragments, 16
//     MFMAs per wave and k-step.  The weight is the A operand, so a lane owns 4 consecutive
//     output columns of one row and both epilogues are moe_tile.hip's (moe_tile_parts.h): gate /
//     up are A fragments 2 p, 2 p + 1.  The activation's e8m0 byte is byte b of the B scale
//     dword, picked by op_sel.
//   * the activation tile: [128][128 B] = 16 KB per buffer, four rounds of lane-linear 16-byte
//     LDS-DMA with the swizzle in the source address (thread: row 32 j + (tid >> 3), slot tid & 7,
//     chunk slot ^ ((row >> 1) & 7)) -- gemm_fp4.hip's layout, whose ds_read_b128 fragment reads
//     touch every bank once.  The fp8 operand's lane group g = lane >> 4 holds the 16-byte chunks
//     g and g + 4 of the step's 128-byte row.
//   * two buffers (weight tile, then activation tile), one barrier per k-step:  wait for step
//     t's DMA, barrier; send step t + 1 into the other buffer; multiply t.  Any number of k-steps
//     >= 1.
//   * activation scales: the tile's [K / 128][128 rows] bytes are staged in LDS once, in the
//     prologue, by plain loads before any DMA is in flight (thread: image row tid & 127, k-steps
//     of parity tid >> 7), transposed into the MFMA's order: the dword of (k-step t, wave column
//     wc, fr) holds image rows 64 wc + fr + 16 b in byte b, so a lane reads one dword per k-step
//     and the op_sel immediate b picks the fragment's row.  The slot bounds the supported K:
//     K / 128 <= 128 k-steps, K <= 16384 (16 KB), which covers Qwen3-30B-A3B (2048 / 768),
//     Mixtral-8x7B (4096 / 14336) and Qwen2-MoE (I = 1408, 2560).
//   * compiled without packed fp32 instructions: the block format's FMAs are v_fma_f32 /
//     v_fmac_f32.
//
// MXFP4 (cbsz = 4, the weight's four dwords in the low half of the operand):
//   * k order inside the step, as gemm_fp4.hip's header records it: the fp4 operand's lane group
//     g holds k = 32 g .. 32 g + 31, which is the 16-byte chunk g of the step's 64-byte weight
//     row, and its scale byte is byte g of the (row, k-step) scale dword.
//   * weight tile [128][64 B] = 8 KB per buffer (two DMA rounds; thread: row 64 j + (tid >> 2),
//     slot tid & 3, chunk slot ^ ((row >> 2) & 3)), gemm_fp4.hip's other layout.
//   * weight scales: on the instruction's scale operand, from a small per-wave LDS slot, as
//     gemm_fp4.hip.  Each wave sends the step's scale dwords of its own 64 weight rows (lane l:
//     row n0 + 64 wr + l) with ONE 4-byte LDS-DMA next to the operand DMAs, into a slot of the
//     buffer that only it reads (256 B per wave and buffer), and reads byte g of its four
//     fragment rows with ds_read_u8.  Chosen over registers a step ahead because that takes four
//     narrow loads per wave and k-step, each touching 16 rows -- the pattern that made the first
//     MXFP4 tile kernel 1.13-1.30x slower (moe_tile.hip's header) -- where the DMA is one
//     instruction touching 64 rows, retired by the vmcnt(0) the loop already has.  Both scale
//     sets on the instruction: the fp32 accumulator holds the finished product, the epilogue
//     scales nothing.
//   * LDS: 2 x 24 KB + 2 KB + 16 KB = 66 KB, two workgroups per CU.
//
// fp8 and block-scaled fp8 (cbsz = 0, all eight operand dwords; the weight's scale operand is the
// constant 127, 2^0):
//   * k order inside the step: both operands are read with the same lane / byte pattern, lane
//     group g holding the 16-byte chunks g and g + 4 of the step's 128-byte row, so the
//     instruction pairs equal k whatever order it gives the lane groups.
//   * weight tile [128][128 B] = 16 KB per buffer, staged and read exactly as the activation tile.
//   * LDS: 2 x 32 KB + 16 KB = 80 KB, half a CU's 160 KB: two workgroups per CU.
//   * fp8, weight scales: the 4 x 4 fp32 row scales a lane's accumulators need are loaded once,
//     before the k-loop, into registers (n0 + 64 wr + 16 a + 4 g .. + 3 < N).  No LDS slot, no DMA
//     in the loop.  They multiply the fp32 accumulators after the loop, before any rounding:
//     gate and up are each scaled by their own row's scale before their bf16 rounding, down
//     before its one rounding -- moe_tile.hip's fp8 rule, so exactly summable operands give that
//     kernel's bits.
//   * block-scaled fp8: the weight's fp32 block scale cannot ride on the instruction's e8m0 scale
//     operand and does not have to: one instruction consumes exactly one 128-k block, an A
//     fragment is exactly one 16-row scale group, so the scale is constant over a whole
//     instruction.  Every MFMA starts from a zero C operand and its result is folded into the
//     running accumulator by one FMA per element, acc = fma(scale, step, acc).  The k-step: 16
//     MFMAs, mutually independent (no accumulator chain), and 64 scalar-by-vector FMAs.  They
//     are written one A fragment apart -- the four MFMAs of fragment a + 1, then the sixteen FMAs
//     of fragment a -- so the FMAs issue while the matrix pipe works on the next fragment and
//     never wait on the instruction just issued.  A wave needs the 4 fp32 of groups
//     (n0 + 64 wr) / 16 + a at k-step t (in bounds: N % 128 == 0, t < K / 128).  They are loaded
//     one k-step ahead, next to that step's DMA issue, by plain wave-uniform vector loads that
//     the loop's vmcnt(0) wait covers together with the DMA.  No LDS slot; nothing is left to
//     scale in the epilogue.
//
// Compiler's resource summary (gate|up / down), no AGPRs, no scratch, 2 waves per SIMD: docs/
// kernels.md has the table.
#include "moe_tile_parts.h"

namespace dli {

namespace {

constexpr int kBK = 128;               // k per step = one MFMA = one scale block
constexpr int kGroup = 16;             // weight rows per block-scale group = one A fragment
constexpr int kAOp = kTM * kBK;        // 16 KB of e4m3
constexpr int kMaxKt = 128;            // k-steps of activation scales a workgroup keeps (16 KB)
// LDS: two buffers (weight tile | activation tile), MXFP4's weight scales ([wave][64 rows] dwords
// per buffer), the activation scales
template <int WF> constexpr int kWOp = WF == kExpertFp4 ? kTN * kBK / 2 : kTN * kBK;
template <int WF> constexpr int kBufOf = kWOp<WF> + kAOp;
template <int WF> constexpr int kWsBuf = WF == kExpertFp4 ? 4 * 256 : 0;
template <int WF> constexpr int kWsOff = 2 * kBufOf<WF>;
template <int WF> constexpr int kAsOff = kWsOff<WF> + 2 * kWsBuf<WF>;

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

// One 128-k block, weight fragment `w` (A operand) x e4m3 activation fragment `x` (B operand,
// blgp = 0), plus c.  MXFP4: e2m1, cbsz = 4, the first four operand dwords, byte 0 of `wsc` scales
// the lane's 32 weight values; fp8: e4m3, cbsz = 0, `wsc` = 127.  Byte SEL of `asc` scales the
// lane's 32 activation values
template <int WF, int SEL>
__device__ __forceinline__ f32x4 mfma_scaled(const i32x4* w, int wsc, const i32x4* x,
                                             const f32x4& c, int asc) {
  const i32x8 b = {x[0][0], x[0][1], x[0][2], x[0][3], x[1][0], x[1][1], x[1][2], x[1][3]};
  if constexpr (WF == kExpertFp4) {
    const i32x8 a = {w[0][0], w[0][1], w[0][2], w[0][3], 0, 0, 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 4, 0, 0, wsc, SEL, asc);
  } else {
    const i32x8 a = {w[0][0], w[0][1], w[0][2], w[0][3], w[1][0], w[1][1], w[1][2], w[1][3]};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0, wsc, SEL, asc);
  }
}

__device__ __forceinline__ void fold(f32x4& acc, float s, const f32x4& step) {
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = __builtin_fmaf(s, step[i], acc[i]);
}

template <int EPI, int WF>
__global__ void __launch_bounds__(kThreads, 2)
moe_tile_scaled_kernel(const uint8_t* __restrict__ aq, const uint8_t* __restrict__ asc,
                       const uint8_t* __restrict__ W, const void* __restrict__ wscale,
                       bf16* __restrict__ out, const int* __restrict__ sorted_pairs,
                       const int* __restrict__ expert_count, const int* __restrict__ expert_offset,
                       int E, int topk, int P, int N, int K) {
  constexpr bool kMx = WF == kExpertFp4;
  constexpr int kBuf = kBufOf<WF>;
  constexpr int kWk = kMx ? 1 : 2;       // 16-byte chunks of a lane's weight fragment
  __shared__ __attribute__((aligned(1024))) char smem[kAsOff<WF> + kMaxKt * kTM];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nb = blockIdx.x;

  int e, rows, start;
  if (!moe_tile_locate(expert_count, expert_offset, E, P, blockIdx.y, lane, e, rows, start)) return;
  const int* pairs = sorted_pairs + start;
  const int n0 = nb * kTN;
  const int kt = K / kBK;
  const size_t Ka = (size_t)K >> 7;

  // the activation row behind image row r: the pair's token (gate|up) or the sorted h row (down)
  auto src_row = [&](int r) -> size_t {
    const int tr = min(r, rows - 1);
    if constexpr (EPI == kMoeGateUp) return (size_t)(min(max(pairs[tr], 0), P - 1) / topk);
    else return (size_t)(start + tr);
  };

  // ---- activation scales of the whole tile -> LDS, transposed (plain loads, before any DMA) ----
  {
    const int r = tid & 127;
    const uint8_t* s = asc + src_row(r) * Ka;
    char* d = smem + kAsOff<WF> + (r >> 6) * 64 + (r & 15) * 4 + ((r >> 4) & 3);
    for (int t = tid >> 7; t < kt; t += 2) d[t * kTM] = (char)s[t];
  }

  // ---- staging: round j fills image rows 32 j .. 32 j + 31 of a 128-byte-row tile (thread: row
  // 32 j + (tid >> 3), slot tid & 7); the chunk that belongs in that slot is the same every round.
  // MXFP4's weight: round j fills image rows 64 j .. 64 j + 63 (row 64 j + (tid >> 2), slot tid & 3)
  const int wr = wave >> 1, wc = wave & 1, fr = lane & 15, g = lane >> 4;
  const int srow = tid >> 3;
  const int chunk = (tid & 7) ^ ((srow >> 1) & 7);
  const size_t Kw = (size_t)K >> (kMx ? 1 : 0);     // bytes of a stored weight row
  const uint8_t* wsrc;
  if constexpr (kMx) {
    const int qrow = tid >> 2;
    wsrc = W + ((size_t)e * N + n0 + qrow) * Kw + (((tid & 3) ^ ((qrow >> 2) & 3)) << 4);
  } else {
    wsrc = W + ((size_t)e * N + n0 + srow) * Kw + chunk * 16;
  }
  const uint8_t* xsrc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) xsrc[j] = aq + src_row(32 * j + srow) * (size_t)K + chunk * 16;
  // MXFP4's weight scales: the dword of (row n0 + 64 wr + lane, k-step) into the wave's own slot
  const uint8_t* ssrc = nullptr;
  if constexpr (kMx)
    ssrc = static_cast<const uint8_t*>(wscale) + ((size_t)e * N + n0 + 64 * wr + lane) * ((size_t)K >> 5);
  auto stage = [&](int t, int buf) {
    char* dst = smem + buf * kBuf + wave * 1024;
    if constexpr (kMx) {
#pragma unroll
      for (int j = 0; j < 2; ++j) glds16(wsrc + (size_t)j * 64 * Kw + (size_t)t * (kBK / 2), dst + j * 4096);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) glds16(wsrc + (size_t)j * 32 * Kw + (size_t)t * kBK, dst + j * 4096);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) glds16(xsrc[j] + (size_t)t * kBK, dst + kWOp<WF> + j * 4096);
    if constexpr (kMx)
      __builtin_amdgcn_global_load_lds(
          (gbl_void*)(ssrc + (size_t)t * 4),
          (lds_void*)(smem + kWsOff<WF> + buf * kWsBuf<WF> + wave * 256), 4, 0, 0);
  };

  // ---- fragments: activation chunks g, g + 4 of row 16 b + fr, and weight chunks g, g + 4 (fp8)
  // or chunk g (MXFP4) of row 16 a + fr, of the wave's 64 x 64 (the multiples of 16 leave the
  // swizzles alone) ----
  int woff[2] = {}, xoff[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    const int c = ((4 * kk + g) ^ ((fr >> 1) & 7)) << 4;
    if constexpr (!kMx) woff[kk] = (64 * wr + fr) * 128 + c;
    xoff[kk] = kWOp<WF> + (64 * wc + fr) * 128 + c;
  }
  if constexpr (kMx) woff[0] = (64 * wr + fr) * 64 + ((g ^ ((fr >> 2) & 3)) << 4);
  const int wsoff = kWsOff<WF> + wave * 256 + fr * 4 + g;       // MXFP4
  const int asoff = kAsOff<WF> + wc * 64 + fr * 4;

  // fp8: the row scales of the lane's output columns n0 + 64 wr + 16 a + 4 g + i, once
  f32x4 rs[4];
  if constexpr (WF == kExpertFp8) {
    const float* se = static_cast<const float*>(wscale) + (size_t)e * N + n0 + 64 * wr + 4 * g;
#pragma unroll
    for (int a = 0; a < 4; ++a) rs[a] = *reinterpret_cast<const f32x4*>(se + 16 * a);
  }
  // block-scaled fp8: group (n0 + 64 wr) / 16 + a of expert e, k-step t.  The same address in
  // every lane; the zero offset is kept in a vector register so that the loads count on vmcnt
  // with the DMA and are covered by the loop's one wait
  const float* bsp = nullptr;
  float bs[4], bn[4];
  if constexpr (WF == kExpertFp8Block) {
    int lane0 = 0;
    asm volatile("" : "+v"(lane0));
    bsp = static_cast<const float*>(wscale) +
          ((size_t)e * (N / kGroup) + (n0 + 64 * wr) / kGroup) * (size_t)kt + lane0;
  }
  auto scales = [&](int t, float (&s)[4]) {
#pragma unroll
    for (int a = 0; a < 4; ++a) s[a] = bsp[(size_t)a * kt + t];
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  if constexpr (WF == kExpertFp8Block) scales(0, bn);
  stage(0, 0);
  for (int t = 0; t < kt; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();   // k-step t has landed for every wave; nobody still reads the other buffer
    if constexpr (WF == kExpertFp8Block) {
#pragma unroll
      for (int a = 0; a < 4; ++a) bs[a] = bn[a];
    }
    if (t + 1 < kt) {
      if constexpr (WF == kExpertFp8Block) scales(t + 1, bn);
      stage(t + 1, (t + 1) & 1);
    }
    asm volatile("" ::: "memory");
    const char* buf = smem + (t & 1) * kBuf;
    i32x4 wf[4][kWk], xf[4][2];
    int wsb[4] = {127, 127, 127, 127};   // MXFP4: the e8m0 byte of fragment row f; fp8: 2^0
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        if (kk < kWk)
          wf[f][kk] = *reinterpret_cast<const i32x4*>(buf + woff[kk] + f * 16 * (kMx ? 64 : 128));
        if (kMx && kk == 0)
          wsb[f] = *reinterpret_cast<const uint8_t*>(smem + wsoff + (t & 1) * kWsBuf<WF> + f * 64);
        xf[f][kk] = *reinterpret_cast<const i32x4*>(buf + xoff[kk] + f * 16 * 128);
      }
    const int as = *reinterpret_cast<const int*>(smem + asoff + t * kTM);
    // the four MFMAs of A fragment a: d[b] = W_a . X_b + c[b]
    auto mfma4 = [&](int a, const f32x4* c, f32x4* d) {
      d[0] = mfma_scaled<WF, 0>(wf[a], wsb[a], xf[0], c[0], as);
      d[1] = mfma_scaled<WF, 1>(wf[a], wsb[a], xf[1], c[1], as);
      d[2] = mfma_scaled<WF, 2>(wf[a], wsb[a], xf[2], c[2], as);
      d[3] = mfma_scaled<WF, 3>(wf[a], wsb[a], xf[3], c[3], as);
    };
    if constexpr (WF == kExpertFp8Block) {
      const f32x4 zero[4] = {};
      f32x4 st[2][4];
#pragma unroll
      for (int a = 0; a <= 4; ++a) {
        if (a < 4) mfma4(a, zero, st[a & 1]);
        if (a > 0) {
#pragma unroll
          for (int b = 0; b < 4; ++b) fold(acc[a - 1][b], bs[a - 1], st[(a - 1) & 1][b]);
        }
      }
    } else {
#pragma unroll
      for (int a = 0; a < 4; ++a) mfma4(a, acc[a], acc[a]);
    }
    asm volatile("" ::: "memory");   // the next DMA into this buffer stays behind its reads
  }

  // fp8: times the row scale of n in fp32, before any rounding
  if constexpr (WF == kExpertFp8) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[a][b][i] *= rs[a][i];
  }
  moe_tile_epilogue<EPI>(acc, out, pairs, rows, start, P, N, n0, wr, wc, fr, g);
}

template <int WF>
void launch_scaled(bf16* out, const uint8_t* a_q, const uint8_t* a_sc, ExpertW W,
                   const int* sorted_pairs, const int* expert_count, const int* expert_offset,
                   int T, int E, int k, int N, int K, int epilogue, hipStream_t stream) {
  const dim3 grid(N / kTN, moe_tile_gemm_capacity(T, E, k));
  const uint8_t* w = static_cast<const uint8_t*>(W.w);
  if (epilogue == kMoeGateUp)
    moe_tile_scaled_kernel<kMoeGateUp, WF><<<grid, kThreads, 0, stream>>>(
        a_q, a_sc, w, W.scale, out, sorted_pairs, expert_count, expert_offset, E, k, T * k, N, K);
  else
    moe_tile_scaled_kernel<kMoeDown, WF><<<grid, kThreads, 0, stream>>>(
        a_q, a_sc, w, W.scale, out, sorted_pairs, expert_count, expert_offset, E, k, T * k, N, K);
}

}  // namespace

int moe_tile_scaled_max_k() { return kMaxKt * kBK; }

int launch_moe_tile_gemm_scaled(bf16* out, const uint8_t* a_q, const uint8_t* a_sc, ExpertW W,
                                const int* sorted_pairs, const int* expert_count,
                                const int* expert_offset, int T, int E, int k, int N, int K,
                                int epilogue, hipStream_t stream) {
  if (W.format != kExpertFp4 && W.format != kExpertFp8 && W.format != kExpertFp8Block) return -6;
  const int rc = moe_tile_check_args(
      T, E, k, N, K, kBK, kMaxKt * kBK, epilogue,
      out != nullptr && a_q != nullptr && a_sc != nullptr && W.w != nullptr &&
          W.scale != nullptr && sorted_pairs != nullptr && expert_count != nullptr &&
          expert_offset != nullptr);
  if (rc != 0) return rc;
  auto launch = W.format == kExpertFp4   ? launch_scaled<kExpertFp4>
                : W.format == kExpertFp8 ? launch_scaled<kExpertFp8>
                                         : launch_scaled<kExpertFp8Block>;
  launch(out, a_q, a_sc, W, sorted_pairs, expert_count, expert_offset, T, E, k, N, K, epilogue,
         stream);
  return 0;
}

}  // namespace dli
