// Sparse mixture-of-experts MLP, MXFP4 experts with many rows, on the block-scaled MFMA: the two
// products of moe_tile.hip (gate|up + SwiGLU, down + scatter) with the weight nibbles and MX fp8
// activations multiplied by v_mfma_scale_f32_16x16x128_f8f6f4 as they are stored.  Both scale sets
// (e8m0 per 32 k of a weight row, e8m0 per 128 k of an activation row) go to the instruction's
// per-lane scale operands, so the fp32 accumulator holds the finished product: nothing is widened,
// no operand is dequantised, the epilogue scales nothing.
//
//   W  = the experts as moe_tile.hip's MXFP4 kernel reads them: nibbles [E, N, K / 2] (element 2 j
//        in the low nibble of byte j), bscale [E, N, K / 32] e8m0 bytes;
//   A  = e4m3 bytes [R, K] with ROW-MAJOR e8m0 scales [R, K / 128] (quant.hip
//        launch_quant_mx_rows).  The rows of a tile are gathered (gate|up: token
//        sorted_pairs[start + r] / k of x quantised once per token; down: row start + r of h
//        quantised in its sorted order), so mx_off's packing of four contiguous rows per dword
//        does not apply; row-major lets a gathered row bring its scales with it.
//
//   * grid, prologue, clamps: moe_tile.hip's, unchanged.  Grid (N / 128, min(E, P) + P / 128),
//     fixed by (T, E, k, N); every wave derives its tile from expert_count / expert_offset (lane l
//     holds experts 4 l .. 4 l + 3, wave prefix sum over ceil(count / 128)); a tile index past
//     the sum returns before any DMA, LDS write or barrier.  Counts are clamped into [0, P], the
//     expert into [0, E), rows into [1, 128], start + rows <= P, pair < P hence token < T.  Image
//     rows past the tile's count repeat its last row (bytes and scales; loaded in bounds,
//     computed, never stored).  No atomics, no host sync; a row's result depends on that row and
//     its expert only.
//   * 4 waves as 2 (weight rows) x 2 (activation rows), 64 x 64 per wave = 4 x 4 fragments.  A
//     k-step is 128 k = one MFMA per fragment pair: 16 MFMAs per wave and k-step (the bf16 loop
//     issues 64 for the same k).  The weight is the A operand (cbsz = 4, its four dwords in the
//     low half of the operand), so a lane owns 4 consecutive output columns of one row and both
//     epilogues are moe_tile.hip's: gate / up are A fragments 2 p, 2 p + 1.
//   * k order inside the step, as gemm_fp4.hip's header records it: the fp4 operand's lane group
//     g = lane >> 4 holds k = 32 g .. 32 g + 31, which is the 16-byte chunk g of the step's
//     64-byte weight row, and its scale byte is byte g of the (row, k-step) scale dword; the fp8
//     operand's lane group g holds the 16-byte chunks g and g + 4 of the 128-byte activation row.
//   * LDS per buffer: weight [128][64 B] = 8 KB (two DMA rounds; thread: row 64 j + (tid >> 2),
//     slot tid & 3, chunk slot ^ ((row >> 2) & 3)) and activations [128][128 B] = 16 KB (four
//     rounds; thread: row 32 j + (tid >> 3), slot tid & 7, chunk slot ^ ((row >> 1) & 7)), both
//     lane-linear 16-byte LDS-DMA with the swizzle in the source address -- gemm_fp4.hip's two
//     layouts, whose ds_read_b128 fragment reads touch every bank once.  Two buffers, one barrier
//     per k-step:  wait for step t's DMA, barrier; send step t + 1 into the other buffer;
//     multiply t.  Any number of k-steps >= 1.
//   * weight scales: a small per-wave LDS slot, as gemm_fp4.hip.  Each wave sends the step's scale
//     dwords of its own 64 weight rows (lane l: row n0 + 64 wr + l) with ONE 4-byte LDS-DMA next
//     to the operand DMAs, into a slot of the buffer that only it reads (256 B per wave and
//     buffer), and reads byte g of its four fragment rows with ds_read_u8.  Chosen over registers
//     a step ahead because that takes four narrow loads per wave and k-step, each touching 16
//     rows -- the pattern that made the first MXFP4 tile kernel 1.13-1.30x slower (moe_tile.hip's
//     header) -- where the DMA is one instruction touching 64 rows, retired by the vmcnt(0) the
//     loop already has.
//   * activation scales: the tile's [K / 128][128 rows] bytes are staged in LDS once, in the
//     prologue, by plain loads before any DMA is in flight (thread: image row tid & 127, k-steps
//     of parity tid >> 7), transposed into the MFMA's order: the dword of (k-step t, wave column
//     wc, fr) holds image rows 64 wc + fr + 16 b in byte b, so a lane reads one dword per k-step
//     and the op_sel immediate b picks the fragment's row.  The slot bounds the supported K:
//     K / 128 <= 128 k-steps, K <= 16384 (16 KB), which covers Qwen3-30B-A3B (2048 / 768),
//     Mixtral-8x7B (4096 / 14336) and Qwen2-MoE (I = 1408, 2560).
//   * LDS: 2 x 24 KB + 2 KB + 16 KB = 66 KB, two workgroups per CU.
//
// fp8 experts (per-row fp32 scales, which need an epilogue scale) are not taken here.
#include "kernels.h"

namespace dli {

namespace {

constexpr int kMaxExperts = 256;
constexpr int kMaxTopK = 8;
constexpr int kTM = 128;               // activation rows per tile
constexpr int kTN = 128;               // weight rows per workgroup
constexpr int kBK = 128;               // k per step = one MFMA
constexpr int kThreads = 256;
constexpr int kWOp = kTN * kBK / 2;    // 8 KB of nibbles
constexpr int kAOp = kTM * kBK;        // 16 KB of e4m3
constexpr int kBuf = kWOp + kAOp;
constexpr int kWsBuf = 4 * 256;        // weight scales: [wave][64 rows] dwords, per buffer
constexpr int kMaxKt = 128;            // k-steps of activation scales a workgroup keeps
constexpr int kWsOff = 2 * kBuf, kAsOff = kWsOff + 2 * kWsBuf;

enum MoeEp { kMoeGateUp = 0, kMoeDown = 1 };

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

// e2m1 (A operand, cbsz = 4: the first four operand dwords) x e4m3 (B operand, blgp = 0), K = 128.
// Byte 0 of `wsc` scales the lane's 32 weight values, byte SEL of `asc` its 32 activation values
template <int SEL>
__device__ __forceinline__ f32x4 mfma_w4(const i32x4& w, int wsc, const i32x4& a0, const i32x4& a1,
                                         const f32x4& c, int asc) {
  const i32x8 a = {w[0], w[1], w[2], w[3], 0, 0, 0, 0};
  const i32x8 b = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 4, 0, 0, wsc, SEL, asc);
}

template <int EPI>
__global__ void __launch_bounds__(kThreads, 2)
moe_tile_mx_kernel(const uint8_t* __restrict__ aq, const uint8_t* __restrict__ asc,
                   const uint8_t* __restrict__ W, const uint8_t* __restrict__ bscale,
                   bf16* __restrict__ out, const int* __restrict__ sorted_pairs,
                   const int* __restrict__ expert_count, const int* __restrict__ expert_offset,
                   int E, int topk, int P, int N, int K) {
  __shared__ __attribute__((aligned(1024))) char smem[kAsOff + kMaxKt * kTM];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = blockIdx.y, nb = blockIdx.x;

  // ---- which expert, which rows: the wave's prefix sum over ceil(count / 128) ----
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
  if (tile >= __shfl(incl, 63, 64)) return;   // before any DMA or barrier; the same in every wave
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
  const int e = min(max(__builtin_amdgcn_readlane(e_l, owner), 0), E - 1);
  const int ti = max(__builtin_amdgcn_readlane(rem, owner), 0);
  const int ce = __builtin_amdgcn_readlane(c_l, owner);
  const int rows = min(max(ce - kTM * ti, 1), min(kTM, P));
  const int start = min(max(expert_offset[e] + kTM * ti, 0), P - rows);
  const int* pairs = sorted_pairs + start;
  const int n0 = nb * kTN;
  const int kt = K / kBK;
  const size_t Kw = (size_t)K >> 1, Ks = (size_t)K >> 5, Ka = (size_t)K >> 7;

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
    char* d = smem + kAsOff + (r >> 6) * 64 + (r & 15) * 4 + ((r >> 4) & 3);
    for (int t = tid >> 7; t < kt; t += 2) d[t * kTM] = (char)s[t];
  }

  // ---- staging ----
  // weight: round j fills image rows 64 j .. 64 j + 63 (thread: row 64 j + (tid >> 2), slot tid & 3)
  const int qrow = tid >> 2;
  const uint8_t* wsrc = W + ((size_t)e * N + n0 + qrow) * Kw + (((tid & 3) ^ ((qrow >> 2) & 3)) << 4);
  // activations: round j fills image rows 32 j .. 32 j + 31 (thread: row 32 j + (tid >> 3), slot
  // tid & 7); the chunk that belongs in that slot is the same every round
  const int srow = tid >> 3;
  const int chunk = (tid & 7) ^ ((srow >> 1) & 7);
  const uint8_t* xsrc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) xsrc[j] = aq + src_row(32 * j + srow) * (size_t)K + chunk * 16;
  // weight scales: the dword of (row n0 + 64 wr + lane, k-step) into the wave's own slot
  const int wr = wave >> 1, wc = wave & 1, fr = lane & 15, g = lane >> 4;
  const uint8_t* ssrc = bscale + ((size_t)e * N + n0 + 64 * wr + lane) * Ks;
  auto stage = [&](int t, int buf) {
    char* dst = smem + buf * kBuf + wave * 1024;
#pragma unroll
    for (int j = 0; j < 2; ++j) glds16(wsrc + (size_t)j * 64 * Kw + (size_t)t * (kBK / 2), dst + j * 4096);
#pragma unroll
    for (int j = 0; j < 4; ++j) glds16(xsrc[j] + (size_t)t * kBK, dst + kWOp + j * 4096);
    __builtin_amdgcn_global_load_lds((gbl_void*)(ssrc + (size_t)t * 4),
                                     (lds_void*)(smem + kWsOff + buf * kWsBuf + wave * 256), 4, 0,
                                     0);
  };

  // ---- fragments: weight chunk g of row 16 a + fr, activation chunks g, g + 4 of row 16 b + fr
  // of the wave's 64 x 64 (the multiples of 16 leave both swizzles alone) ----
  const int woff = (64 * wr + fr) * 64 + ((g ^ ((fr >> 2) & 3)) << 4);
  int xoff[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk)
    xoff[kk] = kWOp + (64 * wc + fr) * 128 + (((4 * kk + g) ^ ((fr >> 1) & 7)) << 4);
  const int wsoff = kWsOff + wave * 256 + fr * 4 + g;
  const int asoff = kAsOff + wc * 64 + fr * 4;

  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  stage(0, 0);
  for (int t = 0; t < kt; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();   // k-step t has landed for every wave; nobody still reads the other buffer
    if (t + 1 < kt) stage(t + 1, (t + 1) & 1);
    asm volatile("" ::: "memory");
    const char* buf = smem + (t & 1) * kBuf;
    i32x4 wf[4], xf[4][2];
    int ws[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      wf[f] = *reinterpret_cast<const i32x4*>(buf + woff + f * 16 * 64);
      ws[f] = *reinterpret_cast<const uint8_t*>(smem + wsoff + (t & 1) * kWsBuf + f * 64);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
        xf[f][kk] = *reinterpret_cast<const i32x4*>(buf + xoff[kk] + f * 16 * 128);
    }
    const int as = *reinterpret_cast<const int*>(smem + asoff + t * kTM);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      acc[a][0] = mfma_w4<0>(wf[a], ws[a], xf[0][0], xf[0][1], acc[a][0], as);
      acc[a][1] = mfma_w4<1>(wf[a], ws[a], xf[1][0], xf[1][1], acc[a][1], as);
      acc[a][2] = mfma_w4<2>(wf[a], ws[a], xf[2][0], xf[2][1], acc[a][2], as);
      acc[a][3] = mfma_w4<3>(wf[a], ws[a], xf[3][0], xf[3][1], acc[a][3], as);
    }
    asm volatile("" ::: "memory");   // the next DMA into this buffer stays behind its reads
  }

  // ---- epilogue: acc[a][b][i] = y[m = 64 wc + 16 b + fr][n = n0 + 64 wr + 16 a + 4 g + i] ----
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

}  // namespace

int moe_tile_mx_max_k() { return kMaxKt * kBK; }

int launch_moe_tile_gemm_mx(bf16* out, const uint8_t* a_q, const uint8_t* a_sc, ExpertW W,
                            const int* sorted_pairs, const int* expert_count,
                            const int* expert_offset, int T, int E, int k, int N, int K,
                            int epilogue, hipStream_t stream) {
  if (W.format != kExpertFp4) return -6;
  if (T <= 0 || E <= 0 || E > kMaxExperts || k <= 0 || k > kMaxTopK) return -1;
  if (N <= 0 || N % kTN != 0 || K <= 0 || K % kBK != 0 || K > kMaxKt * kBK) return -2;
  if ((long)T * k > (1L << 30)) return -3;
  const int cap = moe_tile_gemm_capacity(T, E, k);
  if (cap <= 0 || cap > 65535) return -3;
  if (out == nullptr || a_q == nullptr || a_sc == nullptr || W.w == nullptr ||
      W.scale == nullptr || sorted_pairs == nullptr || expert_count == nullptr ||
      expert_offset == nullptr)
    return -5;
  const dim3 grid(N / kTN, cap);
  const int P = T * k;
  const uint8_t* w = static_cast<const uint8_t*>(W.w);
  const uint8_t* ws = static_cast<const uint8_t*>(W.scale);
  if (epilogue == kMoeGateUp)
    moe_tile_mx_kernel<kMoeGateUp><<<grid, kThreads, 0, stream>>>(
        a_q, a_sc, w, ws, out, sorted_pairs, expert_count, expert_offset, E, k, P, N, K);
  else if (epilogue == kMoeDown)
    moe_tile_mx_kernel<kMoeDown><<<grid, kThreads, 0, stream>>>(
        a_q, a_sc, w, ws, out, sorted_pairs, expert_count, expert_offset, E, k, P, N, K);
  else
    return -4;
  return 0;
}

}  // namespace dli
