// Sparse mixture-of-experts MLP, block-scaled fp8 experts with many rows, on the block-scaled MFMA
// with both operands fp8: the two products of moe_tile.hip (gate|up + SwiGLU, down + scatter) with
// the stored e4m3 weight bytes and MX fp8 activations multiplied by
// v_mfma_scale_f32_16x16x128_f8f6f4.  Nothing is widened to bf16.  The weight's fp32 block scale
// cannot ride on the instruction's e8m0 scale operand and does not have to: one instruction
// consumes exactly one 128-k block, an A fragment is exactly one 16-row scale group, so the scale
// is constant over a whole instruction.  Every MFMA starts from a zero C operand and its result
// is folded into the running accumulator by one FMA per element, acc = fma(scale, step, acc).
//
//   W  = the experts as moe_tile_fp8_block.hip reads them, neither tensor re-laid-out: e4m3fn
//        bytes [E, N, K] in stored row order, scale [E, N / 16, K / 128] fp32 (one per 16 stored
//        rows and 128 k);
//   A  = e4m3 bytes [R, K] with ROW-MAJOR e8m0 scales [R, K / 128] (quant.hip
//        launch_quant_mx_rows), gathered as in moe_tile_f8.hip: gate|up reads token
//        sorted_pairs[start + r] / k of x quantised once per token, down reads row start + r of h
//        quantised in its sorted order.
//
//   * grid, prologue, clamps, guards, LDS layout, staging and fragment reads: moe_tile_f8.hip's,
//     unchanged.  Grid (N / 128, min(E, P) + P / 128), fixed by (T, E, k, N); every wave derives
//     its tile from expert_count / expert_offset (wave prefix sum over ceil(count / 128)); a tile
//     index past the sum returns before any DMA, LDS write or barrier.  Counts are clamped into
//     [0, P], the expert into [0, E), rows into [1, 128], start + rows <= P, pair < P hence
//     token < T.  Image rows past the tile's count repeat its last row (loaded in bounds,
//     computed, never stored).  No atomics, no host sync; a row's result depends on that row and
//     its expert only.
//   * 4 waves as 2 (weight rows) x 2 (activation rows), 64 x 64 per wave = 4 x 4 fragments.  The
//     weight is the A operand, so a lane owns 4 consecutive output columns of one row; gate / up
//     are A fragments 2 p, 2 p + 1.  The weight's scale operand is the constant 127 (2^0); the
//     activation's e8m0 byte is byte b of the B scale dword, picked by op_sel.
//   * the k-step: 16 MFMAs with a zero C operand, mutually independent (no accumulator chain),
//     and 64 scalar-by-vector FMAs.  They are written one A fragment apart -- the four MFMAs of
//     fragment a + 1, then the sixteen FMAs of fragment a -- so the FMAs issue while the matrix
//     pipe works on the next fragment and never wait on the instruction just issued.
//   * weight scales: a wave needs the 4 fp32 of groups (n0 + 64 wr) / 16 + a at k-step t
//     (in bounds: N % 128 == 0, t < K / 128).  They are loaded one k-step ahead, next to that
//     step's DMA issue, by plain wave-uniform vector loads that the loop's vmcnt(0) wait covers
//     together with the DMA.  No LDS slot.  File compiled without packed fp32 instructions: the
//     FMAs are v_fma_f32 / v_fmac_f32.
//   * epilogue: nothing is left to scale.  Gate and up are each rounded to bf16, then
//     silu(gate) * up; down is rounded once and scattered to row sorted_pairs[j].
//   * activation scales: as moe_tile_f8.hip, the tile's [K / 128][128 rows] bytes staged in LDS
//     once in the prologue, transposed into the MFMA's order.  The slot bounds the supported K:
//     K / 128 <= 128 k-steps, K <= 16384.
//   * LDS: 2 x 32 KB + 16 KB = 80 KB, half a CU's 160 KB: two workgroups per CU.  Compiler's
//     resource summary, both instantiations: 187 VGPRs, no AGPRs, no scratch, 81920 bytes of LDS,
//     2 waves per SIMD.
#include "kernels.h"

namespace dli {

namespace {

constexpr int kMaxExperts = 256;
constexpr int kMaxTopK = 8;
constexpr int kTM = 128;               // activation rows per tile
constexpr int kTN = 128;               // weight rows per workgroup
constexpr int kBK = 128;               // k per step = one MFMA = one scale block
constexpr int kGroup = 16;             // weight rows per scale group = one A fragment
constexpr int kThreads = 256;
constexpr int kOp = kTM * kBK;         // 16 KB of e4m3, either operand
constexpr int kBuf = 2 * kOp;          // weight tile, then activation tile
constexpr int kMaxKt = 128;            // k-steps of activation scales a workgroup keeps (16 KB)
constexpr int kAsOff = 2 * kBuf;
constexpr int kLds = kAsOff + kMaxKt * kTM;

enum MoeEp { kMoeGateUp = 0, kMoeDown = 1 };

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

// one 128-k block of e4m3 (A operand) x e4m3 (B operand) from a zero accumulator.  The weight's
// scale operand is 2^0; byte SEL of `asc` scales the lane's 32 activation values
template <int SEL>
__device__ __forceinline__ f32x4 mfma_step(const i32x4& w0, const i32x4& w1, const i32x4& a0,
                                           const i32x4& a1, int asc) {
  const i32x8 a = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3]};
  const i32x8 b = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, z, 0, 0, 0, 127, SEL, asc);
}

__device__ __forceinline__ void fold(f32x4& acc, float s, const f32x4& step) {
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = __builtin_fmaf(s, step[i], acc[i]);
}

template <int EPI>
__global__ void __launch_bounds__(kThreads, 2)
moe_tile_f8_block_kernel(const uint8_t* __restrict__ aq, const uint8_t* __restrict__ asc,
                         const uint8_t* __restrict__ W, const float* __restrict__ wscale,
                         bf16* __restrict__ out, const int* __restrict__ sorted_pairs,
                         const int* __restrict__ expert_count,
                         const int* __restrict__ expert_offset, int E, int topk, int P, int N,
                         int K) {
  __shared__ __attribute__((aligned(1024))) char smem[kLds];
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
    char* d = smem + kAsOff + (r >> 6) * 64 + (r & 15) * 4 + ((r >> 4) & 3);
    for (int t = tid >> 7; t < kt; t += 2) d[t * kTM] = (char)s[t];
  }

  // ---- staging: round j fills image rows 32 j .. 32 j + 31 of either operand (thread: row
  // 32 j + (tid >> 3), slot tid & 7); the chunk that belongs in that slot is the same every round
  const int srow = tid >> 3;
  const int chunk = (tid & 7) ^ ((srow >> 1) & 7);
  const uint8_t* wsrc = W + ((size_t)e * N + n0 + srow) * (size_t)K + chunk * 16;
  const uint8_t* xsrc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) xsrc[j] = aq + src_row(32 * j + srow) * (size_t)K + chunk * 16;
  auto stage = [&](int t, int buf) {
    char* dst = smem + buf * kBuf + wave * 1024;
#pragma unroll
    for (int j = 0; j < 4; ++j) glds16(wsrc + (size_t)j * 32 * K + (size_t)t * kBK, dst + j * 4096);
#pragma unroll
    for (int j = 0; j < 4; ++j) glds16(xsrc[j] + (size_t)t * kBK, dst + kOp + j * 4096);
  };

  // ---- fragments: chunks g, g + 4 of weight row 16 a + fr and of activation row 16 b + fr of
  // the wave's 64 x 64 (the multiples of 16 leave the swizzle alone) ----
  const int wr = wave >> 1, wc = wave & 1, fr = lane & 15, g = lane >> 4;
  int woff[2], xoff[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    const int c = ((4 * kk + g) ^ ((fr >> 1) & 7)) << 4;
    woff[kk] = (64 * wr + fr) * 128 + c;
    xoff[kk] = kOp + (64 * wc + fr) * 128 + c;
  }
  const int asoff = kAsOff + wc * 64 + fr * 4;

  // ---- weight scales: group (n0 + 64 wr) / 16 + a of expert e, k-step t.  The same address in
  // every lane; the zero offset is kept in a vector register so that the loads count on vmcnt
  // with the DMA and are covered by the loop's one wait
  int lane0 = 0;
  asm volatile("" : "+v"(lane0));
  const float* wsp = wscale + ((size_t)e * (N / kGroup) + (n0 + 64 * wr) / kGroup) * (size_t)kt + lane0;
  auto scales = [&](int t, float (&s)[4]) {
#pragma unroll
    for (int a = 0; a < 4; ++a) s[a] = wsp[(size_t)a * kt + t];
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  float ws[4], wn[4];
  scales(0, wn);
  stage(0, 0);
  for (int t = 0; t < kt; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();   // k-step t has landed for every wave; nobody still reads the other buffer
#pragma unroll
    for (int a = 0; a < 4; ++a) ws[a] = wn[a];
    if (t + 1 < kt) {
      scales(t + 1, wn);
      stage(t + 1, (t + 1) & 1);
    }
    asm volatile("" ::: "memory");
    const char* buf = smem + (t & 1) * kBuf;
    i32x4 wf[4][2], xf[4][2];
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        wf[f][kk] = *reinterpret_cast<const i32x4*>(buf + woff[kk] + f * 16 * 128);
        xf[f][kk] = *reinterpret_cast<const i32x4*>(buf + xoff[kk] + f * 16 * 128);
      }
    const int as = *reinterpret_cast<const int*>(smem + asoff + t * kTM);
    f32x4 st[2][4];
#pragma unroll
    for (int a = 0; a <= 4; ++a) {
      if (a < 4) {
        f32x4* s = st[a & 1];
        s[0] = mfma_step<0>(wf[a][0], wf[a][1], xf[0][0], xf[0][1], as);
        s[1] = mfma_step<1>(wf[a][0], wf[a][1], xf[1][0], xf[1][1], as);
        s[2] = mfma_step<2>(wf[a][0], wf[a][1], xf[2][0], xf[2][1], as);
        s[3] = mfma_step<3>(wf[a][0], wf[a][1], xf[3][0], xf[3][1], as);
      }
      if (a > 0) {
        const f32x4* s = st[(a - 1) & 1];
#pragma unroll
        for (int b = 0; b < 4; ++b) fold(acc[a - 1][b], ws[a - 1], s[b]);
      }
    }
    asm volatile("" ::: "memory");   // the next DMA into this buffer stays behind its reads
  }

  // ---- epilogue: acc[a][b][i] = y[m = 64 wc + 16 b + fr][n = n0 + 64 wr + 16 a + 4 g + i],
  // already scaled ----
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

int moe_tile_f8_block_max_k() { return kMaxKt * kBK; }

int launch_moe_tile_gemm_f8_block(bf16* out, const uint8_t* a_q, const uint8_t* a_sc, ExpertW W,
                                  const int* sorted_pairs, const int* expert_count,
                                  const int* expert_offset, int T, int E, int k, int N, int K,
                                  int epilogue, hipStream_t stream) {
  if (W.format != kExpertFp8Block) return -6;
  if (T <= 0 || E <= 0 || E > kMaxExperts || k <= 0 || k > kMaxTopK) return -1;
  if (N <= 0 || N % kTN != 0 || K <= 0 || K % kBK != 0 || K > kMaxKt * kBK) return -2;
  if ((long)T * k > (1L << 30)) return -3;
  const int cap = moe_tile_gemm_capacity(T, E, k);
  if (cap <= 0 || cap > 65535) return -3;
  if (epilogue != kMoeGateUp && epilogue != kMoeDown) return -4;
  if (out == nullptr || a_q == nullptr || a_sc == nullptr || W.w == nullptr ||
      W.scale == nullptr || sorted_pairs == nullptr || expert_count == nullptr ||
      expert_offset == nullptr)
    return -5;
  const dim3 grid(N / kTN, cap);
  const int P = T * k;
  const uint8_t* w = static_cast<const uint8_t*>(W.w);
  const float* ws = static_cast<const float*>(W.scale);
  if (epilogue == kMoeGateUp)
    moe_tile_f8_block_kernel<kMoeGateUp><<<grid, kThreads, 0, stream>>>(
        a_q, a_sc, w, ws, out, sorted_pairs, expert_count, expert_offset, E, k, P, N, K);
  else
    moe_tile_f8_block_kernel<kMoeDown><<<grid, kThreads, 0, stream>>>(
        a_q, a_sc, w, ws, out, sorted_pairs, expert_count, expert_offset, E, k, P, N, K);
  return 0;
}

}  // namespace dli
