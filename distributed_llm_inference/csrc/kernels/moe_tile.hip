// Sparse mixture-of-experts MLP, experts with many rows: a grouped MFMA tile GEMM over the routed
// experts' bf16 weights.  moe.hip's grouped kernel streams an expert's weights once per tile of
// <= 32 rows, which is the right shape for decode rows and the wrong one once an expert has
// hundreds (prefill chunks, Mixtral at a 512-sequence micro-batch): here a workgroup multiplies a
// tile of <= 128 rows of sorted_pairs with 128 weight rows of the tile's expert, both operands
// staged in LDS, so a weight byte is read once per 128 rows.
//
//   * grid (N / 128, min(E, P) + P / 128), fixed by (T, E, k, N) alone; workgroup (nb, tile).
//     The 128-row tiles are not in the routing tables (those stay moe_group's 32-row tiles): every
//     wave derives its tile from expert_count in a prologue of its own -- lane l holds experts
//     4 l .. 4 l + 3 (E <= 256), the tiles ceil(count / 128) of the lanes are prefix-summed across
//     the wave, and the one lane whose range holds the tile index finds the expert and the tile's
//     number inside it.  A tile index past the sum returns before any DMA or barrier.  Every value
//     is clamped before it forms an address (counts into [0, P], expert into [0, E), rows into
//     [1, 128], start + rows <= P, pair < P hence token < T).
//   * 4 waves as 2 (weight rows) x 2 (activation rows), 64 x 64 per wave = 4 x 4 fragments of
//     v_mfma_f32_16x16x32_bf16 with the weight as the A operand (the accumulator holds the tile
//     transposed: a lane owns 4 consecutive output columns of one row).
//   * k-step of 64 (128 bytes of every row).  Both operand tiles [128 rows][128 B] are staged by
//     16-byte LDS-DMA, lane-linear in LDS; 16-byte chunk c of row r sits in slot c ^ ((r >> 1) & 7)
//     -- gemm_tile.hip's swizzle, applied to the per-lane source address -- so the fragment
//     ds_read_b128s are conflict-free.  The activation rows are gathered: the source address is
//     per lane already, so a gathered row is only a different pointer.  Image rows past the
//     tile's count repeat its last row (loaded in bounds, computed, never stored).
//   * two LDS buffers of 32 KB (weight | activation tile), one barrier per k-step:
//         wait for k-step t's DMA, barrier; send k-step t + 1 into the other buffer; multiply t
//     the barrier also says that every wave is done reading the other buffer (k-step t - 1).  Any
//     number of k-steps >= 1 (K % 64 == 0).  Two workgroups per CU overlap one's wait with the
//     other's MFMAs.
//   * epilogue 0 (gate|up): gate and up of an output column are 16 rows apart inside every
//     aligned 32-row block of the swiglu_interleave'd weight, i.e. A fragments 2 p and 2 p + 1 of
//     a wave: the lane holds both; gate and up rounded to bf16, silu(gate) * up in fp32, rounded;
//     h[start + r, I].  epilogue 1 (down): row r goes to y[sorted_pairs[start + r], H].
//   * no atomics; a row's result depends on that row and its expert only (the k order is fixed).
//
// Quantised experts (WF = kTileFp8, kTileFp4) keep all of the above -- grid, prologue, the
// gathered bf16 activation tile and its swizzle, the wave layout, the MFMAs and their order, one
// barrier per k-step, both epilogues -- and change the weight operand alone: the quantised bytes
// are what the LDS-DMA stages, and a lane widens its A fragment to bf16 in registers when it reads
// it (fp8x8_to_bf16x8 / fp4x8_to_bf16x8: exact).  A lane's fragment of MFMA kk holds the same
// k = 64 t + 32 kk + 8 g .. + 7 of its weight row as in the bf16 kernel, so the products and the
// order they are summed in are the bf16 kernel's on the widened weights.  The activations are
// never quantised.
//   * fp8 (W8 [E, N, K] e4m3fn bytes, w_scale [E, N] fp32): a k-step stages [128 rows][64 B] in
//     two DMA rounds (thread: row 64 j + (tid >> 2), 16-byte slot tid & 3).  The fragment is the 8
//     bytes 32 kk + 8 g .. + 7 of the row, one ds_read_b64.  That instruction is served in two
//     halves of 32 lanes (fr 0 .. 15 x two values of g) over 64 banks = four 64-byte rows: lane-
//     linear, rows fr, fr + 4, fr + 8, fr + 12 meet on the same 16 bytes (4-way).  16-byte chunk c
//     of row r therefore sits in slot c ^ ((r >> 2) & 3) ^ ((r >> 4) & 3): the four rows take the
//     four slots, and the two g of a half the two 8-byte halves of a slot -- every bank once.  The
//     second term is the fragment number f, constant within one read: with it the reads of two
//     fragments are no longer a compile-time constant apart, which keeps the compiler from fusing
//     them into ds_read2st64_b64 (half the rate, 32 banks, 2-way on this image).  The row scale
//     multiplies the fp32 accumulator in the epilogue, gate and up each by their own row's before
//     their bf16 rounding, down before its one rounding (moe.hip's order).
//   * MXFP4 (W4 [E, N, K / 2] nibbles, bscale [E, N, K / 32] e8m0 bytes; K % 128 == 0): a k-step
//     stages [128 rows][32 B] in one DMA round (thread: row tid >> 1, slot tid & 1).  The fragment
//     is the dword 4 kk + g of the row's 8, one ds_read_b32 (32 banks = four rows per half).  The
//     16 rows of a half read two dwords of one 16-byte chunk each, 32 dwords on the 16 banks that
//     8 chunks x 2 dwords can reach whatever the placement of the chunks: 2-way is this
//     fragment's floor.  Chunk c of row r sits in slot c ^ ((r >> 2) & 1), which reaches it
//     (lane-linear: 4-way).  The block scale of (row, k-step t, MFMA kk) is bscale[row][2 t + kk].
//     A lane keeps the four bytes of a pair of k-steps (2 u, 2 u + 1) of each of its four
//     fragment rows in a register: one 4-byte vector load per row and pair (K % 128 == 0, so the
//     k-steps come in pairs and the dword is aligned), issued behind the DMA that an even k-step
//     sends and covered by the loop's vmcnt(0) twice before its first use.  (One 2-byte load per
//     row and k-step instead measured 1.13-1.30x slower at 8-2048 rows per expert: a load that
//     touches 16 rows costs the address unit about what a 1 KB DMA does, so four per wave and
//     k-step nearly doubled its work, which at 128-row tiles is level with the MFMAs'.)  The
//     scale is spent in the widening (2^(byte - 127), exact): nothing is left for the epilogue.
//   * LDS per buffer: 8 + 16 KB (fp8), 4 + 16 KB (MXFP4), against 16 + 16 KB.
#include "kernels.h"

namespace dli {

namespace {

constexpr int kMaxExperts = 256;
constexpr int kMaxTopK = 8;
constexpr int kTM = 128;          // activation rows per tile
constexpr int kTN = 128;          // weight rows per workgroup
constexpr int kBK = 64;           // k per step
constexpr int kThreads = 256;
constexpr int kOp = 128 * 128;    // bytes of one staged operand tile

enum MoeEp { kMoeGateUp = 0, kMoeDown = 1 };
enum TileWf { kTileBf16 = 0, kTileFp8 = 1, kTileFp4 = 2 };

// bytes of one staged weight tile (128 rows of one k-step) and of one buffer (weight | activation)
template <int WF> constexpr int kWOp = WF == kTileBf16 ? kOp : WF == kTileFp8 ? kOp / 2 : kOp / 4;
template <int WF> constexpr int kBufOf = kWOp<WF> + kOp;

// W: the experts' [E, N, K] bf16, [E, N, K] e4m3 bytes (wscale: [E, N] fp32 row scales) or
// [E, N, K / 2] MXFP4 bytes (wscale: [E, N, K / 32] e8m0 block scales)
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
  } else if constexpr (WF == kTileFp8) {
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
    } else if constexpr (WF == kTileFp8) {
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
      if constexpr (WF == kTileFp8)
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

  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

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
    asm volatile("" ::: "memory");
    const char* buf = smem + (t & 1) * kBuf;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        if constexpr (WF == kTileBf16) {
          af[f] = *reinterpret_cast<const bf16x8*>(buf + aoff + f * 2048 + foff[kk]);
        } else if constexpr (WF == kTileFp8) {
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
        for (int b = 0; b < 4; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[a], bfr[b], acc[a][b], 0, 0, 0);
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

int moe_tile_gemm_capacity(int T, int E, int k) {
  const long P = (long)T * k;
  return (int)((E < P ? E : P) + P / kTM);
}

namespace {

template <int WF>
int launch_tile(bf16* out, const bf16* x, const void* W, const void* wscale,
                const int* sorted_pairs, const int* expert_count, const int* expert_offset, int T,
                int E, int k, int N, int K, int epilogue, hipStream_t stream) {
  if (T <= 0 || E <= 0 || E > kMaxExperts || k <= 0 || k > kMaxTopK) return -1;
  if (N <= 0 || N % kTN != 0 || K <= 0 || K % kBK != 0) return -2;
  if (WF == kTileFp4 && K % 128 != 0) return -2;
  if ((long)T * k > (1L << 30)) return -3;
  const int cap = moe_tile_gemm_capacity(T, E, k);
  if (cap <= 0 || cap > 65535) return -3;
  if (out == nullptr || x == nullptr || W == nullptr || sorted_pairs == nullptr ||
      expert_count == nullptr || expert_offset == nullptr)
    return -5;
  if (WF != kTileBf16 && wscale == nullptr) return -5;
  const dim3 grid(N / kTN, cap);
  const int P = T * k;
  if (epilogue == kMoeGateUp)
    moe_tile_gemm_kernel<kMoeGateUp, WF><<<grid, kThreads, 0, stream>>>(
        x, W, out, sorted_pairs, expert_count, expert_offset, E, k, P, N, K, wscale);
  else if (epilogue == kMoeDown)
    moe_tile_gemm_kernel<kMoeDown, WF><<<grid, kThreads, 0, stream>>>(
        x, W, out, sorted_pairs, expert_count, expert_offset, E, k, P, N, K, wscale);
  else
    return -4;
  return 0;
}

}  // namespace

int launch_moe_tile_gemm(bf16* out, const bf16* x, ExpertW W, const int* sorted_pairs,
                         const int* expert_count, const int* expert_offset, int T, int E, int k,
                         int N, int K, int epilogue, hipStream_t stream) {
  static_assert(kTileBf16 == kExpertBf16 && kTileFp8 == kExpertFp8 && kTileFp4 == kExpertFp4);
  switch (W.format) {
    case kExpertBf16:
      return launch_tile<kTileBf16>(out, x, W.w, nullptr, sorted_pairs, expert_count,
                                    expert_offset, T, E, k, N, K, epilogue, stream);
    case kExpertFp8:
      return launch_tile<kTileFp8>(out, x, W.w, W.scale, sorted_pairs, expert_count,
                                   expert_offset, T, E, k, N, K, epilogue, stream);
    case kExpertFp4:
      return launch_tile<kTileFp4>(out, x, W.w, W.scale, sorted_pairs, expert_count,
                                   expert_offset, T, E, k, N, K, epilogue, stream);
  }
  return -6;
}

}  // namespace dli
