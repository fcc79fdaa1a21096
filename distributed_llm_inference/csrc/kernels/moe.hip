// Sparse mixture-of-experts MLP (Qwen3-MoE, Mixtral, Qwen2-MoE) with bf16, fp8 (e4m3fn, one fp32 scale per
// weight row) or MXFP4 (e2m1 nibbles, one e8m0 scale per 32 k) expert weights: routing, a grouped
// weight-streaming MFMA GEMM over the hit experts, and the weighted combine.  Every grid is fixed
// by (T, E, k, N) alone and every count is read from device memory, so the launches are
// hipGraph-capturable and the same launches serve 1 decode row, decode batches and prefill chunks.
//
//   * moe_topk (wave per token).  E <= 256 router logits (bf16) per token.  Softmax is monotone,
//     so the top-k of the probabilities is the top-k of the logits: every logit becomes an
//     order-preserving integer key with 255 - index in its low byte, and k wave-wide maxima of
//     that key select the experts -- ties go to the lower index, -0 ranks as +0, a NaN ranks as
//     the greatest value (torch.topk's order).  The weights are softmax probabilities in fp32
//     (exp(l - max) / sum over all E), optionally divided by their top-k sum (slot order), rounded
//     to bf16 and stored as fp32.
//   * moe_group (workgroup per expert).  Scan 1 histograms the [T k] id list in LDS (integer
//     counts: the same whatever order the atomics arrive in); the workgroup of expert e takes its
//     offset and its first tile from the counts of the experts before it.  Scan 2 walks the list in
//     order, 256 pairs at a time, and a block prefix sum of the "is mine" flags gives every pair
//     its slot: sorted_pairs is the stable sort of the pair indices t k + slot by expert.  An
//     expert's range is cut into tiles of <= 32 rows; at most min(E, P) + P / 32 tiles exist.
//     Ids are clamped into [0, E), so the counts always sum to P and nothing is written outside
//     the tables.
//   * moe_grouped_gemm.  The small kernels' product, wstream_core.h's, on the experts' weights
//     (the operand layouts of the three formats, x through LDS, the K split over the 8 waves and
//     the load pipeline are described there).  Grid (N / 32, tile capacity); workgroup (nb, tile)
//     multiplies the <= 32 rows of its tile with rows 32 nb .. 32 nb + 31 of its tile's expert:
//     the weight rows are loaded as they are (N % 32 == 0), the x rows through the tile's table
//     (below; image rows past the tile's count repeat its last row).  A tile index >= n_tiles
//     returns before any DMA or barrier.  1-16 rows use one MFMA B tile, 17-32 two (a
//     workgroup-uniform branch on the table's row count, not a host dispatch).  An expert with
//     more than 32 rows is read once per tile (through L2 / Infinity Cache when its tiles run
//     close together); numbering the workgroups tile-major instead, so that an expert's tiles run
//     side by side, measured no faster (docs/kernels.md).  Epilogues:
//       gate|up: the x rows are gathered -- row r of the tile is token sorted_pairs[start + r] / k
//         (the LDS-DMA source address is per lane already) -- and SwiGLU is applied to
//         swiglu_interleave'd weight rows as in the small kernels: gate and up rounded to bf16,
//         silu(gate) * up in fp32, rounded; h[start + r, I].
//       down: x rows are h[start .. start + rows); row r goes to y[sorted_pairs[start + r], H].
//     Every table value is clamped before it forms an address (expert into [0, E), rows into
//     [1, 32], start + rows <= P, pair < P hence token < T): a garbage table cannot leave the
//     buffers.
//     bf16 weights (WF = kMoeBf16): W [E, N, K].
//     fp8 weights (WF = kMoeFp8: W8 [E, N, K] e4m3fn bytes, w_scale [E, N] fp32): the k order, the
//     wave's steps and the order of the MFMAs are the bf16 variant's.  The activations are never
//     quantised; the scale of weight row n of expert e, w_scale[e N + n], multiplies the fp32
//     accumulator after the K-split sum (gate and up each by their own row's scale before their
//     bf16 rounding).
//     MXFP4 weights (WF = kMoeFp4: W4 [E, N, K / 2] bytes, element 2 j in the low nibble of byte
//     j, bscale [E, N, K / 32] e8m0 bytes): again the k order, the wave's steps and the order of
//     the MFMAs are the bf16 variant's, so the result is the bf16 kernel's on the dequantised
//     weights bit for bit.  The scale is spent in the widening: nothing is left for the epilogue,
//     and the activations are never quantised.
//   * moe_combine.  out[t] = bf16(sum_slot w[t, slot] * y[t k + slot]) in fp32, slot order.
//
// Shared expert (Qwen2-MoE): every token of a sparse layer also runs one dense SwiGLU expert, on
// the dense kernels, whose output s[t] is scaled by sigmoid(shared_expert_gate(x[t])).  The gate
// row is stored behind the E router rows, so the router product hands over logits [T, ld] with
// ld > E: columns 0 .. E - 1 are the router's, column E is the gate's logit, columns past E are
// row padding and are never read.  Two template instantiations, kShared = true, carry it; the
// kShared = false ones are the kernels above, unchanged:
//   * moe_topk<true>: the row stride is ld; lane 0 also loads logits[t, E] and stores
//     shared_w[t] = float(bf16(1 / (1 + exp(-logit)))) -- F.sigmoid of the bf16 logit, rounded
//     to bf16 and held as fp32 like the top-k weights.  The column takes no part in the ranking
//     or in the softmax sum: ids and w are those of the contiguous [:, :E] slice, bit for bit.
//   * moe_combine<true>: out[t] = bf16(sum_slot w[t, slot] * y[t k + slot] + shared_w[t] * s[t]),
//     fp32, the slots in order, then the shared term, then the one rounding; the vector width,
//     the guard and the launch shape are moe_combine<false>'s.
#include "wstream_core.h"

namespace dli {

namespace {

constexpr int kMaxExperts = 256;
constexpr int kMaxTopK = 8;

// ------------------------------------------------------------------------------------- top-k
constexpr int kTopkWaves = 4;

__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
  return v;
}

// kShared: logits rows are ld >= E + 1 apart and column E is the shared expert's gate logit
// (shared_w [T] gets its sigmoid); else ld == E and shared_w is not touched
template <bool kShared>
__global__ void __launch_bounds__(kTopkWaves * 64)
moe_topk_kernel(const bf16* __restrict__ logits, int* __restrict__ ids, float* __restrict__ w,
                float* __restrict__ shared_w, int T, int E, int ld, int k, int renorm) {
  const int t = blockIdx.x * kTopkWaves + wave_id();
  if (t >= T) return;
  const int lane = lane_id();
  if constexpr (kShared) {
    if (lane == 0) {
      const float gl = (float)logits[(size_t)t * ld + E];
      shared_w[t] = (float)(bf16)(1.f / (1.f + expf(-gl)));
    }
  }
  // lane holds experts lane + 64 q; key = (ordered 16-bit logit + 1) << 8 | (255 - index), 0 =
  // absent or already taken
  unsigned key[4];
  float val[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = lane + 64 * q;
    unsigned bits = 0;
    if (j < E) bits = __builtin_bit_cast(unsigned short, logits[(size_t)t * ld + j]);
    if (bits == 0x8000u) bits = 0;   // -0 ranks as +0
    const unsigned sk = (bits & 0x8000u) ? (~bits & 0xffffu) : (bits | 0x8000u);
    key[q] = j < E ? ((sk + 1) << 8) | (unsigned)(255 - j) : 0u;
    val[q] = __uint_as_float(bits << 16);
  }
  int sel[kMaxTopK];
  float sval[kMaxTopK];
#pragma unroll
  for (int s = 0; s < kMaxTopK; ++s) {
    sel[s] = 0;
    sval[s] = 0.f;
    if (s >= k) continue;
    const unsigned best = wave_max_u32(max(max(key[0], key[1]), max(key[2], key[3])));
    const unsigned sk = (best >> 8) - 1;
    const unsigned bits = (sk & 0x8000u) ? (sk ^ 0x8000u) : (~sk & 0xffffu);
    sel[s] = 255 - (int)(best & 0xffu);
    sval[s] = __uint_as_float(bits << 16);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (key[q] == best) key[q] = 0u;
  }
  const float mx = sval[0];
  float part = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (lane + 64 * q < E) part += expf(val[q] - mx);
  const float sum = wave_reduce_sum(part);
  float p[kMaxTopK];
  float tot = 0.f;
#pragma unroll
  for (int s = 0; s < kMaxTopK; ++s) {
    p[s] = s < k ? expf(sval[s] - mx) / sum : 0.f;
    tot += p[s];
  }
#pragma unroll
  for (int s = 0; s < kMaxTopK; ++s) {
    if (s < k && lane == s) {
      const float v = renorm ? p[s] / tot : p[s];
      ids[(size_t)t * k + s] = sel[s];
      w[(size_t)t * k + s] = (float)(bf16)v;
    }
  }
}

// ------------------------------------------------------------------------------------- grouping
constexpr int kGroupThreads = 256;

__global__ void __launch_bounds__(kGroupThreads)
moe_group_kernel(const int* __restrict__ ids, int* __restrict__ expert_count,
                 int* __restrict__ expert_offset, int* __restrict__ sorted_pairs,
                 int* __restrict__ tile_expert, int* __restrict__ tile_start,
                 int* __restrict__ tile_rows, int* __restrict__ n_tiles, int P, int E, int cap) {
  __shared__ int hist[kMaxExperts];
  __shared__ int wsum[kGroupThreads / 64];
  const int e = blockIdx.x;
  const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
  for (int j = tid; j < E; j += kGroupThreads) hist[j] = 0;
  __syncthreads();
  for (int i = tid; i < P; i += kGroupThreads)
    atomicAdd(&hist[min(max(ids[i], 0), E - 1)], 1);
  __syncthreads();
  int offset = 0, tbase = 0;
  for (int j = 0; j < e; ++j) {
    const int c = hist[j];
    offset += c;
    tbase += (c + 31) >> 5;
  }
  const int cnt = hist[e];
  const int ntile = (cnt + 31) >> 5;
  if (tid == 0) {
    expert_count[e] = cnt;
    expert_offset[e] = offset;
    if (e == E - 1) {
      expert_offset[E] = offset + cnt;
      n_tiles[0] = min(tbase + ntile, cap);
    }
  }
  for (int i = tid; i < ntile; i += kGroupThreads) {
    if (tbase + i < cap) {   // always: sum ceil(c / 32) <= min(E, P) + P / 32
      tile_expert[tbase + i] = e;
      tile_start[tbase + i] = offset + 32 * i;
      tile_rows[tbase + i] = min(32, cnt - 32 * i);
    }
  }
  // scatter: pairs in ascending order, 256 at a time; slot = pairs of mine before this one
  int running = offset;
  for (int base = 0; base < P; base += kGroupThreads) {
    const int i = base + tid;
    const bool mine = i < P && min(max(ids[i], 0), E - 1) == e;
    const unsigned long long bal = __ballot(mine);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    int wpre = 0, total = 0;
#pragma unroll
    for (int v = 0; v < kGroupThreads / 64; ++v) {
      const int c = wsum[v];
      if (v < wave) wpre += c;
      total += c;
    }
    const int pos = running + wpre + before;
    if (mine && pos < P) sorted_pairs[pos] = i;
    running += total;
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------- grouped GEMM
constexpr int kTileRows = 32;          // activation rows per tile: two 16-column B tiles

enum MoeEp { kMoeGateUp = 0, kMoeDown = 1 };
enum MoeWf { kMoeBf16 = kWsBf16, kMoeFp8 = kWsFp8, kMoeFp4 = kWsFp4 };

// k-steps of weight loads in flight per lane: 8 (bf16) / 4 (fp8) 16-byte loads per step, 16
// loads in flight either way (fp8 with 2 measured 0-4 % slower: docs/kernels.md); fp4 has 2
// 16-byte loads and 2 scale bytes per step: 4 + 4 in flight with 2, which measured 0-7 % faster
// than 4 and 8 at 1-16 rows and 4-5 % slower than 4 at Mixtral's 128 / 512 rows (docs/kernels.md)
template <int WF> constexpr int kUnrollOf = WF == kMoeFp8 ? 4 : 2;

__device__ __forceinline__ int clamp_pair(int p, int P) { return min(max(p, 0), P - 1); }

// One tile: `rows` (1 .. 16 MT) activation rows x the 32 weight rows n0 .. n0 + 31 of W [N, K].
// pairs = sorted_pairs + start.  W is the expert's [N, K] bf16 (WF = kMoeBf16), e4m3 bytes with
// its N row scales `wscale` (fp32, kMoeFp8) or [N, K / 2] MXFP4 bytes with its [N, K / 32] e8m0
// block scales `wscale` (bytes, kMoeFp4).
template <int MT, int EPI, int WF>
__device__ __forceinline__ void moe_tile(char* smem, const bf16* __restrict__ x,
                                         const char* __restrict__ W,
                                         const void* __restrict__ wscale, bf16* __restrict__ out,
                                         const int* __restrict__ pairs, int start, int rows,
                                         int nb, int topk, int P, int N, int K) {
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  const int n0 = nb * kWsRowsWg;

  // N % 32 == 0: both A tiles are whole.  Image rows past `rows` repeat the tile's last row.
  f32x4 acc[2][MT];
  if (!ws_accumulate<MT, WF, kUnrollOf<WF>>(
          smem, x, W, static_cast<const uint8_t*>(wscale), n0, K, [](int n) { return n; },
          [&](int row) {
            const int tr = min(row, rows - 1);
            if constexpr (EPI == kMoeGateUp)
              return (size_t)(clamp_pair(pairs[tr], P) / topk);   // token
            else
              return (size_t)(start + tr);   // h row
          },
          acc))
    return;

  // ---- epilogue: acc[a][b][e] = y[m = 16 b + r][n = n0 + 16 a + 4 g + e] ----
  if constexpr (WF == kMoeFp8) {   // the scales of the lane's four weight rows per A tile
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const f32x4 ws = *reinterpret_cast<const f32x4*>(static_cast<const float*>(wscale) + n0 +
                                                       16 * a + 4 * g);
#pragma unroll
      for (int b = 0; b < MT; ++b)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[a][b][e] *= ws[e];
    }
  }
  if constexpr (EPI == kMoeGateUp) {
    const int I = N >> 1;
    const int col = 16 * nb + 4 * g;
#pragma unroll
    for (int b = 0; b < MT; ++b) {
      const int m = 16 * b + r;
      if (m >= rows) continue;
      bf16x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float gt = (float)(bf16)acc[0][b][e];
        const float up = (float)(bf16)acc[1][b][e];
        o[e] = (bf16)(silu(gt) * up);
      }
      *reinterpret_cast<bf16x4*>(out + (size_t)(start + m) * I + col) = o;
    }
  } else {
#pragma unroll
    for (int b = 0; b < MT; ++b) {
      const int m = 16 * b + r;
      if (m >= rows) continue;
      const size_t dst = (size_t)clamp_pair(pairs[m], P);
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (bf16)acc[a][b][e];
        *reinterpret_cast<bf16x4*>(out + dst * N + n0 + 16 * a + 4 * g) = o;
      }
    }
  }
}

template <int EPI, int WF>
__global__ void __launch_bounds__(kWsThreads)
moe_grouped_gemm_kernel(const bf16* __restrict__ x, const void* __restrict__ W,
                        const void* __restrict__ wscale, bf16* __restrict__ out,
                        const int* __restrict__ sorted_pairs,
                        const int* __restrict__ tile_expert, const int* __restrict__ tile_start,
                        const int* __restrict__ tile_rows, const int* __restrict__ n_tiles,
                        int E, int topk, int P, int N, int K) {
  __shared__ __attribute__((aligned(1024))) char smem[kWsSmem<kTileRows / 16>];
  const int tile = blockIdx.y, nb = blockIdx.x;
  if (tile >= n_tiles[0]) return;   // before any DMA or barrier
  const int e = min(max(tile_expert[tile], 0), E - 1);
  const int rows = min(max(tile_rows[tile], 1), min(kTileRows, P));
  const int start = min(max(tile_start[tile], 0), P - rows);
  // expert e's weights and scales: N rows of 2 K (bf16), K (fp8) or K / 2 (fp4) bytes; N fp32
  // row scales (fp8) or N K / 32 block-scale bytes (fp4)
  const size_t wrow = WF == kMoeFp4 ? (size_t)(K >> 1) : (size_t)K * (WF == kMoeFp8 ? 1 : 2);
  const char* We = static_cast<const char*>(W) + (size_t)e * N * wrow;
  const void* se = nullptr;
  if constexpr (WF == kMoeFp8) se = static_cast<const float*>(wscale) + (size_t)e * N;
  if constexpr (WF == kMoeFp4)
    se = static_cast<const uint8_t*>(wscale) + (size_t)e * N * (size_t)(K >> 5);
  const int* pairs = sorted_pairs + start;
  if (rows <= 16)
    moe_tile<1, EPI, WF>(smem, x, We, se, out, pairs, start, rows, nb, topk, P, N, K);
  else
    moe_tile<2, EPI, WF>(smem, x, We, se, out, pairs, start, rows, nb, topk, P, N, K);
}

// ------------------------------------------------------------------------------------- combine
// kShared: shared [T, H] (bf16) times shared_w [T] is added after the k slots
template <bool kShared>
__global__ void __launch_bounds__(256)
moe_combine_kernel(const bf16* __restrict__ y, const float* __restrict__ w,
                   const bf16* __restrict__ shared, const float* __restrict__ shared_w,
                   bf16* __restrict__ out, int T, int k, int H) {
  const int hv = H >> 3;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)T * hv) return;
  const size_t t = idx / hv;
  const int c = (int)(idx % hv) * 8;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  for (int s = 0; s < k; ++s) {
    const float ws = w[t * k + s];
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(y + (t * k + s) * H + c);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += ws * (float)v[j];
  }
  if constexpr (kShared) {
    const float ws = shared_w[t];
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(shared + t * H + c);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += ws * (float)v[j];
  }
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (bf16)acc[j];
  *reinterpret_cast<bf16x8*>(out + t * H + c) = o;
}

}  // namespace

int moe_tile_capacity(int T, int E, int k) {
  const long P = (long)T * k;
  return (int)((E < P ? E : P) + P / 32);
}

int launch_moe_topk(int* ids, float* w, const bf16* logits, int T, int E, int k, bool renorm,
                    hipStream_t stream) {
  if (T <= 0 || E <= 0 || E > kMaxExperts || k <= 0 || k > kMaxTopK || k > E) return -1;
  if (ids == nullptr || w == nullptr || logits == nullptr) return -5;
  moe_topk_kernel<false><<<(T + kTopkWaves - 1) / kTopkWaves, kTopkWaves * 64, 0, stream>>>(
      logits, ids, w, nullptr, T, E, E, k, renorm ? 1 : 0);
  return 0;
}

int launch_moe_topk_shared(int* ids, float* w, float* shared_w, const bf16* logits, int T, int E,
                           int ld, int k, bool renorm, hipStream_t stream) {
  if (T <= 0 || E <= 0 || E > kMaxExperts || k <= 0 || k > kMaxTopK || k > E) return -1;
  if (ld <= E || ld > (1 << 16)) return -2;   // column E must exist in every row
  if (ids == nullptr || w == nullptr || logits == nullptr || shared_w == nullptr) return -5;
  moe_topk_kernel<true><<<(T + kTopkWaves - 1) / kTopkWaves, kTopkWaves * 64, 0, stream>>>(
      logits, ids, w, shared_w, T, E, ld, k, renorm ? 1 : 0);
  return 0;
}

int launch_moe_group(const int* ids, int* expert_count, int* expert_offset, int* sorted_pairs,
                     int* tile_expert, int* tile_start, int* tile_rows, int* n_tiles, int T, int E,
                     int k, int cap, hipStream_t stream) {
  if (T <= 0 || E <= 0 || E > kMaxExperts || k <= 0 || k > kMaxTopK) return -1;
  if ((long)T * k > (1L << 30) || cap < moe_tile_capacity(T, E, k)) return -2;
  moe_group_kernel<<<E, kGroupThreads, 0, stream>>>(ids, expert_count, expert_offset,
                                                    sorted_pairs, tile_expert, tile_start,
                                                    tile_rows, n_tiles, T * k, E, cap);
  return 0;
}

namespace {

template <int WF>
int launch_grouped(bf16* out, const bf16* x, const void* W, const void* wscale,
                   const int* sorted_pairs, const int* tile_expert, const int* tile_start,
                   const int* tile_rows, const int* n_tiles, int cap, int T, int E, int k, int N,
                   int K, int epilogue, hipStream_t stream) {
  if (T <= 0 || E <= 0 || E > kMaxExperts || k <= 0 || k > kMaxTopK) return -1;
  if (N <= 0 || N % 32 != 0 || K <= 0 || K % 128 != 0) return -2;
  if (cap <= 0 || cap > 65535 || (long)T * k > (1L << 30)) return -3;
  if (out == nullptr || x == nullptr || W == nullptr) return -5;
  if (WF != kMoeBf16 && wscale == nullptr) return -5;
  const dim3 grid(N / kWsRowsWg, cap);
  const int P = T * k;
  if (epilogue == kMoeGateUp)
    moe_grouped_gemm_kernel<kMoeGateUp, WF><<<grid, kWsThreads, 0, stream>>>(
        x, W, wscale, out, sorted_pairs, tile_expert, tile_start, tile_rows, n_tiles, E, k, P, N,
        K);
  else if (epilogue == kMoeDown)
    moe_grouped_gemm_kernel<kMoeDown, WF><<<grid, kWsThreads, 0, stream>>>(
        x, W, wscale, out, sorted_pairs, tile_expert, tile_start, tile_rows, n_tiles, E, k, P, N,
        K);
  else
    return -4;
  return 0;
}

}  // namespace

int launch_moe_grouped_gemm(bf16* out, const bf16* x, ExpertW W, const int* sorted_pairs,
                            const int* tile_expert, const int* tile_start, const int* tile_rows,
                            const int* n_tiles, int cap, int T, int E, int k, int N, int K,
                            int epilogue, hipStream_t stream) {
  static_assert(kMoeBf16 == kExpertBf16 && kMoeFp8 == kExpertFp8 && kMoeFp4 == kExpertFp4);
  switch (W.format) {
    case kExpertBf16:
      return launch_grouped<kMoeBf16>(out, x, W.w, nullptr, sorted_pairs, tile_expert, tile_start,
                                      tile_rows, n_tiles, cap, T, E, k, N, K, epilogue, stream);
    case kExpertFp8:
      return launch_grouped<kMoeFp8>(out, x, W.w, W.scale, sorted_pairs, tile_expert, tile_start,
                                     tile_rows, n_tiles, cap, T, E, k, N, K, epilogue, stream);
    case kExpertFp4:
      return launch_grouped<kMoeFp4>(out, x, W.w, W.scale, sorted_pairs, tile_expert, tile_start,
                                     tile_rows, n_tiles, cap, T, E, k, N, K, epilogue, stream);
  }
  return -6;
}

int launch_moe_combine(bf16* out, const bf16* y, const float* w, int T, int k, int H,
                       hipStream_t stream) {
  if (T <= 0 || k <= 0 || k > kMaxTopK || H <= 0 || H % 8 != 0) return -1;
  const size_t n = (size_t)T * (H / 8);
  moe_combine_kernel<false><<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(
      y, w, nullptr, nullptr, out, T, k, H);
  return 0;
}

int launch_moe_combine_shared(bf16* out, const bf16* y, const float* w, const bf16* shared,
                              const float* shared_w, int T, int k, int H, hipStream_t stream) {
  if (T <= 0 || k <= 0 || k > kMaxTopK || H <= 0 || H % 8 != 0) return -1;
  if (out == nullptr || y == nullptr || w == nullptr || shared == nullptr ||
      shared_w == nullptr)
    return -5;
  const size_t n = (size_t)T * (H / 8);
  moe_combine_kernel<true><<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(
      y, w, shared, shared_w, out, T, k, H);
  return 0;
}

}  // namespace dli
