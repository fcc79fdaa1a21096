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
//   * moe_grouped_gemm.  gemm_fp8_small.hip's structure on bf16 weights: the weight is the MFMA A
//     operand of v_mfma_f32_16x16x32_bf16 (lane (r, g) holds W[n0 + r][128 t + 32 g + 8 i + j] for
//     MFMA i of k-step t: four non-temporal 16-byte loads per A tile and step), 32 weight rows per
//     workgroup, the 8 waves split K, each wave stages the x of its own k-step by LDS-DMA in a
//     private double buffer (swizzle on the source address) and the partials are added in wave
//     order in LDS.  Grid (N / 32, tile capacity); workgroup (nb, tile) multiplies the <= 32 rows
//     of its tile with rows 32 nb .. 32 nb + 31 of its tile's expert.  A tile index >= n_tiles
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
//     fp8 weights (WF = kMoeFp8: W8 [E, N, K] e4m3fn bytes, w_scale [E, N] fp32): the same kernel
//     with gemm_fp8_small.hip's A operand -- lane (r, g) loads the 32 bytes
//     W8[n0 + 16 a + r][128 t + 32 g .. + 31] as two non-temporal 16-byte loads per A tile and
//     step, and dwords 2 i, 2 i + 1, widened e4m3 -> bf16 in registers (exact), are its A fragment
//     of MFMA i: the k order, the wave's steps and the order of the MFMAs are the bf16 variant's.
//     The activations are never quantised; the scale of weight row n of expert e,
//     w_scale[e N + n], multiplies the fp32 accumulator after the K-split sum (gate and up each
//     by their own row's scale before their bf16 rounding).
//     MXFP4 weights (WF = kMoeFp4: W4 [E, N, K / 2] bytes, element 2 j in the low nibble of byte
//     j, bscale [E, N, K / 32] e8m0 bytes): the same kernel with gemm_fp4_small.hip's A operand --
//     lane (r, g) loads the 16 bytes W4[n0 + 16 a + r][64 t + 16 g .. + 15] = W[..][128 t + 32 g
//     .. + 31] as one non-temporal 16-byte load per A tile and step, exactly one scale block, and
//     the block's byte bscale[n0 + 16 a + r][4 t + g]; dword i, widened e2m1 -> bf16 in registers
//     with the block's 2^(byte - 127) (v_cvt_scalef32_pk_bf16_fp4, exact), is its A fragment of
//     MFMA i: again the k order, the wave's steps and the order of the MFMAs are the bf16
//     variant's, so the result is the bf16 kernel's on the dequantised weights bit for bit.  The
//     scale is spent in the widening: nothing is left for the epilogue, and the activations are
//     never quantised.
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
#include "kernels.h"

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
constexpr int kWaves = 8;              // K-split ways = waves per workgroup
constexpr int kThreads = kWaves * 64;
constexpr int kRowsWg = 32;            // weight rows per workgroup: two 16-row A tiles
constexpr int kTileRows = 32;          // activation rows per tile: two 16-column B tiles

enum MoeEp { kMoeGateUp = 0, kMoeDown = 1 };
enum MoeWf { kMoeBf16 = 0, kMoeFp8 = 1, kMoeFp4 = 2 };

// k-steps of weight loads in flight per lane: 8 (bf16) / 4 (fp8) 16-byte loads per step, 16
// loads in flight either way (fp8 with 2 measured 0-4 % slower: docs/kernels.md); fp4 has 2
// 16-byte loads and 2 scale bytes per step: 4 + 4 in flight with 2, which measured 0-7 % faster
// than 4 and 8 at 1-16 rows and 4-5 % slower than 4 at Mixtral's 128 / 512 rows (docs/kernels.md)
template <int WF> constexpr int kUnrollOf = WF == kMoeFp8 ? 4 : 2;
static_assert(kUnrollOf<kMoeBf16> % 2 == 0 && kUnrollOf<kMoeFp8> % 2 == 0 &&
                  kUnrollOf<kMoeFp4> % 2 == 0,
              "a group starts on x buffer 0");

typedef unsigned u32x4m __attribute__((ext_vector_type(4)));   // nontemporal-loadable 16 B

typedef __attribute__((address_space(3))) void lds_void_m;
typedef __attribute__((address_space(1))) void gbl_void_m;

// 16 bytes per lane global -> LDS (LDS-DMA): the wave's 64 lanes fill 1 KB at `lds_wave_base`
__device__ __forceinline__ void glds16(const void* g, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((gbl_void_m*)g, (lds_void_m*)lds_wave_base, 16, 0, 0);
}
template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// the 16-byte slot of chunk ch of x row c in the staged image is ch ^ swz(c)
__device__ __forceinline__ int swz(int c) { return c ^ ((c & 4) << 1); }

// one dword = 8 e2m1 nibbles (element 2 b, 2 b + 1 in byte b) -> 8 bf16, scaled by s (exact)
__device__ __forceinline__ bf16x8 fp4x8_to_bf16x8(unsigned d, float s) {
  const bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 0);
  const bf16x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 1);
  const bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 2);
  const bf16x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 3);
  return bf16x8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}

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
  constexpr int kWB = WF == kMoeBf16 ? 2 : 1;   // bytes per weight (kMoeFp4: half a byte, below)
  constexpr int kWL = WF == kMoeFp4 ? 1 : 2 * kWB;   // 16-byte loads per A tile and k-step
  constexpr int kStepB = 16 * 4 * kWL;         // bytes of a weight row per k-step: 4 lanes' loads
  constexpr int kUnroll = kUnrollOf<WF>;
  constexpr int kXBuf = MT * 16 * 256;   // one k-step of x: 16 MT rows x 128 bf16
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int n0 = nb * kRowsWg;
  const int kt = K >> 7;
  char* xw = smem + wave * (2 * kXBuf);   // this wave's two x buffers; nobody else touches them

  // this lane's weight rows (A tiles 0 / 1; N % 32 == 0: both whole) at its 32-k block of step 0
  // (kMoeFp4: a row is K / 2 bytes, and the lane's scale byte of step 0 is block g of its row)
  const char* wp[2];
  const uint8_t* sp[2];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const size_t n = (size_t)(n0 + 16 * a + r);
    if constexpr (WF == kMoeFp4) {
      wp[a] = W + n * (size_t)(K >> 1) + 16 * g;
      sp[a] = static_cast<const uint8_t*>(wscale) + n * (size_t)(K >> 5) + g;
    } else {
      wp[a] = W + (n * K + 32 * g) * kWB;
      sp[a] = nullptr;
    }
  }
  // x staging: DMA instruction q fills image rows 4 q .. 4 q + 3 (lane l: row 4 q + (l >> 4),
  // slot l & 15) with whole 256-byte row pieces; the slot permutation is on the source address.
  // Image rows past `rows` repeat the tile's last row.
  const bf16* xsrc[4 * MT];
#pragma unroll
  for (int q = 0; q < 4 * MT; ++q) {
    const int row = 4 * q + g;
    const int tr = min(row, rows - 1);
    size_t src;
    if constexpr (EPI == kMoeGateUp) src = (size_t)(clamp_pair(pairs[tr], P) / topk);   // token
    else src = (size_t)(start + tr);                                                    // h row
    xsrc[q] = x + src * K + ((r ^ swz(row & 15)) << 3);
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
  // kMoeFp4: the scale bytes are vector memory loads too, issued here with the weight loads,
  // i.e. before the next stage_x -- so "all but the 4 MT newest" below still covers them
  auto load_w = [&](int t, u32x4m (&wv)[2][kWL], unsigned (&sc)[2]) {
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
      for (int i = 0; i < kWL; ++i)
        wv[a][i] = __builtin_nontemporal_load(
            reinterpret_cast<const u32x4m*>(wp[a] + (size_t)t * kStepB + 16 * i));
      if constexpr (WF == kMoeFp4) sc[a] = sp[a][(size_t)t * 4];
    }
  };
  auto stage_x = [&](int t, int buf) {
#pragma unroll
    for (int q = 0; q < 4 * MT; ++q)
      glds16(xsrc[q] + (size_t)t * 128, xw + buf * kXBuf + q * 1024);
  };
  auto step = [&](int buf, const u32x4m (&wv)[2][kWL], const unsigned (&sc)[2]) {
    bf16x8 xb[MT][4];
#pragma unroll
    for (int b = 0; b < MT; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        xb[b][i] = *reinterpret_cast<const bf16x8*>(xw + buf * kXBuf + b * 4096 + xoff[i]);
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      float s = 0.f;   // kMoeFp4: 2^(byte - 127), byte in [1, 254]
      if constexpr (WF == kMoeFp4) s = __uint_as_float(sc[a] << 23);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        bf16x8 wf;
        if constexpr (WF == kMoeFp4)   // dword i of the lane's 4: exact widening
          wf = fp4x8_to_bf16x8(wv[a][0][i], s);
        else if constexpr (WF == kMoeFp8)   // dwords 2 i, 2 i + 1 of the lane's 8: exact widening
          wf = fp8x8_to_bf16x8(uint2{wv[a][i >> 1][2 * (i & 1)], wv[a][i >> 1][2 * (i & 1) + 1]});
        else
          wf = __builtin_bit_cast(bf16x8, wv[a][i]);
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
    u32x4m wv[kUnroll][2][kWL];
    unsigned sc[kUnroll][2];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) load_w(wave + (i + u) * kWaves, wv[u], sc[u]);
    asm volatile("" ::: "memory");
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      if (u + 1 < kUnroll || i + kUnroll < nsteps) {
        stage_x(wave + (i + u + 1) * kWaves, (u + 1) & 1);
        wait_vm<4 * MT>();
      } else {
        wait_vm<0>();
      }
      step(u & 1, wv[u], sc[u]);
      asm volatile("" ::: "memory");   // the next DMA into this buffer stays behind its reads
    }
  }
  for (; i < nsteps; ++i) {   // fewer than kUnroll steps left
    u32x4m wv[2][kWL];
    unsigned sc[2];
    load_w(wave + i * kWaves, wv, sc);
    asm volatile("" ::: "memory");
    if (i + 1 < nsteps) {
      stage_x(wave + (i + 1) * kWaves, (i + 1) & 1);
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
__global__ void __launch_bounds__(kThreads)
moe_grouped_gemm_kernel(const bf16* __restrict__ x, const void* __restrict__ W,
                        const void* __restrict__ wscale, bf16* __restrict__ out,
                        const int* __restrict__ sorted_pairs,
                        const int* __restrict__ tile_expert, const int* __restrict__ tile_start,
                        const int* __restrict__ tile_rows, const int* __restrict__ n_tiles,
                        int E, int topk, int P, int N, int K) {
  __shared__ __attribute__((aligned(1024))) char smem[kWaves * 2 * (kTileRows * 256)];
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
  const dim3 grid(N / kRowsWg, cap);
  const int P = T * k;
  if (epilogue == kMoeGateUp)
    moe_grouped_gemm_kernel<kMoeGateUp, WF><<<grid, kThreads, 0, stream>>>(
        x, W, wscale, out, sorted_pairs, tile_expert, tile_start, tile_rows, n_tiles, E, k, P, N,
        K);
  else if (epilogue == kMoeDown)
    moe_grouped_gemm_kernel<kMoeDown, WF><<<grid, kThreads, 0, stream>>>(
        x, W, wscale, out, sorted_pairs, tile_expert, tile_start, tile_rows, n_tiles, E, k, P, N,
        K);
  else
    return -4;
  return 0;
}

}  // namespace

int launch_moe_grouped_gemm(bf16* out, const bf16* x, const bf16* W, const int* sorted_pairs,
                            const int* tile_expert, const int* tile_start, const int* tile_rows,
                            const int* n_tiles, int cap, int T, int E, int k, int N, int K,
                            int epilogue, hipStream_t stream) {
  return launch_grouped<kMoeBf16>(out, x, W, nullptr, sorted_pairs, tile_expert, tile_start,
                                  tile_rows, n_tiles, cap, T, E, k, N, K, epilogue, stream);
}

int launch_moe_grouped_gemm_fp8(bf16* out, const bf16* x, const uint8_t* W8, const float* w_scale,
                                const int* sorted_pairs, const int* tile_expert,
                                const int* tile_start, const int* tile_rows, const int* n_tiles,
                                int cap, int T, int E, int k, int N, int K, int epilogue,
                                hipStream_t stream) {
  return launch_grouped<kMoeFp8>(out, x, W8, w_scale, sorted_pairs, tile_expert, tile_start,
                                 tile_rows, n_tiles, cap, T, E, k, N, K, epilogue, stream);
}

int launch_moe_grouped_gemm_fp4(bf16* out, const bf16* x, const uint8_t* W4, const uint8_t* bscale,
                                const int* sorted_pairs, const int* tile_expert,
                                const int* tile_start, const int* tile_rows, const int* n_tiles,
                                int cap, int T, int E, int k, int N, int K, int epilogue,
                                hipStream_t stream) {
  return launch_grouped<kMoeFp4>(out, x, W4, bscale, sorted_pairs, tile_expert, tile_start,
                                 tile_rows, n_tiles, cap, T, E, k, N, K, epilogue, stream);
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
