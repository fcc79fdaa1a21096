// Repetition / presence / frequency penalties on the sampling rank (absent in the reference, which
// has no LM head - SURVEY K13).  State: one int32 table [slots, V]; bit 31 of a word = "token is
// in the prompt", bits 0-30 = n_out, the times the token was generated.  A slot belongs to one
// running sequence.
//
//   penalty_apply   edits the logits [B, V] in place for rows with a slot, before the sampler:
//                     seen (word != 0):   l = l > 0 ? l / r : l * r
//                     generated n times:  l = fma(-f, n, l);  l -= p if n > 0
//                   fp32 arithmetic, one RNE rounding to bf16 at the store; only elements whose
//                   word is non-zero are stored, the rest of the row is not written at all.
//                   Grid (column chunk, row): 256 threads x 4 elements x 4 vectors = 4096 columns
//                   per workgroup, so one penalised row at V = 128256 is 32 workgroups; rows
//                   without a slot exit at once (workgroup-uniform branch).  16-byte table loads
//                   pair with 8-byte (bf16) / 16-byte (fp32) logit accesses when V % 4 == 0 and
//                   the rows are aligned; else one element per lane.
//   penalty_feed    prefill-time: zero the rows of the segments that (re)assign a slot, then mark
//                   prompt tokens (atomic or of bit 31) and count earlier outputs (atomic add) -
//                   integer atomics, so duplicates count and the result is order-independent.
//   penalty_update  after the sampler: table[slot[b]][token[b]] += 1, one thread per row.
#include "kernels.h"

namespace dli {

namespace {

constexpr int kApplyThreads = 256;
constexpr int kApplyVecs = 4;                                   // 4-element vectors per lane
constexpr int kApplyCols = kApplyThreads * 4 * kApplyVecs;      // columns per workgroup

__device__ __forceinline__ float penalise(float l, int w, float r, float f, float p) {
  const int n = w & 0x7fffffff;
  l = l > 0.f ? l / r : l * r;
  l = __fmaf_rn(-f, (float)n, l);
  return n > 0 ? l - p : l;
}

template <bool F32, bool VEC>
__global__ void __launch_bounds__(kApplyThreads) penalty_apply_kernel(PenaltyParams p) {
  const int row = blockIdx.y;
  const int slot = p.pen_slot[row];
  if (slot < 0 || slot >= p.slots) return;
  const float r = p.rep[row], f = p.freq[row], pr = p.pres[row];
  const int V = p.V;
  const int* trow = p.table + (size_t)slot * V;
  const int c0 = blockIdx.x * kApplyCols;
  if constexpr (VEC) {
    const int n4 = V >> 2;
    const int4* t4 = reinterpret_cast<const int4*>(trow);
    int4 w[kApplyVecs];
#pragma unroll
    for (int u = 0; u < kApplyVecs; ++u) {
      const int i4 = (c0 >> 2) + u * kApplyThreads + threadIdx.x;
      w[u] = i4 < n4 ? t4[i4] : make_int4(0, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < kApplyVecs; ++u) {
      const int i4 = (c0 >> 2) + u * kApplyThreads + threadIdx.x;
      if ((w[u].x | w[u].y | w[u].z | w[u].w) == 0) continue;   // (also i4 >= n4)
      const int ww[4] = {w[u].x, w[u].y, w[u].z, w[u].w};
      if constexpr (F32) {
        float* lp = static_cast<float*>(p.logits) + (size_t)row * p.row_stride + (size_t)i4 * 4;
        const f32x4 v = *reinterpret_cast<const f32x4*>(lp);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (ww[j] != 0) lp[j] = penalise(v[j], ww[j], r, f, pr);
      } else {
        bf16* lp = static_cast<bf16*>(p.logits) + (size_t)row * p.row_stride + (size_t)i4 * 4;
        const bf16x4 v = *reinterpret_cast<const bf16x4*>(lp);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (ww[j] != 0) lp[j] = (bf16)penalise((float)v[j], ww[j], r, f, pr);
      }
    }
  } else {
    const int c1 = c0 + kApplyCols < V ? c0 + kApplyCols : V;
    for (int i = c0 + threadIdx.x; i < c1; i += kApplyThreads) {
      const int w = trow[i];
      if (w == 0) continue;
      if constexpr (F32) {
        float* lp = static_cast<float*>(p.logits) + (size_t)row * p.row_stride + i;
        *lp = penalise(*lp, w, r, f, pr);
      } else {
        bf16* lp = static_cast<bf16*>(p.logits) + (size_t)row * p.row_stride + i;
        *lp = (bf16)penalise((float)*lp, w, r, f, pr);
      }
    }
  }
}

// grid (row chunk, segment): zero the slot's row of every segment with reset
__global__ void __launch_bounds__(256) penalty_reset_kernel(int* table, int slots, int V,
                                                            const int* segs) {
  const int* s = segs + blockIdx.y * 5;
  const int slot = s[0];
  if (!s[2] || slot < 0 || slot >= slots) return;
  int* trow = table + (size_t)slot * V;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < V; i += gridDim.x * blockDim.x)
    trow[i] = 0;
}

// grid (token chunk, segment)
__global__ void __launch_bounds__(256) penalty_feed_kernel(int* table, int slots, int V,
                                                           const int* segs, const int* tokens) {
  const int* s = segs + blockIdx.y * 5;
  const int slot = s[0], kind = s[1], first = s[3], n = s[4];
  if (slot < 0 || slot >= slots) return;
  int* trow = table + (size_t)slot * V;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int t = tokens[first + i];
    if (t < 0 || t >= V) continue;
    if (kind == 0)
      atomicOr(&trow[t], (int)0x80000000u);
    else
      atomicAdd(&trow[t], 1);
  }
}

__global__ void __launch_bounds__(256) penalty_update_kernel(int* table, int slots, int V,
                                                             const int* pen_slot,
                                                             const int* tokens, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int slot = pen_slot[b], t = tokens[b];
  if (slot < 0 || slot >= slots || t < 0 || t >= V) return;
  atomicAdd(&table[(size_t)slot * V + t], 1);   // (two rows may share a slot in a hand-made batch)
}

}  // namespace

int launch_penalty_apply(const PenaltyParams& p, int B, hipStream_t stream) {
  if (B == 0 || p.V == 0) return 0;
  const uintptr_t lg = reinterpret_cast<uintptr_t>(p.logits);
  const bool vec = p.V % 4 == 0 && p.row_stride % 4 == 0 &&
                   reinterpret_cast<uintptr_t>(p.table) % 16 == 0 &&
                   lg % (p.logits_is_f32 ? 16 : 8) == 0;
  const dim3 grid((p.V + kApplyCols - 1) / kApplyCols, B);
  if (p.logits_is_f32) {
    if (vec) penalty_apply_kernel<true, true><<<grid, kApplyThreads, 0, stream>>>(p);
    else penalty_apply_kernel<true, false><<<grid, kApplyThreads, 0, stream>>>(p);
  } else {
    if (vec) penalty_apply_kernel<false, true><<<grid, kApplyThreads, 0, stream>>>(p);
    else penalty_apply_kernel<false, false><<<grid, kApplyThreads, 0, stream>>>(p);
  }
  return 0;
}

int launch_penalty_feed(int* table, int slots, int V, const int* segs, int n_seg,
                        const int* tokens, int max_n, hipStream_t stream) {
  if (n_seg == 0) return 0;
  const int rb = (V + 256 * 16 - 1) / (256 * 16);
  penalty_reset_kernel<<<dim3(rb > 0 ? rb : 1, n_seg), 256, 0, stream>>>(table, slots, V, segs);
  if (max_n > 0) {
    const int tb = (max_n + 255) / 256;
    penalty_feed_kernel<<<dim3(tb < 64 ? tb : 64, n_seg), 256, 0, stream>>>(table, slots, V, segs,
                                                                            tokens);
  }
  return 0;
}

int launch_penalty_update(int* table, int slots, int V, const int* pen_slot, const int* tokens,
                          int B, hipStream_t stream) {
  if (B == 0) return 0;
  penalty_update_kernel<<<(B + 255) / 256, 256, 0, stream>>>(table, slots, V, pen_slot, tokens, B);
  return 0;
}

}  // namespace dli
