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
//   * block-scaled fp8 (kTileFp8Block: fp8's bytes, scale [E, N / 16, K / 128] fp32, one per 16
//     stored rows and 128 k; K % 128 == 0): staged and widened as fp8.  Each of a wave's four
//     16-row A fragments is one scale group, and a scale block is two k-steps, so the wave keeps a
//     second accumulator set for the current block: the MFMAs of steps 2 u and 2 u + 1 run into
//     it, and the odd step adds scale[group][u] * block sum to the running sum (64 fused
//     multiply-adds per lane and pair of steps, next to 64 MFMAs per wave) and clears it.  The
//     four scales of a pair are wave-uniform loads issued at its even step.  Nothing is left for
//     the epilogue.  Instantiated in moe_tile_fp8_block.hip (compiled without packed fp32
//     instructions); registers and occupancy: docs/kernels.md.
//   * LDS per buffer: 8 + 16 KB (fp8, block-scaled fp8), 4 + 16 KB (MXFP4), against 16 + 16 KB.
//
// The kernel template and its launcher are in moe_tile_core.h.
#include "moe_tile_core.h"

namespace dli {

int moe_tile_gemm_capacity(int T, int E, int k) {
  const long P = (long)T * k;
  return (int)((E < P ? E : P) + P / kTM);
}

int launch_moe_tile_gemm(bf16* out, const bf16* x, ExpertW W, const int* sorted_pairs,
                         const int* expert_count, const int* expert_offset, int T, int E, int k,
                         int N, int K, int epilogue, hipStream_t stream) {
  static_assert(kTileBf16 == kExpertBf16 && kTileFp8 == kExpertFp8 && kTileFp4 == kExpertFp4 &&
                kTileFp8Block == kExpertFp8Block);
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
    case kExpertFp8Block:   // moe_tile_fp8_block.hip
      return launch_moe_tile_fp8_block(out, x, W.w, W.scale, sorted_pairs, expert_count,
                                       expert_offset, T, E, k, N, K, epilogue, stream);
  }
  return -6;
}

}  // namespace dli
