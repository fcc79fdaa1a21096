// Sparse mixture-of-experts MLP, block-scaled fp8 experts (the hub's 128 x 128 FP8 checkpoints):
// the grouped weight-streaming MFMA GEMM of moe.hip / moe_grouped.h instantiated for
// WF = kMoeFp8Block.  W8 [E, N, K] holds e4m3fn bytes in the stored row order, scale
// [E, N / 16, K / 128] one fp32 per 16 consecutive stored rows and 128 consecutive k.
//
//   * why 16 rows.  A workgroup's 32 weight rows are two 16-row MFMA A tiles, so one scale covers
//     a whole A tile of a k-step (128 k): the rescale is one fp32 factor per (A tile, step), the
//     same in every lane.  A checkpoint's 128-row block is eight such groups (the loader repeats
//     its scale), and after ops.swiglu_interleave 16 consecutive stored gate|up rows are still 16
//     consecutive rows of one projection, so the expansion is exact for gate|up as well.
//   * the k-loop (wstream_core.h, kWsFp8Block).  Per step and A tile the four MFMAs accumulate into
//     a zeroed step accumulator, then acc += scale * step on the vector ALU: 4 MT fused
//     multiply-adds per A tile and step next to 4 MT MFMAs.  The two scale dwords of a step are
//     loaded with the step's weight loads, kUnroll = 4 steps ahead.  Everything else -- x through
//     LDS, the K split over the 8 waves and its sum in LDS, SwiGLU, the scatter -- is the other
//     formats', and nothing is left for the epilogue.
//   * this file is compiled without packed fp32 instructions (the rescale must not become
//     v_pk_fma_f32); the instantiations of the other formats stay in moe.hip with the code they had.
#include "moe_grouped.h"

namespace dli {

int launch_moe_grouped_fp8_block(bf16* out, const bf16* x, const void* W, const void* wscale,
                                 const int* sorted_pairs, const int* tile_expert,
                                 const int* tile_start, const int* tile_rows, const int* n_tiles,
                                 int cap, int T, int E, int k, int N, int K, int epilogue,
                                 hipStream_t stream) {
  return launch_grouped<kMoeFp8Block>(out, x, W, wscale, sorted_pairs, tile_expert, tile_start,
                                      tile_rows, n_tiles, cap, T, E, k, N, K, epilogue, stream);
}

}  // namespace dli
