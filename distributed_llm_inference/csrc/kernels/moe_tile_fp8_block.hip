// Sparse mixture-of-experts MLP, block-scaled fp8 experts with many rows: the grouped MFMA tile
// GEMM of moe_tile.hip / moe_tile_core.h instantiated for WF = kTileFp8Block (W8 [E, N, K] e4m3fn
// bytes, scale [E, N / 16, K / 128] fp32).  The layout, the second accumulator set and the flush
// every second k-step are described in moe_tile.hip.  This file is compiled without packed fp32
// instructions (the flush must not become v_pk_fma_f32); the instantiations of the other formats
// stay in moe_tile.hip with the code they had.
#include "moe_tile_core.h"

namespace dli {

int launch_moe_tile_fp8_block(bf16* out, const bf16* x, const void* W, const void* wscale,
                              const int* sorted_pairs, const int* expert_count,
                              const int* expert_offset, int T, int E, int k, int N, int K,
                              int epilogue, hipStream_t stream) {
  return launch_tile<kTileFp8Block>(out, x, W, wscale, sorted_pairs, expert_count, expert_offset,
                                    T, E, k, N, K, epilogue, stream);
}

}  // namespace dli
