"""The dense small-M kernels (csrc/kernels/gemm_fp8_small.hip, gemm_fp4_small.hip) and the grouped
sparse-MoE kernel (moe.hip) are one weight-streaming MFMA core (wstream_core.h) behind different
row maps and epilogues, so with a trivial grouping -- one expert, top-1, every token routed to it,
T = M <= 32: one tile, sorted_pairs the identity -- they do the same MFMAs on the same operands in
the same order, add the K-split partials in the same wave order and round once: the outputs are
equal bit for bit.  No tolerance anywhere: torch.equal on the raw bf16.

The callers keep their own kUnroll (small fp8 2 / grouped fp8 4, small fp4 4 / grouped fp4 2,
grouped bf16 2), so at K = 1152 (9 k-steps: wave 0 has two) and K = 4224 (33 steps: wave 0 has
five) the same operands go through the whole-group path in one kernel and the tail path in the
other; K = 128 is one step, seven waves have none.  M = 3 / 16 use one MFMA B tile, 17 / 32 two;
3 and 17 leave clamped image rows."""
import functools

import pytest
import torch

from distributed_llm_inference import ops

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
U8 = torch.uint8
FP8 = torch.float8_e4m3fn

SHAPES = [(M, N, K) for M in (3, 16, 17, 32) for N in (32, 64) for K in (128, 1152, 4224)]
shapes = pytest.mark.parametrize("M,N,K", SHAPES)


def _bits(t):
    return t.view(torch.int16)


@functools.lru_cache(maxsize=None)
def inputs(M, N, K):
    """Seeded CPU operands of one shape: x bf16 normal; fp8 bytes uniform over the 254 codes that
    are no NaN, positive fp32 row scales that are no powers of two; e2m1 nibbles uniform, e8m0
    block-scale bytes in [120, 134]."""
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K)
    x = torch.randn(M, K, generator=g).to(BF)
    c = torch.randint(0, 254, (N, K), generator=g)
    w8 = (c + (c >= 0x7f).long()).to(U8)         # skips 0x7f; 0xff is never reached
    assert not bool(((w8 & 0x7f) == 0x7f).any())
    ws = (0.003 + 0.004 * torch.rand(N, generator=g)).float()
    frac = torch.frexp(ws)[0]
    assert bool((ws > 0).all()) and not bool((frac == 0.5).any())
    w4 = torch.randint(0, 256, (N, K // 2), generator=g).to(U8)
    bs = torch.randint(120, 135, (N, K // 32), generator=g).to(U8)
    return dict(x=x, w8=w8.view(FP8), ws=ws, w4=w4, bs=bs)


def _on(gpu, M, N, K):
    c = {k: v.to(gpu) for k, v in inputs(M, N, K).items()}
    ids = torch.zeros(M, 1, dtype=torch.int32, device=gpu)
    c["r"] = ops.moe_group(ids, torch.ones(M, 1, device=gpu), 1)
    return c


def _equal(small, grouped, what):
    torch.cuda.synchronize()
    assert bool(small.float().isfinite().all()) and bool((small != 0).any()), what
    assert small.shape == grouped.shape, what
    assert torch.equal(_bits(small), _bits(grouped)), what


@shapes
def test_trivial_grouping_is_the_identity(gpu, M, N, K):
    r = _on(gpu, M, N, K)["r"]
    assert r.sorted_pairs[:M].tolist() == list(range(M))
    assert int(r.n_tiles[0]) == 1 and int(r.tile_rows[0]) == M and int(r.tile_start[0]) == 0


@shapes
def test_small_fp8_plain_equals_grouped_fp8_down(gpu, M, N, K):
    c = _on(gpu, M, N, K)
    small = ops.small_gemm_fp8(c["x"], c["w8"], c["ws"])
    grouped = ops.moe_grouped_gemm(c["x"], c["w8"][None], c["r"], down=True,
                                   w_scale=c["ws"][None], tiles=False)
    _equal(small, grouped, f"fp8 plain / down M={M} N={N} K={K}")


@shapes
def test_small_fp4_plain_equals_grouped_fp4_down(gpu, M, N, K):
    c = _on(gpu, M, N, K)
    small = ops.small_gemm_fp4(c["x"], c["w4"], c["bs"])
    grouped = ops.moe_grouped_gemm(c["x"], c["w4"][None], c["r"], down=True,
                                   w_block_scale=c["bs"][None], tiles=False)
    _equal(small, grouped, f"fp4 plain / down M={M} N={N} K={K}")


@shapes
def test_small_fp8_swiglu_equals_grouped_fp8_gate_up(gpu, M, N, K):
    c = _on(gpu, M, N, K)
    small = ops.small_gemm_fp8(c["x"], c["w8"], c["ws"], swiglu=True)
    grouped = ops.moe_grouped_gemm(c["x"], c["w8"][None], c["r"], w_scale=c["ws"][None],
                                   tiles=False)
    _equal(small, grouped, f"fp8 swiglu / gate|up M={M} N={N} K={K}")


@shapes
def test_small_fp4_swiglu_equals_grouped_fp4_gate_up(gpu, M, N, K):
    c = _on(gpu, M, N, K)
    small = ops.small_gemm_fp4(c["x"], c["w4"], c["bs"], swiglu=True)
    grouped = ops.moe_grouped_gemm(c["x"], c["w4"][None], c["r"], w_block_scale=c["bs"][None],
                                   tiles=False)
    _equal(small, grouped, f"fp4 swiglu / gate|up M={M} N={N} K={K}")


@shapes
def test_small_fp4_plain_equals_grouped_bf16_on_dequantised_weights(gpu, M, N, K):
    """Ties the bf16 arm in: e2m1 * 2^(byte - 127) is exact in bf16."""
    c = _on(gpu, M, N, K)
    wb = ops.dequantize_mxfp4(c["w4"], c["bs"])
    assert wb.dtype == BF and wb.shape == (N, K)
    small = ops.small_gemm_fp4(c["x"], c["w4"], c["bs"])
    grouped = ops.moe_grouped_gemm(c["x"], wb[None], c["r"], down=True, tiles=False)
    _equal(small, grouped, f"fp4 plain / bf16 down M={M} N={N} K={K}")
