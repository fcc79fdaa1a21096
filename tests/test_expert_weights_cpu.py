"""``ops.ExpertWeights``: the routed experts' weights with the scale of their format (bf16, fp8 with
row scales, MXFP4 with block scales).  Format and logical sizes, ``dequantize`` against the
formulas written out, ``ops.moe_grouped_gemm`` on an ``ExpertWeights`` against its keyword form
bit for bit, and the rejected combinations."""
import pytest
import torch

from distributed_llm_inference import ops

BF = torch.bfloat16
E, N, K = 2, 32, 128
FMTS = ["bf16", "fp8", "mxfp4"]
SCALE_KW = {"fp8": "w_scale", "mxfp4": "w_block_scale"}


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.fixture(scope="module")
def weights():
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(E, N, K, generator=g) / K ** 0.5).to(BF)
    return {fmt: ops.ExpertWeights.quantize(w, fmt) for fmt in FMTS}


def test_format_and_logical_sizes(weights):
    for fmt in FMTS:
        e = weights[fmt]
        assert (e.format, e.E, e.N, e.K) == (fmt, E, N, K)
    assert weights["bf16"].scale is None
    w8, s8 = weights["fp8"]
    assert w8.dtype == torch.float8_e4m3fn and w8.shape == (E, N, K)
    assert s8.dtype == torch.float32 and s8.shape == (E, N)
    w4, s4 = weights["mxfp4"]
    assert w4.dtype == torch.uint8 and w4.shape == (E, N, K // 2)
    assert s4.dtype == torch.uint8 and s4.shape == (E, N, K // 32)
    for fmt, fn in (("fp8", ops.quantize_expert_weights_fp8),
                    ("mxfp4", ops.quantize_expert_weights_mxfp4)):
        q, s = fn(weights["bf16"].w)
        assert torch.equal(weights[fmt].w.view(torch.uint8), q.view(torch.uint8))
        assert torch.equal(weights[fmt].scale, s)
    with pytest.raises(ValueError, match="format"):
        ops.ExpertWeights.quantize(weights["bf16"].w, "int8")
    with pytest.raises(ValueError, match="expert weights are"):
        ops.ExpertWeights(weights["bf16"].w.float()).format


def test_dequantize_is_the_blocks_old_arithmetic(weights):
    for e in range(E):
        w, _ = weights["bf16"]
        assert torch.equal(_bits(weights["bf16"].dequantize(e)), _bits(w[e]))
        w8, s8 = weights["fp8"]
        want = (w8[e].float() * s8[e][:, None]).to(BF)       # fp32 product, one rounding
        assert torch.equal(_bits(weights["fp8"].dequantize(e)), _bits(want))
        w4, s4 = weights["mxfp4"]
        want = ops.dequantize_mxfp4(w4[e], s4[e])
        got = weights["mxfp4"].dequantize(e)
        assert got.dtype == BF and torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("fmt", FMTS)
def test_grouped_gemm_equals_the_keyword_form(weights, fmt):
    """Both epilogues.  The gate|up epilogue reads rows in ``swiglu_interleave`` order, whose unit
    is 256 rows, so its weights are [E, 256, K]; the down product runs on the [E, 32, K] ones."""
    T, k = 6, 2
    g = torch.Generator().manual_seed(6)
    x = torch.randn(T, K, generator=g).to(BF)
    h = torch.randn(T * k, K, generator=g).to(BF)
    r = ops.moe_route(torch.randn(T, E, generator=g).to(BF), k, True)
    gate_up = ops.ExpertWeights.quantize(
        (torch.randn(E, 256, K, generator=g) / K ** 0.5).to(BF), fmt)
    for down, xin, e in ((False, x, gate_up), (True, h, weights[fmt])):
        kw = {SCALE_KW[fmt]: e.scale} if fmt != "bf16" else {}
        got = ops.moe_grouped_gemm(xin, e, r, down=down)
        want = ops.moe_grouped_gemm(xin, e.w, r, down=down, **kw)
        assert got.shape == (T * k, N if down else 128)
        assert torch.equal(_bits(got), _bits(want))
        assert float(want.float().abs().max()) > 0.01


def test_rejected_combinations(weights):
    x = torch.randn(4, K).to(BF)
    r = ops.moe_route(torch.randn(4, E).to(BF), 2, True)
    w8, s8 = weights["fp8"]
    w4, s4 = weights["mxfp4"]
    wb = weights["bf16"].w
    for kw in ({"w_scale": s8}, {"w_block_scale": s4}):
        with pytest.raises(ValueError, match="ExpertWeights"):
            ops.moe_grouped_gemm(x, weights["fp8"], r, **kw)
    with pytest.raises(ValueError, match="w_block_scale"):       # fp8 weights, a uint8 scale
        ops.moe_grouped_gemm(x, ops.ExpertWeights(w8, s4), r)
    with pytest.raises(ValueError, match="w_block_scale"):
        ops.moe_grouped_gemm(x, ops.ExpertWeights(w8, s8.to(torch.uint8)), r)
    for s in (s8, s4):                                           # bf16 weights with a scale
        with pytest.raises(ValueError):
            ops.moe_grouped_gemm(x, ops.ExpertWeights(wb, s), r)
    with pytest.raises(ValueError, match="w_block_scale"):       # nibbles without their scales
        ops.moe_grouped_gemm(x, ops.ExpertWeights(w4), r)
    with pytest.raises(ValueError, match="w_scale"):             # fp8 weights without theirs
        ops.moe_grouped_gemm(x, ops.ExpertWeights(w8), r)
