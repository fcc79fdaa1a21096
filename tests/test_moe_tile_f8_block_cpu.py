"""The CPU side of moe_tile_scaled.hip: ``moe_grouped_gemm(f8_block=True)``, the oracle of the
GPU path, ``moe_uses_f8_block`` and the ``KernelPolicy.moe_tile_f8_block`` knob."""
import pytest
import torch

import moe_tile_cases as mc
from distributed_llm_inference import ops
from distributed_llm_inference.config import KernelPolicy
from distributed_llm_inference.ops import reference as ref

BF = torch.bfloat16
E, K = mc.E, mc.K_TOP


@pytest.mark.parametrize("down", [False, True])
def test_f8_block_cpu_path_and_refusals(down):
    H, I = 256, 128
    g = torch.Generator().manual_seed(12)
    ids = mc.explicit_ids()
    r = ops.moe_group(ids, torch.ones(ids.shape), E)
    N, Kd, R = (H, I, ids.numel()) if down else (2 * I, H, ids.shape[0])
    x = torch.randn(R, Kd, generator=g).to(BF)
    wb = (torch.randn(E, N, Kd, generator=g) / Kd ** 0.5).to(BF)
    w = ops.ExpertWeights.quantize(wb, "fp8_block")
    got = ops.moe_grouped_gemm(x, w, r, down=down, f8_block=True)
    want = ref.moe_grouped_gemm(ops.quant_mx_rows(x).dequantize(), w, r, int(down),
                                torch.zeros_like(got))
    assert torch.equal(got, want)
    assert torch.equal(ops.moe_grouped_gemm(ops.quant_mx_rows(x), w, r, down=down, f8_block=True), want)
    plain = ops.moe_grouped_gemm(x, w, r, down=down)
    assert not torch.equal(got, plain)
    for kw in ({}, {"f8_block": None}, {"f8_block": False}):      # every knob off
        assert torch.equal(ops.moe_grouped_gemm(x, w, r, down=down, **kw), plain)
    odd = ops.ExpertWeights(w.w[:, :N - 16].contiguous(), w.scale[:, :N // 16 - 1].contiguous())
    for bad, kw in [(w, {"mx": True}), (w, {"tiles": False}), (odd, {}), (wb, {}),
                    (ops.ExpertWeights.quantize(wb, "fp8"), {}),
                    (ops.ExpertWeights.quantize(wb, "mxfp4"), {})]:
        with pytest.raises(ValueError, match="f8_block=True"):
            ops.moe_grouped_gemm(x, bad, r, down=down, f8_block=True, **kw)
    with pytest.raises(ValueError, match="mx=True"):              # stays what it was
        ops.moe_grouped_gemm(x, w, r, down=down, mx=True)


@pytest.mark.parametrize("fmt,rows_q,knob,dev,T,want", [
    ("fp8_block", 32, True, "cuda", 128, True),
    ("fp8_block", 32, True, "cuda", 127, False),    # below the tile threshold: T k < rows E
    ("fp8_block", 32, False, "cuda", 128, False),   # the knob is off
    ("fp8_block", 0, True, "cuda", 128, False),     # quantised experts are not on the tiles
    ("fp8_block", 32, True, "cpu", 128, False),
    ("fp8", 32, True, "cuda", 128, False),          # every other format ignores it
    ("mxfp4", 32, True, "cuda", 128, False),
    ("bf16", 32, True, "cuda", 128, False),
])
def test_moe_uses_f8_block_truth_table(fmt, rows_q, knob, dev, T, want):
    with ops.kernel_policy(moe_tile_rows=32, moe_tile_rows_q=rows_q, moe_tile_f8_block=knob):
        assert ops.moe_uses_f8_block(T, K, E, fmt, torch.device(dev)) is want
        assert ops.moe_uses_f8(T, K, E, fmt, torch.device(dev)) is False     # its own knob is off


def test_policy_override_round_trip():
    assert KernelPolicy().moe_tile_f8_block is False
    on = KernelPolicy().with_overrides("moe_tile_rows_q=32,moe_tile_f8_block=1")
    assert on.moe_tile_f8_block is True and on.moe_tile_rows_q == 32 and on.moe_tile_f8 is False
    assert on.with_overrides("moe_tile_f8_block=0") == KernelPolicy(moe_tile_rows_q=32)
