"""The CPU side of the block-scaled fp8 x fp8 MoE tile GEMM (moe_tile_scaled.hip):
``moe_grouped_gemm(mx=True)`` on fp8 experts is the oracle of the GPU path, ``moe_uses_f8`` and the
``KernelPolicy.moe_tile_f8`` knob."""
import pytest
import torch

import moe_tile_cases as mc
from distributed_llm_inference import ops
from distributed_llm_inference.config import KernelPolicy
from distributed_llm_inference.ops import reference as ref

BF = torch.bfloat16
E, K = mc.E, mc.K_TOP


@pytest.mark.parametrize("down", [False, True])
def test_mx_cpu_path_on_fp8_experts(down):
    H, I = 256, 128
    g = torch.Generator().manual_seed(12)
    ids = mc.explicit_ids()
    r = ops.moe_group(ids, torch.ones(ids.shape), E)
    N, Kd, R = (H, I, ids.numel()) if down else (2 * I, H, ids.shape[0])
    x = torch.randn(R, Kd, generator=g).to(BF)
    w = ops.ExpertWeights.quantize((torch.randn(E, N, Kd, generator=g) / Kd ** 0.5).to(BF), "fp8")
    assert w.format == "fp8"
    got = ops.moe_grouped_gemm(x, w, r, down=down, mx=True)
    want = ref.moe_grouped_gemm(ops.quant_mx_rows(x).dequantize(), w, r, int(down),
                                torch.zeros_like(got))
    assert torch.equal(got, want)
    plain = ops.moe_grouped_gemm(x, w, r, down=down)
    assert not torch.equal(got, plain)
    # every knob off: mx=None is the call without mx
    assert torch.equal(ops.moe_grouped_gemm(x, w, r, down=down, mx=None), plain)
    with pytest.raises(ValueError, match="bf16 experts"):
        ops.moe_grouped_gemm(x, torch.zeros(E, N, Kd, dtype=BF), r, down=down, mx=True)


@pytest.mark.parametrize("fmt,rows_q,knob,dev,T,want", [
    ("fp8", 32, True, "cuda", 128, True),
    ("fp8", 32, True, "cuda", 127, False),       # below the tile threshold: T k < rows E
    ("fp8", 32, False, "cuda", 128, False),      # the knob is off
    ("fp8", 0, True, "cuda", 128, False),        # quantised experts are not on the tiles
    ("fp8", 32, True, "cpu", 128, False),
    ("mxfp4", 32, True, "cuda", 128, False),     # MXFP4 and bf16 experts ignore it
    ("bf16", 32, True, "cuda", 128, False),
])
def test_moe_uses_f8_truth_table(fmt, rows_q, knob, dev, T, want):
    with ops.kernel_policy(moe_tile_rows=32, moe_tile_rows_q=rows_q, moe_tile_f8=knob):
        assert ops.moe_uses_f8(T, K, E, fmt, torch.device(dev)) is want
        assert ops.moe_uses_mx(T, K, E, fmt, torch.device(dev)) is False     # its own knob is off


def test_policy_override_round_trip():
    assert KernelPolicy().moe_tile_f8 is False
    on = KernelPolicy().with_overrides("moe_tile_rows_q=32,moe_tile_f8=1")
    assert on.moe_tile_f8 is True and on.moe_tile_rows_q == 32 and on.moe_tile_mx is False
    assert on.with_overrides("moe_tile_f8=0") == KernelPolicy(moe_tile_rows_q=32)
