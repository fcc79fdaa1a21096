"""The CPU side of the block-scaled MoE tile GEMM (moe_tile_scaled.hip): ``moe_grouped_gemm(mx=True)``
is the oracle of the GPU path, ``moe_uses_mx`` and the ``KernelPolicy.moe_tile_mx`` knob."""
import pytest
import torch

import moe_tile_cases as mc
from distributed_llm_inference import ops
from distributed_llm_inference.config import KernelPolicy
from distributed_llm_inference.ops import reference as ref

BF = torch.bfloat16
E, K = mc.E, mc.K_TOP


@pytest.mark.parametrize("down", [False, True])
def test_mx_cpu_path_is_the_explicit_formula(down):
    H, I = 256, 128
    g = torch.Generator().manual_seed(11)
    ids = mc.explicit_ids()
    r = ops.moe_group(ids, torch.ones(ids.shape), E)
    pairs = r.sorted_pairs.long()
    N, Kd, R = (H, I, ids.numel()) if down else (2 * I, H, ids.shape[0])
    x = torch.randn(R, Kd, generator=g).to(BF)
    w = ops.ExpertWeights.quantize((torch.randn(E, N, Kd, generator=g) / Kd ** 0.5).to(BF), "mxfp4")
    got = ops.moe_grouped_gemm(x, w, r, down=down, mx=True)
    xd = ops.mx_quantize(x).dequantize()
    assert torch.equal(ops.quant_mx_rows(x).dequantize(), xd)
    for e in range(E):
        a, b = int(r.expert_offset[e]), int(r.expert_offset[e + 1])
        wd = ops.dequantize_mxfp4(w.w[e], w.scale[e]).float().t()
        if down:
            assert torch.equal(got[pairs[a:b]], (xd[a:b] @ wd).to(BF))
        else:
            assert torch.equal(got[a:b], ref._swiglu_interleaved(xd[pairs[a:b] // K] @ wd))
    assert not torch.equal(got, ops.moe_grouped_gemm(x, w, r, down=down, mx=False))
    with pytest.raises(ValueError, match="MXFP4"):
        ops.moe_grouped_gemm(x, torch.zeros(E, N, Kd, dtype=BF), r, down=down, mx=True)


@pytest.mark.parametrize("fmt,rows_q,knob,dev,T,want", [
    ("mxfp4", 32, True, "cuda", 128, True),
    ("mxfp4", 32, True, "cuda", 127, False),     # below the tile threshold: T k < rows E
    ("mxfp4", 32, False, "cuda", 128, False),    # the knob is off
    ("mxfp4", 0, True, "cuda", 128, False),      # quantised experts are not on the tiles
    ("mxfp4", 32, True, "cpu", 128, False),
    ("fp8", 32, True, "cuda", 128, False),       # fp8 and bf16 experts ignore it
    ("bf16", 32, True, "cuda", 128, False),
])
def test_moe_uses_mx_truth_table(fmt, rows_q, knob, dev, T, want):
    with ops.kernel_policy(moe_tile_rows=32, moe_tile_rows_q=rows_q, moe_tile_mx=knob):
        assert ops.moe_uses_mx(T, K, E, fmt, torch.device(dev)) is want


def test_policy_override_round_trip():
    assert KernelPolicy().moe_tile_mx is False
    on = KernelPolicy().with_overrides("moe_tile_rows_q=32,moe_tile_mx=1")
    assert on.moe_tile_mx is True and on.moe_tile_rows_q == 32
    assert on.with_overrides("moe_tile_mx=0") == KernelPolicy(moe_tile_rows_q=32)
