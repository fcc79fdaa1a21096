"""The tile-GEMM switch for quantised experts without a GPU: the ``moe_tile_rows_q`` policy field
and its refusals, ``ops.moe_uses_tiles`` per weight format at the exact threshold, and the CPU
path ignoring the field.  The kernels (csrc/kernels/moe_tile.hip, fp8 and MXFP4 instantiations)
are pinned by tests/test_moe_tile_q_gpu.py."""
import pytest
import torch

from distributed_llm_inference import ops
from distributed_llm_inference.config import KernelPolicy

BF = torch.bfloat16


def test_policy_field_default_parse_and_refusals():
    assert KernelPolicy().moe_tile_rows_q == 0
    assert KernelPolicy().with_overrides("moe_tile_rows_q=64").moe_tile_rows_q == 64
    assert KernelPolicy(moe_tile_rows_q=32).moe_tile_rows_q == 32
    assert KernelPolicy(moe_tile_rows_q=1024).moe_tile_rows_q == 1024
    for bad in (16, 2048, 31, 1025, -64):
        with pytest.raises(ValueError, match="moe_tile_rows_q"):
            KernelPolicy(moe_tile_rows_q=bad)
        with pytest.raises(ValueError, match="moe_tile_rows_q"):
            KernelPolicy().with_overrides(f"moe_tile_rows_q={bad}")
    # the two knobs are set and refused independently
    p = KernelPolicy().with_overrides("moe_tile_rows=128,moe_tile_rows_q=64")
    assert (p.moe_tile_rows, p.moe_tile_rows_q) == (128, 64)
    assert KernelPolicy(moe_tile_rows_q=64).moe_tile_rows == 0
    assert KernelPolicy(moe_tile_rows=64).moe_tile_rows_q == 0


def test_predicate_per_weight_format():
    cuda, cpu = torch.device("cuda:0"), torch.device("cpu")
    assert ops.policy().moe_tile_rows_q == 0
    for fmt in ("bf16", "fp8", "mxfp4"):
        assert not ops.moe_uses_tiles(4096, 2, 8, fmt, cuda)             # both fields 0: never
    with ops.kernel_policy(moe_tile_rows_q=64):
        for fmt in ("fp8", "mxfp4"):
            assert ops.moe_uses_tiles(256, 2, 8, fmt, cuda)              # 512 pairs = 64 x 8
            assert not ops.moe_uses_tiles(255, 2, 8, fmt, cuda)          # 510 pairs
            assert ops.moe_uses_tiles(1024, 8, 128, fmt, "cuda")
            assert not ops.moe_uses_tiles(1023, 8, 128, fmt, "cuda")
            assert not ops.moe_uses_tiles(4096, 2, 8, fmt, cpu)
            assert not ops.moe_uses_tiles(4096, 2, 8, fmt, torch.zeros(1).device)
        assert not ops.moe_uses_tiles(4096, 2, 8, "bf16", cuda)          # bf16 ignores the field
    with ops.kernel_policy(moe_tile_rows=64):                            # ... and they ignore bf16's
        assert ops.moe_uses_tiles(256, 2, 8, "bf16", cuda)
        for fmt in ("fp8", "mxfp4"):
            assert not ops.moe_uses_tiles(4096, 2, 8, fmt, cuda)
    with ops.kernel_policy(moe_tile_rows=128, moe_tile_rows_q=32):       # each its own threshold
        assert not ops.moe_uses_tiles(256, 2, 8, "bf16", cuda)
        assert ops.moe_uses_tiles(512, 2, 8, "bf16", cuda)
        assert ops.moe_uses_tiles(128, 2, 8, "fp8", cuda)
        assert not ops.moe_uses_tiles(127, 2, 8, "mxfp4", cuda)
    assert not ops.moe_uses_tiles(256, 2, 8, "fp8", cuda)


def _quantised_inputs():
    g = torch.Generator().manual_seed(5)
    T, E, k, H, I = 256, 8, 2, 128, 128
    x = torch.randn(T, H, generator=g).to(BF)
    logits = torch.randn(T, E, generator=g).to(BF)
    wgu = (torch.randn(E, 2 * I, H, generator=g) / H ** 0.5).to(BF)
    wd = (torch.randn(E, H, I, generator=g) / I ** 0.5).to(BF)
    return T, E, k, x, logits, wgu, wd


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
def test_cpu_path_ignores_the_policy(fmt):
    T, E, k, x, logits, wgu, wd = _quantised_inputs()
    if fmt == "fp8":
        (qgu, sgu), (qd, sd) = ops.quantize_expert_weights_fp8(wgu), ops.quantize_expert_weights_fp8(wd)
        one = dict(w_scale=sgu)
    else:
        (qgu, sgu), (qd, sd) = (ops.quantize_expert_weights_mxfp4(wgu),
                                ops.quantize_expert_weights_mxfp4(wd))
        one = dict(w_block_scale=sgu)
    gate_up, down = ops.ExpertWeights(qgu, sgu), ops.ExpertWeights(qd, sd)
    base = ops.moe_mlp(x, logits, gate_up, down, k, True)
    with ops.kernel_policy(moe_tile_rows_q=64):
        assert T * k >= 64 * E and not ops.moe_uses_tiles(T, k, E, fmt, x.device)
        got = ops.moe_mlp(x, logits, gate_up, down, k, True)
        r = ops.moe_route(logits, k, True)
        forced = ops.moe_grouped_gemm(x, qgu, r, tiles=True, **one)   # the CPU path ignores `tiles`
    assert torch.equal(got.view(torch.int16), base.view(torch.int16))
    assert float(base.float().abs().max()) > 0.05
    assert torch.equal(forced.view(torch.int16),
                       ops.moe_grouped_gemm(x, qgu, r, tiles=False, **one).view(torch.int16))


def test_forcing_tiles_on_quantised_weights_needs_the_policy(monkeypatch):
    """``tiles=True`` with fp8 or MXFP4 weights on the GPU path is refused while the field is 0,
    before anything native is touched, and passes the front end's check once it is set (the
    device test is replaced so that the refusal can be seen without a GPU)."""
    T, E, k, x, logits, wgu, _ = _quantised_inputs()
    w8, s8 = ops.quantize_expert_weights_fp8(wgu)
    w4, s4 = ops.quantize_expert_weights_mxfp4(wgu)
    r = ops.moe_route(logits, k, True)
    assert ops.policy().moe_tile_rows_q == 0
    monkeypatch.setattr(ops, "_gpu", lambda t: True)

    class Reached(Exception):
        pass

    def native():
        raise Reached

    monkeypatch.setattr(ops, "native", native)
    with pytest.raises(ValueError, match="tiles=True needs bf16 expert weights"):
        ops.moe_grouped_gemm(x, w8, r, w_scale=s8, tiles=True)
    with pytest.raises(ValueError, match="tiles=True needs bf16 expert weights"):
        ops.moe_grouped_gemm(x, w4, r, w_block_scale=s4, tiles=True)
    with ops.kernel_policy(moe_tile_rows=64):                            # bf16's knob does not help
        with pytest.raises(ValueError, match="tiles=True needs bf16 expert weights"):
            ops.moe_grouped_gemm(x, w8, r, w_scale=s8, tiles=True)
    with ops.kernel_policy(moe_tile_rows_q=64):
        with pytest.raises(Reached):
            ops.moe_grouped_gemm(x, w8, r, w_scale=s8, tiles=True)
        with pytest.raises(Reached):
            ops.moe_grouped_gemm(x, w4, r, w_block_scale=s4, tiles=True)
