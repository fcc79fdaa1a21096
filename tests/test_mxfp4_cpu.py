"""MXFP4 weights (OCP MX: e2m1 elements, one e8m0 scale per 32) on the CPU: the quantiser / the
dequantiser (the oracle of the GPU kernels), Linear, a stage, and the CLI."""
import io
import json
from contextlib import redirect_stdout

import pytest
import torch
import torch.nn.functional as F

from distributed_llm_inference import cli, ops
from distributed_llm_inference.config import ModelSpec
from distributed_llm_inference.models import CausalLMStage
from distributed_llm_inference.models.common import Linear
from distributed_llm_inference.ops import reference as ref

BF = torch.bfloat16
GRID = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]

# tests/test_engine_gpu.py's SPEC
SPEC = ModelSpec(name="t", vocab_size=1000, hidden_size=256, intermediate_size=512, num_layers=4,
                 num_heads=8, num_kv_heads=2, head_dim=32, rope_theta=10000.0,
                 max_position_embeddings=4096)

# relative logits error of the MXFP4 stage against the bf16 stage (SPEC, seed 9, prefill of
# tokens 1..49 on the CPU), as measured when the mode was added (docs/kernels.md quotes it)
STAGE_REL_ERR = 0.2898


def _wide_weight(n, k, seed):
    """Random weights whose per-block magnitudes span 2^-20 .. 2^10."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, k // 32, 32, generator=g)
    ex = torch.randint(-20, 11, (n, k // 32, 1), generator=g).float()
    return (w * torch.exp2(ex)).reshape(n, k)


def _nibbles(packed):
    return torch.stack([packed & 0xF, packed >> 4], -1).reshape(packed.shape[0], -1)


@pytest.mark.parametrize("s", [-9, -1, 0, 3, 10])
def test_grid_values_round_trip_exactly(s):
    vals = torch.tensor(GRID + [-v for v in GRID] + GRID + [-v for v in GRID]) * 2.0 ** s
    packed, scales = ops.quantize_weight_mxfp4(vals.reshape(1, 32))
    assert scales.tolist() == [[127 + s]]            # amax = 6 * 2^s: e = s + 2 - 2
    nib = _nibbles(packed)[0].tolist()
    assert nib[:8] == list(range(8)) and nib[9:16] == list(range(9, 16))
    assert nib[8] == 0                               # -0 is stored as +0
    deq = ops.dequantize_mxfp4(packed, scales)
    assert deq.dtype == BF and torch.equal(deq.float(), vals.reshape(1, 32))


@pytest.mark.parametrize("s", [-7, 0, 5])
def test_ties_round_to_even_mantissa_and_saturate(s):
    sc = 2.0 ** s
    # amax 6 -> unit scale 2^s; ties: 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2,
    # 3.5 -> 4, 5 -> 4 (the neighbour whose mantissa bit is 0)
    src = [6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -2.5, -3.5, -5.0, 2.6, 2.4, 0.2, 0.3]
    want = [6.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, -2.0, -4.0, -4.0, 3.0, 2.0, 0.0, 0.5]
    w = torch.zeros(1, 32)
    w[0, :len(src)] = torch.tensor(src) * sc
    deq = ops.dequantize_mxfp4(*ops.quantize_weight_mxfp4(w)).float()
    assert deq[0, :len(src)].tolist() == [v * sc for v in want]
    # amax = 7.9 * 2^s: e = s, and 7.9 saturates to 6 (both signs)
    w = torch.zeros(1, 32)
    w[0, 0], w[0, 1], w[0, 2] = 7.9 * sc, -7.9 * sc, 5.1 * sc
    packed, scales = ops.quantize_weight_mxfp4(w)
    assert scales.tolist() == [[127 + s]]
    assert ops.dequantize_mxfp4(packed, scales).float()[0, :3].tolist() == [6 * sc, -6 * sc, 6 * sc]


def test_zero_block_and_bad_inputs():
    w = torch.zeros(2, 64)
    w[1, 40] = 1.0
    packed, scales = ops.quantize_weight_mxfp4(w)
    assert scales[0].tolist() == [127, 127] and scales[1, 0].item() == 127
    assert int(packed[0].sum()) == 0 and int(packed[1, :16].sum()) == 0
    for bad in (float("nan"), float("inf"), float("-inf")):
        w2 = w.clone()
        w2[0, 3] = bad
        with pytest.raises(ValueError):
            ops.quantize_weight_mxfp4(w2)
    with pytest.raises(ValueError):
        ops.quantize_weight_mxfp4(torch.zeros(4, 48))
    packed, scales = ops.quantize_weight_mxfp4(torch.randn(3, 96).to(BF))
    assert packed.shape == (3, 48) and packed.dtype == torch.uint8
    assert scales.shape == (3, 3) and scales.dtype == torch.uint8


def test_quantiser_properties_wide_range():
    w = _wide_weight(96, 256, 1)
    packed, scales = ops.quantize_weight_mxfp4(w)
    deq = ops.dequantize_mxfp4(packed, scales)
    assert int(scales.min()) >= 1 and int(scales.max()) <= 254
    # on the grid: |deq| / 2^(scale - 127) is one of the 8 magnitudes
    unit = torch.exp2(scales.float() - 127).repeat_interleave(32, dim=1)
    mag = (deq.float().abs() / unit).reshape(-1)
    assert set(mag.tolist()) <= set(GRID)
    # idempotent
    p2, s2 = ops.quantize_weight_mxfp4(deq)
    assert torch.equal(p2, packed) and torch.equal(s2, scales)
    # per block: max |w - deq| <= amax / 4
    err = (w - deq.float()).abs().reshape(96, 8, 32).amax(-1)
    amax = w.abs().reshape(96, 8, 32).amax(-1)
    assert bool((err <= amax / 4).all()), (err / amax).max().item()
    # chunked processing changes nothing (rows are independent)
    big = _wide_weight(300, 8192 * 8, 2)      # > one 2^24-element chunk
    pb, sb = ops.quantize_weight_mxfp4(big)
    pr, sr = ops.quantize_weight_mxfp4(big[255:258])
    assert torch.equal(pb[255:258], pr) and torch.equal(sb[255:258], sr)
    assert torch.equal(ops.dequantize_mxfp4(pb, sb)[255:258], ops.dequantize_mxfp4(pr, sr))


def test_swiglu_interleave_commutes_with_quantisation():
    w = _wide_weight(512, 128, 3).to(BF)
    p1, s1 = ops.quantize_weight_mxfp4(ops.swiglu_interleave(w))
    p0, s0 = ops.quantize_weight_mxfp4(w)
    assert torch.equal(p1, ops.swiglu_interleave(p0)) and torch.equal(s1, ops.swiglu_interleave(s0))


def test_linear_mxfp4_cpu_is_the_bf16_path_on_the_dequantised_weight():
    torch.manual_seed(4)
    lin = Linear(128, 72, bias=True)
    lin.weight.data.copy_(_wide_weight(72, 128, 5).to(BF) * 0.01)
    lin.bias.data.copy_(torch.randn(72).to(BF))
    w0 = lin.weight.data.clone()
    lin.quantize_mxfp4()
    assert lin.is_fp4 and not lin.is_fp8 and not lin.is_int8 and lin.weight.numel() == 0
    assert lin.weight_fp4.shape == (72, 64) and lin.weight_block_scale.shape == (72, 4)
    assert "fp4=True" in lin.extra_repr()
    wd = ops.dequantize_mxfp4(*ops.quantize_weight_mxfp4(w0))
    assert torch.equal(lin.dense_weight(), wd)
    for shape in ((1, 128), (5, 128), (2, 3, 128)):
        x = torch.randn(*shape).to(BF)
        assert torch.equal(lin(x), F.linear(x, wd, lin.bias))
    assert lin.stream_weights()[0] is lin.weight_fp4
    keep = Linear(64, 8)
    keep.weight.data.normal_()
    keep.quantize_mxfp4(keep_bf16=True)
    assert keep.weight.numel() == 64 * 8 and keep.is_fp4
    with pytest.raises(ValueError):
        Linear(48, 8).quantize_mxfp4()


def test_skinny_gemm_fp4_cpu_reference():
    torch.manual_seed(6)
    I, K = 128, 64
    w = ops.swiglu_interleave((torch.randn(2 * I, K) * 0.05).to(BF))
    packed, scales = ops.quantize_weight_mxfp4(w)
    wd = ops.dequantize_mxfp4(packed, scales).float()
    x = torch.randn(2, K).to(BF)
    bias = torch.randn(2 * I).to(BF)
    y = ops.skinny_gemm_fp4(x, packed, scales, bias)
    assert torch.equal(y, (x.float() @ wd.t() + bias.float()).to(BF))
    h = ops.skinny_gemm_fp4(x, packed, scales, swiglu=True)
    assert torch.equal(h, ops.swiglu_interleaved((x.float() @ wd.t()).to(BF)))
    nw = (1 + 0.1 * torch.randn(K)).to(BF)
    yn = ops.skinny_gemm_fp4(x, packed, scales, norm=ops.RowNorm(nw, 1e-5))
    assert torch.equal(yn, ops.skinny_gemm_fp4(ops.rms_norm(x, nw, 1e-5)[0], packed, scales))


def _prefill_logits(stage, prompts):
    pool = stage.make_pool(16, block_size=64)
    sids = list(range(len(prompts)))
    for s, p in zip(sids, prompts):
        pool.manager.append(s, len(p))
    meta = pool.build_metadata(sids, [len(p) for p in prompts])
    meta.logits_rows = torch.cumsum(torch.tensor([len(p) for p in prompts]), 0) - 1
    ids = torch.tensor([t for p in prompts for t in p], dtype=torch.int32)
    return stage(ids, meta, pool).float()


def test_stage_mxfp4_prefill_on_cpu_close_to_bf16():
    """Relative logits error of the MXFP4 stage against the bf16 stage: the measured value
    (STAGE_REL_ERR) with a 25 % margin for torch-version differences in fp32 accumulation."""
    stage = CausalLMStage(SPEC, 0, 4).init_random(9)
    prompts = [list(range(1, 50))]
    a = _prefill_logits(stage, prompts)
    assert stage.quantize("mxfp4") is stage
    lins = [m for m in stage.block.modules() if isinstance(m, Linear)]
    assert len(lins) == 16 and all(m.is_fp4 and m.weight.numel() == 0 for m in lins)
    assert stage.head.proj is None or not stage.head.proj.is_fp4   # the LM head stays bf16
    b = _prefill_logits(stage, prompts)
    rel = ((a - b).norm() / a.norm()).item()
    print(f"mxfp4 vs bf16 relative logits error: {rel:.4f}")
    assert 0.0 < rel < 1.25 * STAGE_REL_ERR, rel
    # the alias and the named method give the same weights
    s2 = CausalLMStage(SPEC, 0, 4).init_random(9).quantize("fp4")
    s3 = CausalLMStage(SPEC, 0, 4).init_random(9).quantize_mxfp4()
    for m1, m2, m3 in zip(lins, (m for m in s2.block.modules() if isinstance(m, Linear)),
                          (m for m in s3.block.modules() if isinstance(m, Linear))):
        assert torch.equal(m1.weight_fp4, m2.weight_fp4) and torch.equal(m1.weight_fp4, m3.weight_fp4)
        assert torch.equal(m1.weight_block_scale, m2.weight_block_scale)


def test_fused_swiglu_order_on_mxfp4_weights_cpu():
    """set_fused_swiglu permutes the nibble rows and their scale rows: same MLP output."""
    stage = CausalLMStage(SPEC.replace(num_layers=1), 0, 1).init_random(2).quantize("mxfp4")
    mlp = stage.block.layers[0].mlp
    x = (torch.randn(3, SPEC.hidden_size) * 0.5).to(BF)
    y0 = mlp(x)
    p0 = mlp.gate_up_proj.weight_fp4.clone()
    stage.block.set_fused_swiglu(True)
    assert mlp.fused_swiglu and not torch.equal(mlp.gate_up_proj.weight_fp4, p0)
    assert torch.equal(mlp(x), y0)
    stage.block.set_fused_swiglu(False)
    assert torch.equal(mlp.gate_up_proj.weight_fp4, p0)


def test_unknown_mode_and_gpt2_raise():
    stage = CausalLMStage(SPEC, 0, 1).init_random(0)
    with pytest.raises(ValueError, match="mxfp4"):
        stage.quantize("fp5")
    gpt2 = ModelSpec(name="g", arch="gpt2", vocab_size=100, hidden_size=64, intermediate_size=256,
                     num_layers=1, num_heads=4, num_kv_heads=4, head_dim=16,
                     max_position_embeddings=128)
    with pytest.raises(NotImplementedError, match="MXFP4"):
        CausalLMStage(gpt2, 0, 1).init_random(0).quantize("mxfp4")


def _plan(argv):
    buf = io.StringIO()
    with redirect_stdout(buf):
        assert cli.main(["plan", "--model", "llama-3-70b", "--gpus", "1"] + argv) == 0
    return json.loads(buf.getvalue())


def test_cli_fp4_flag_and_plan():
    import argparse
    ap = argparse.ArgumentParser()
    cli._common(ap)
    a = ap.parse_args(["--fp4"])
    assert a.fp4 and not a.fp8 and not a.int8
    assert cli.engine_config(a).quantize == "mxfp4"
    assert cli.engine_config(ap.parse_args(["--fp8"])).quantize == "fp8"
    assert cli.engine_config(ap.parse_args([])).quantize is False
    for both in (["--fp4", "--fp8"], ["--fp4", "--int8"]):
        with pytest.raises(SystemExit):
            ap.parse_args(both)
    fp4, fp8, bf16 = _plan(["--fp4"]), _plan(["--fp8"]), _plan([])
    assert fp4["weight_bytes_per_param"] == 17 / 32
    assert fp8["weight_bytes_per_param"] == 1 and bf16["weight_bytes_per_param"] == 2
    s4, s8 = fp4["stages"][0], fp8["stages"][0]
    assert s4["weights_gb"] < s8["weights_gb"] < bf16["stages"][0]["weights_gb"]
    assert s4["kv_capacity_tokens"] > s8["kv_capacity_tokens"]
    spec = __import__("distributed_llm_inference.config", fromlist=["resolve_model"]).resolve_model(
        "llama-3-70b")
    layers = spec.num_layers * spec.layer_param_count()
    assert abs((s8["weights_gb"] - s4["weights_gb"]) * 1e9 - layers * 15 / 32) < 0.02e9
