"""128 x 128 block-scaled FP8 checkpoints (HF quant_method "fp8") and the "fp8_block" expert
format on the CPU: a synthetic Qwen3-MoE layer written with safetensors loads byte for byte,
computes what its dequantised bf16 twin computes, round-trips, and the refusals."""
import json
import os

import pytest
import torch
from safetensors.torch import save_file

from distributed_llm_inference import ops
from distributed_llm_inference.config import ModelSpec
from distributed_llm_inference.models.stage import make_block
from distributed_llm_inference.utils.model import load_block

BF, FP8 = torch.bfloat16, torch.float8_e4m3fn
ATOL, RTOL = 2e-2, 2e-2      # tests/test_moe_fp8_gpu.py's oracle tolerance
E, H, I = 4, 256, 128
QCFG = dict(quant_method="fp8", fmt="e4m3", activation_scheme="dynamic",
            weight_block_size=[128, 128])


def _spec(**kw):
    return ModelSpec(name="moe-f8", model_type="qwen3_moe", qk_norm=True, vocab_size=512,
                     hidden_size=H, intermediate_size=512, num_layers=1, num_heads=2,
                     num_kv_heads=1, head_dim=128, rms_norm_eps=1e-6, rope_theta=10000.0,
                     max_position_embeddings=4096, bos_token_id=1, eos_token_id=2,
                     num_experts=E, num_experts_per_tok=2, moe_intermediate_size=I,
                     norm_topk_prob=True, **kw)


def _full(s):
    return s.repeat_interleave(128, 0).repeat_interleave(128, 1)


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    """Two directories holding one layer: `f8` as the hub writes block-scaled FP8 (every
    projection e4m3 with weight_scale_inv; router and norms bf16), `bf` its explicit
    dequantisation bf16(w8 * scale); plus the raw tensors."""
    root = tmp_path_factory.mktemp("ckpt")
    sd = make_block(_spec(), [0]).init_random(3).layers[0].hf_state_dict()
    g = torch.Generator().manual_seed(1)
    f8, bf = {}, {}
    for k, w in sd.items():
        if k.endswith("_proj.weight"):
            n, m = w.shape
            w = w * 4 if "experts" in k else w            # unit-scale expert products
            s = (torch.rand(n // 128, m // 128, generator=g) + 1) * w.float().abs().max() / 448
            w8 = (w.float() / _full(s)).to(FP8)
            f8[k], f8[k + "_scale_inv"] = w8, s
            bf[k] = (w8.float() * _full(s)).to(BF)
        else:
            f8[k] = bf[k] = w.clone()
    for name, tensors, q in (("f8", f8, QCFG), ("bf", bf, None)):
        os.makedirs(root / name)
        save_file({"model.layers.0." + k: v.contiguous() for k, v in tensors.items()},
                  str(root / name / "model.safetensors"))
        cfg = _spec().to_hf_dict()
        if q:
            cfg["quantization_config"] = q
        (root / name / "config.json").write_text(json.dumps(cfg))
    return root, f8, bf


def test_block_fp8_checkpoint_loads_bytes_and_scales_and_matches_its_bf16_twin(ckpt):
    root, f8, bf = ckpt
    lq = load_block(str(root / "f8"), [0]).layers[0]          # no flag: the experts stay fp8
    lb = load_block(str(root / "bf"), [0]).layers[0]
    m = lq.mlp
    assert m.is_fp8_block and not lb.mlp.is_fp8
    gu, dn = m.experts("w_gate_up"), m.experts("w_down")
    assert gu.format == dn.format == "fp8_block"
    assert gu.scale.shape == (E, 2 * I // 16, H // 128)
    assert dn.scale.shape == (E, H // 16, I // 128)
    for e in range(E):
        pre = f"mlp.experts.{e}."
        keys = [pre + n + "_proj.weight" for n in ("gate", "up", "down")]
        g8, u8, d8 = (f8[k] for k in keys)
        gs, us, ds = (_full(f8[k + "_scale_inv"]) for k in keys)
        assert torch.equal(gu.w[e].view(torch.uint8),
                           ops.swiglu_interleave(torch.cat([g8, u8]).view(torch.uint8)))
        assert torch.equal(ops.reference.expand_fp8_block_scale(gu.scale[e]),
                           ops.swiglu_interleave(torch.cat([gs, us])))
        assert torch.equal(dn.w[e].view(torch.uint8), d8.view(torch.uint8))
        assert torch.equal(ops.reference.expand_fp8_block_scale(dn.scale[e]), ds)
    # everything else is the bf16 twin's, bit for bit; the experts round-trip to it
    assert torch.equal(lq.self_attn.qkv_proj.weight, lb.self_attn.qkv_proj.weight)
    assert torch.equal(lq.self_attn.o_proj.weight, lb.self_attn.o_proj.weight)
    back = m.hf_dict()
    assert all(torch.equal(back[k], bf[k]) for k in bf if k.startswith("mlp."))
    x = torch.randn(24, H, generator=torch.Generator().manual_seed(2)).to(BF)
    with torch.no_grad():
        got, want = m(x), lb.mlp(x)
    err = (got.float() - want.float()).abs()
    assert want.float().abs().max() > 0.5
    assert bool((err <= ATOL + RTOL * want.float().abs()).all()), err.max()
    # "bf16" dequantises the experts as well
    ld = load_block(str(root / "f8"), [0], use_quantized="bf16").layers[0]
    assert torch.equal(ld.mlp.w_gate_up, lb.mlp.w_gate_up) and not ld.mlp.is_fp8


def test_fp8_block_format_quantiser_and_refusals(ckpt):
    root, f8, _ = ckpt
    w = torch.randn(2, 256, 256, generator=torch.Generator().manual_seed(4)).to(BF)
    rows, blk = ops.ExpertWeights.quantize(w, "fp8"), ops.ExpertWeights.quantize(w, "fp8_block")
    assert (rows.format, blk.format) == ("fp8", "fp8_block") and blk.scale.shape == (2, 16, 2)
    amax = w.float().reshape(2, 16, 16, 2, 128).abs().amax((2, 4))
    assert torch.equal(blk.scale, amax / 448)
    assert (blk.dequantize(1).float() - w[1].float()).abs().max() <= amax[1].max() / 16
    r = ops.moe_route(torch.randn(8, 2).to(BF), 1, False)
    with pytest.raises(ValueError, match="mx=True"):
        ops.moe_grouped_gemm(torch.zeros(8, 256, dtype=BF), blk, r, down=True, mx=True)
    with pytest.raises(ValueError, match="fp8_experts"):       # a second quantising mode
        load_block(str(root / "f8"), [0], use_quantized="fp8_experts")
    with pytest.raises(ValueError, match="weight_block_size"):
        ModelSpec.from_hf_config(dict(_spec().to_hf_dict(),
                                      quantization_config=dict(QCFG, weight_block_size=[64, 64])))
    bad = dict(f8)
    key = "mlp.experts.1.up_proj.weight_scale_inv"
    bad[key] = torch.ones(2, 2)
    with pytest.raises(ValueError, match="weight_scale_inv"):
        make_block(_spec(weight_quant="fp8_block"), [0]).layers[0].load_hf_state_dict(bad)
