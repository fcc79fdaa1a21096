"""The "fp8_block" mode on the CPU: a synthetic 128 x 128 block-scaled FP8 layer (dense, and
sparse with a shared expert) keeps its stored bytes under the mode and loads as today without it;
plan's byte count."""
import json

import pytest
import torch

from distributed_llm_inference import cli, ops
from distributed_llm_inference.config import ModelSpec, resolve_model
from distributed_llm_inference.models.stage import make_block
from distributed_llm_inference.ops.reference import expand_fp8_block_scale

BF, FP8 = torch.bfloat16, torch.float8_e4m3fn
BASE = dict(vocab_size=512, hidden_size=256, intermediate_size=512, num_layers=1, num_heads=8,
            num_kv_heads=2, head_dim=32, rope_theta=10000.0, max_position_embeddings=4096)
SPECS = {
    "dense": ModelSpec(name="d", model_type="qwen3", qk_norm=True, **BASE),
    "shared": ModelSpec(name="s", model_type="qwen2_moe", attention_bias=True, num_experts=4,
                        num_experts_per_tok=2, moe_intermediate_size=128,
                        shared_expert_intermediate_size=256, **BASE),
}


def _full(s, rows):
    return s.repeat_interleave(128, 0)[:rows].repeat_interleave(128, 1)


def _checkpoint_layer(spec):
    """One layer as the hub writes block-scaled FP8: every projection e4m3fn with its
    weight_scale_inv [ceil(out / 128), in / 128], the rest bf16.  Also the fp32 products
    w8 * scale that dequantize_fp8_block_weight forms before its rounding."""
    sd = make_block(spec, [0]).init_random(3).layers[0].hf_state_dict()
    g = torch.Generator().manual_seed(1)
    f8, prod = {}, {}
    for k, w in sd.items():
        if k.endswith("_proj.weight"):
            n, m = w.shape
            s = (torch.rand((n + 127) // 128, m // 128, generator=g) + 1) * w.float().abs().max() / 448
            f8[k], f8[k + "_scale_inv"] = (w.float() / _full(s, n)).to(FP8), s
            prod[k] = f8[k].float() * _full(s, n)
        else:
            f8[k] = w.clone()
    return f8, prod


@pytest.mark.parametrize("kind", ["dense", "shared"])
@pytest.mark.parametrize("fused", [False, True])
def test_mode_keeps_stored_bytes_and_default_is_unchanged(kind, fused):
    spec = SPECS[kind]
    f8, prod = _checkpoint_layer(spec)
    kept, plain = (make_block(spec, [0]).layers[0] for _ in range(2))
    mlp = lambda layer: layer.mlp.shared_expert if kind == "shared" else layer.mlp
    for layer in (kept, plain):
        mlp(layer).set_fused_swiglu(fused)
    kept.load_hf_state_dict(dict(f8), keep_fp8_block=True)
    plain.load_hf_state_dict(dict(f8))
    pre = "mlp.shared_expert." if kind == "shared" else "mlp."
    perm = ops.swiglu_interleave if fused else (lambda t: t)
    groups = {
        "qkv": (kept.self_attn.qkv_proj, plain.self_attn.qkv_proj,
                [f"self_attn.{n}_proj.weight" for n in "qkv"], lambda t: t),
        "o": (kept.self_attn.o_proj, plain.self_attn.o_proj, ["self_attn.o_proj.weight"],
              lambda t: t),
        "gate_up": (mlp(kept).gate_up_proj, mlp(plain).gate_up_proj,
                    [pre + "gate_proj.weight", pre + "up_proj.weight"], perm),
        "down": (mlp(kept).down_proj, mlp(plain).down_proj, [pre + "down_proj.weight"],
                 lambda t: t),
    }
    for name, (lin, ref, keys, p) in groups.items():
        assert lin.is_fp8_block and not lin.is_fp8 and lin.weight.numel() == 0, name
        assert lin.weight_fp8_block_scale.shape == (lin.out_features // 16, lin.in_features // 128)
        assert torch.equal(lin.weight_fp8_block.view(torch.uint8),
                           p(torch.cat([f8[k].view(torch.uint8) for k in keys])))
        want = p(torch.cat([prod[k] for k in keys]))
        assert torch.equal(lin.weight_fp8_block.float()
                           * expand_fp8_block_scale(lin.weight_fp8_block_scale), want), name
        # without the mode: today's bf16 weights, one rounding of the same product
        assert not ref.is_fp8_block and torch.equal(ref.weight, want.to(BF)), name
    if kind == "shared":   # the routed experts hold their stored bytes either way
        assert kept.mlp.is_fp8_block and plain.mlp.is_fp8_block
        assert torch.equal(kept.mlp.w_gate_up.view(torch.uint8),
                           plain.mlp.w_gate_up.view(torch.uint8))
    # the kept layer computes what the op's oracle computes from those bytes
    x = torch.randn(5, 256, generator=torch.Generator().manual_seed(2)).to(BF)
    lin = kept.self_attn.qkv_proj
    want = x.float() @ torch.cat([prod[k] for k in groups["qkv"][2]]).t()
    if lin.bias is not None:
        want = want + lin.bias.float()
    assert torch.equal(lin(x), want.to(BF))


def test_quantize_mode_on_bf16_weights_and_odd_shapes():
    """On bf16 weights the mode is ops.quantize_expert_weights_fp8_block with E = 1; a Linear
    whose sides are not multiples of 128 stays bf16."""
    block = make_block(SPECS["dense"], [0]).init_random(3)
    w = block.layers[0].self_attn.o_proj.weight.clone()
    from distributed_llm_inference.models.stage import apply_quantization
    apply_quantization(block, "fp8_block")
    lin = block.layers[0].self_attn.o_proj
    w8, s = ops.quantize_expert_weights_fp8_block(w[None])
    assert torch.equal(lin.weight_fp8_block.view(torch.uint8), w8[0].view(torch.uint8))
    assert torch.equal(lin.weight_fp8_block_scale, s[0])
    from distributed_llm_inference.models.common import Linear
    odd = Linear(128, 192)
    assert odd.quantize_fp8_block() is False and not odd.is_fp8_block and odd.weight.numel()


def test_plan_counts_one_byte_and_a_scale_share(capsys):
    def plan(*flags):
        assert cli.main(["plan", "--model", "qwen3-32b", "--gpus", "1", *flags]) == 0
        return json.loads(capsys.readouterr().out)
    spec = resolve_model("qwen3-32b")
    bf, f8 = plan(), plan("--fp8-block")
    assert f8["weight_bytes_per_param"] == 1 + 4 / 2048
    emb = 2 * spec.vocab_size * spec.hidden_size * 2
    layers = spec.num_layers * int(spec.layer_param_count() * (1 + 4 / 2048))
    assert f8["stages"][0]["weights_gb"] == round((layers + emb) / 1e9, 2)
    assert f8["stages"][0]["weights_gb"] < 0.55 * bf["stages"][0]["weights_gb"]
    assert f8["stages"][0]["kv_capacity_tokens"] > bf["stages"][0]["kv_capacity_tokens"]
