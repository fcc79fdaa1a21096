"""fp8 expert weights for sparse-MoE models on the CPU reference path: the per-expert quantiser,
the rounding points of ops.moe_mlp with row scales, the "fp8_experts" mode at module / block /
stage level, what it must leave alone, its refusals, the CLI flag and the memory plan.  The kernel
is pinned by tests/test_moe_fp8_gpu.py."""
import argparse
import io
import json
from contextlib import redirect_stdout

import pytest
import torch

from distributed_llm_inference import cli, ops
from distributed_llm_inference.config import PRESETS, ModelSpec, refuse_moe_quantization
from distributed_llm_inference.models import CausalLMStage
from distributed_llm_inference.models.llama.modules import MoEMLP
from distributed_llm_inference.ops import reference as ref

BF = torch.bfloat16
FP8 = torch.float8_e4m3fn
PROMPTS = [[5, 17, 99, 3, 250, 7, 7, 1], [8, 2, 64]]


def _tiny(model_type="qwen3_moe", **kw):
    base = dict(name="tiny-moe", model_type=model_type, vocab_size=256, hidden_size=128,
                intermediate_size=256, num_layers=2, num_heads=4, num_kv_heads=2, head_dim=64,
                rms_norm_eps=1e-6, rope_theta=1000000.0, max_position_embeddings=4096,
                bos_token_id=1, eos_token_id=2, num_experts=8, num_experts_per_tok=2,
                moe_intermediate_size=128, norm_topk_prob=True, qk_norm=True)
    if model_type == "mixtral":
        base.update(qk_norm=False, intermediate_size=128, head_dim=32)
    base.update(kw)
    return ModelSpec(**base)


def _dequant(w8, scale):
    return w8.float() * scale[..., None]


# ------------------------------------------------------------------ the quantiser
def test_quantize_expert_weights_fp8():
    g = torch.Generator().manual_seed(1)
    E, N, K = 4, 96, 256
    w = (torch.randn(E, N, K, generator=g) / K ** 0.5).to(BF)
    w[1, 5] = 0                                        # an all-zero row
    w[2, 7] *= 2.0 ** -12 * torch.rand(K, generator=g).to(BF)   # a row with subnormal quotients
    w8, scale = ops.quantize_expert_weights_fp8(w)
    assert w8.shape == (E, N, K) and w8.dtype == FP8
    assert scale.shape == (E, N) and scale.dtype == torch.float32
    assert w8.is_contiguous() and scale.is_contiguous()
    assert bool(scale.isfinite().all()) and bool((scale > 0).all())
    assert bool((w8[1, 5].float() == 0).all())
    # the rule is quantize_weight_fp8's, expert by expert
    for e in range(E):
        q, s = ops.quantize_weight_fp8(w[e])
        assert torch.equal(q.view(torch.uint8), w8[e].view(torch.uint8))
        assert torch.equal(s.reshape(-1), scale[e])
    amax = w.float().abs().amax(-1)
    assert torch.equal(scale, amax.clamp_min(1e-12) / 448)
    # e4m3: a 3-bit mantissa (half an ulp <= 2^-4 of the value), smallest subnormal 2^-9
    wf = w.float()
    err = (_dequant(w8, scale) - wf).abs()
    bound = torch.maximum(2.0 ** -4 * wf.abs(), 2.0 ** -10 * scale[..., None])
    assert bool((err <= bound).all()), (err - bound).max().item()
    assert bool((_dequant(w8, scale)[2, 7] != 0).any())


# ------------------------------------------------------------------ rounding points
def test_reference_moe_mlp_with_scales_is_the_dense_definition():
    """ops.moe_mlp with fp8 weights and row scales on the CPU against the definition written out
    per token and slot in fp32 on the dequantised weights, with the bf16 path's rounding points."""
    gen = torch.Generator().manual_seed(9)
    T, H, I, E, k = 19, 128, 128, 8, 2
    x = torch.randn(T, H, generator=gen).to(BF)
    wg = (0.1 * torch.randn(E, I, H, generator=gen)).to(BF)
    wu = (0.1 * torch.randn(E, I, H, generator=gen)).to(BF)
    wd = (0.1 * torch.randn(E, H, I, generator=gen)).to(BF)
    logits = torch.randn(T, E, generator=gen).to(BF)
    w_gate_up = torch.stack([ops.swiglu_interleave(torch.cat([wg[e], wu[e]], 0)) for e in range(E)])
    gu8, sgu = ops.quantize_expert_weights_fp8(w_gate_up)
    d8, sd = ops.quantize_expert_weights_fp8(wd)
    got = ops.moe_mlp(x, logits, ops.ExpertWeights(gu8, sgu), ops.ExpertWeights(d8, sd), k, True)
    dgu = torch.stack([ops.swiglu_deinterleave(_dequant(gu8[e], sgu[e])) for e in range(E)])
    dg, du, dd = dgu[:, :I], dgu[:, I:], _dequant(d8, sd)
    ids, w = ref.moe_topk(logits, k, True)
    want = torch.zeros(T, H)
    for t in range(T):
        for s in range(k):
            e = int(ids[t, s])
            gate = (x[t].float() @ dg[e].t()).to(BF).float()
            up = (x[t].float() @ du[e].t()).to(BF).float()
            h = (torch.nn.functional.silu(gate) * up).to(BF).float()
            want[t] += w[t, s] * (h @ dd[e].t()).to(BF).float()
    assert got.dtype == BF
    assert (got.float() - want.to(BF).float()).abs().max().item() <= 2.0 ** -6 * want.abs().max().item()
    # a scale without fp8 weights, fp8 weights without a scale, a scale of the wrong shape
    r = ops.moe_route(logits, k, True)
    with pytest.raises(ValueError, match="w_scale"):
        ops.moe_grouped_gemm(x, w_gate_up, r, w_scale=sgu)
    with pytest.raises(ValueError, match="w_scale"):
        ops.moe_grouped_gemm(x, gu8, r)
    with pytest.raises(ValueError, match="w_scale"):
        ops.moe_grouped_gemm(x, gu8, r, w_scale=sgu[:, :-1])


# ------------------------------------------------------------------ model level
def _run_stage(stage, prompts, decode_steps=0):
    """Prefill all prompts as one varlen batch, then greedy-decode; returns list of logits rows."""
    pool = stage.make_pool(64, block_size=32)
    m = pool.manager
    sids = list(range(len(prompts)))
    for s, p in zip(sids, prompts):
        m.append(s, len(p))
    meta = pool.build_metadata(sids, [len(p) for p in prompts])
    meta.logits_rows = torch.cumsum(torch.tensor([len(p) for p in prompts]), 0) - 1
    ids = torch.tensor([t for p in prompts for t in p])
    logits = [stage(ids, meta, pool).float()]
    toks = logits[-1].argmax(-1)
    for _ in range(decode_steps):
        for s in sids:
            m.append(s, 1)
        meta = pool.build_metadata(sids, [1] * len(sids))
        logits.append(stage(toks.to(torch.int32), meta, pool).float())
        toks = logits[-1].argmax(-1)
    return logits


def _expert_state(stage):
    out = []
    for layer in stage.block.layers:
        m = layer.mlp
        out.append((m.w_gate_up.data, m.w_gate_up_scale, m.w_down.data, m.w_down_scale))
    return out


def _bf16_state(stage):
    """Everything the mode must leave alone."""
    sd = {k: v.clone() for k, v in stage.state_dict().items()
          if not k.endswith(("mlp.w_gate_up", "mlp.w_down"))}
    assert any(k.endswith("mlp.gate.weight") for k in sd)
    assert any(k.endswith("self_attn.qkv_proj.weight") for k in sd)
    assert any(k.endswith("input_layernorm.weight") for k in sd)
    assert any(k.startswith("embed.") for k in sd) and any(k.startswith("head.") for k in sd)
    return sd


@pytest.mark.parametrize("model_type", ["qwen3_moe", "mixtral"])
def test_fp8_experts_mode_at_block_and_stage_level(model_type):
    spec = _tiny(model_type)
    base = CausalLMStage(spec, 0, 2).init_random(7)
    before = _bf16_state(base)
    stages = [CausalLMStage(spec, 0, 2).init_random(7) for _ in range(3)]
    assert stages[0].quantize_experts_fp8() is stages[0]
    assert stages[1].block.quantize_experts_fp8() is stages[1].block
    assert stages[2].quantize("fp8_experts") is stages[2]
    for li, layer in enumerate(stages[0].block.layers):
        m, b = layer.mlp, base.block.layers[li].mlp
        assert isinstance(m, MoEMLP) and m.is_fp8 and not b.is_fp8
        assert m.w_gate_up.dtype == FP8 and m.w_down.dtype == FP8
        assert m.w_gate_up.shape == b.w_gate_up.shape and m.w_down.shape == b.w_down.shape
        assert m.w_gate_up_scale.shape == (8, 256) and m.w_down_scale.shape == (8, 128)
        assert m.w_gate_up_scale.dtype == torch.float32
        w8, s = ops.quantize_expert_weights_fp8(b.w_gate_up.data)
        assert torch.equal(m.w_gate_up.view(torch.uint8), w8.view(torch.uint8))
        assert torch.equal(m.w_gate_up_scale, s)
        assert isinstance(m.gate.weight, torch.nn.Parameter) and m.gate.weight.dtype == BF
    for other in stages[1:]:
        for a, b in zip(_expert_state(stages[0]), _expert_state(other)):
            for x, y in zip(a, b):
                assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    for st in stages:                                   # router, attention, norms, embedding, head
        after = _bf16_state(st)
        assert sorted(after) == sorted(before)
        for k, v in before.items():
            assert after[k].dtype == v.dtype and torch.equal(after[k], v), k
    stages[0].quantize_experts_fp8()                     # idempotent
    assert torch.equal(stages[0].block.layers[0].mlp.w_gate_up.view(torch.uint8),
                       stages[1].block.layers[0].mlp.w_gate_up.view(torch.uint8))

    # hf_dict: the dequantised weights rounded to bf16, loadable into a bf16 stage ...
    deq = CausalLMStage(spec, 0, 2).init_random(7)
    for q, d in zip(stages[0].block.layers, deq.block.layers):
        sd = q.hf_state_dict()
        assert all(v.dtype == BF for v in sd.values())
        with torch.no_grad():
            d.load_hf_state_dict({k: v.clone() for k, v in sd.items()})
        assert torch.equal(d.mlp.w_gate_up, _dequant(q.mlp.w_gate_up, q.mlp.w_gate_up_scale).to(BF))
        assert torch.equal(d.mlp.w_down, _dequant(q.mlp.w_down, q.mlp.w_down_scale).to(BF))
        assert not torch.equal(d.mlp.w_down, base.block.layers[0].mlp.w_down)
        # ... and a quantised module does not load: quantise after loading
        with pytest.raises(RuntimeError, match="quantize_experts_fp8"):
            q.load_hf_state_dict(sd)
    # the stage on fp8 experts against the same stage on those dequantised bf16 weights
    got = _run_stage(stages[0], PROMPTS, decode_steps=1)
    want = _run_stage(deq, PROMPTS, decode_steps=1)
    for a, b in zip(got, want):
        err = (a - b).abs()
        assert bool((err <= 2e-2 + 2e-2 * b.abs()).all()), err.max().item()
    assert want[0].abs().max() > 0.1


# ------------------------------------------------------------------ refusals, CLI, plan
def test_fp8_experts_refusals():
    for name in ("tiny-llama", "tiny-gpt2"):
        spec = PRESETS[name]
        stage = CausalLMStage(spec, 0, 1).init_random(0)
        with pytest.raises(ValueError, match="fp8_experts"):
            stage.quantize("fp8_experts")
        with pytest.raises(ValueError, match="fp8_experts"):
            stage.quantize_experts_fp8()
        with pytest.raises(ValueError, match="fp8_experts"):
            refuse_moe_quantization(spec, "fp8_experts")
    for mt in ("qwen3_moe", "mixtral"):
        spec = _tiny(mt)
        refuse_moe_quantization(spec, "fp8_experts")
        for mode in ("fp8", True, "int8", "mxfp4"):
            with pytest.raises(ValueError, match="sparse MoE"):
                refuse_moe_quantization(spec, mode)
            with pytest.raises(ValueError, match="sparse MoE"):
                CausalLMStage(spec, 0, 1).init_random(0).quantize(mode)
    for name in ("qwen3-30b-a3b", "mixtral-8x7b"):
        refuse_moe_quantization(PRESETS[name], "fp8_experts")


def test_cli_fp8_experts_flag():
    ap = argparse.ArgumentParser()
    cli._common(ap)
    a = ap.parse_args(["--model", "qwen3-30b-a3b", "--fp8-experts"])
    assert a.fp8_experts and not a.fp8 and not a.int8 and not a.fp4
    assert cli.engine_config(a).quantize == "fp8_experts"
    assert cli.engine_config(ap.parse_args(["--model", "qwen3-30b-a3b"])).quantize is False
    for other in ("--fp8", "--int8", "--fp4"):
        with pytest.raises(SystemExit):
            ap.parse_args(["--fp8-experts", other])
    with pytest.raises(ValueError, match="sparse MoE"):
        cli.engine_config(ap.parse_args(["--model", "qwen3-30b-a3b", "--fp8"]))
    with pytest.raises(ValueError, match="fp8_experts"):
        cli.engine_config(ap.parse_args(["--model", "llama-3-8b", "--fp8-experts"]))


def _plan(model, argv):
    buf = io.StringIO()
    with redirect_stdout(buf):
        assert cli.main(["plan", "--model", model, "--gpus", "1"] + argv) == 0
    return json.loads(buf.getvalue())


def test_plan_fp8_experts():
    spec = PRESETS["qwen3-30b-a3b"]
    H, I, E, L = spec.hidden_size, spec.moe_intermediate_size, spec.num_experts, spec.num_layers
    assert spec.expert_param_count() == E * 3 * H * I == 604 * 1000 * 1000 - 20224
    assert PRESETS["llama-3-8b"].expert_param_count() == 0
    layer = spec.layer_param_count()
    per_layer = E * 3 * H * I + 4 * E * (2 * I + H) + 2 * (layer - E * 3 * H * I)
    emb = spec.vocab_size * H * 2
    got = _plan("qwen3-30b-a3b", ["--fp8-experts"])
    assert got["weight_bytes_per_param"] == per_layer / layer
    st = got["stages"][0]
    assert st["weights_gb"] == round((L * per_layer + 2 * emb) / 1e9, 2)
    bf16 = _plan("qwen3-30b-a3b", [])
    fp8_formula = round((L * layer + 2 * emb) / 1e9, 2)
    assert fp8_formula < st["weights_gb"] < bf16["stages"][0]["weights_gb"]
    assert st["kv_capacity_tokens"] > bf16["stages"][0]["kv_capacity_tokens"]
    # the other modes' numbers are what they were
    assert bf16["weight_bytes_per_param"] == 2
    assert bf16["stages"][0]["weights_gb"] == round((L * layer * 2 + 2 * emb) / 1e9, 2)
    d8, d4, d16 = (_plan("llama-3-70b", f) for f in (["--fp8"], ["--fp4"], []))
    dense = PRESETS["llama-3-70b"]
    demb = dense.vocab_size * dense.hidden_size * 2
    for res, per in ((d8, 1), (d4, 17 / 32), (d16, 2)):
        assert res["weight_bytes_per_param"] == per
        want = dense.num_layers * int(dense.layer_param_count() * per) + 2 * demb
        assert res["stages"][0]["weights_gb"] == round(want / 1e9, 2)
    with pytest.raises(ValueError, match="no experts"):
        _plan("llama-3-70b", ["--fp8-experts"])
