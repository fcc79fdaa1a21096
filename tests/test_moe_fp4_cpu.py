"""MXFP4 expert weights for sparse-MoE models on the CPU reference path: the per-expert quantiser,
the rounding points of ops.moe_mlp with block scales, the "mxfp4_experts" mode at module / block /
stage level, what it must leave alone, its refusals, the CLI flag and the memory plan.  The kernel
is pinned by tests/test_moe_fp4_gpu.py."""
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
U8 = torch.uint8
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


def _dequant(packed, scales):
    return torch.stack([ref.dequantize_mxfp4(packed[e], scales[e]) for e in range(packed.shape[0])])


# ------------------------------------------------------------------ the quantiser
def test_quantize_expert_weights_mxfp4():
    g = torch.Generator().manual_seed(1)
    E, N, K = 4, 96, 256
    w = (torch.randn(E, N, K, generator=g) / K ** 0.5).to(BF)
    w[1, 5] = 0                                        # an all-zero row
    w[2, 7, 32:64] *= 2.0 ** -9                        # a block far below its neighbours
    packed, scales = ops.quantize_expert_weights_mxfp4(w)
    assert packed.shape == (E, N, K // 2) and packed.dtype == U8
    assert scales.shape == (E, N, K // 32) and scales.dtype == U8
    assert packed.is_contiguous() and scales.is_contiguous()
    assert bool((packed[1, 5] == 0).all()) and bool((scales[1, 5] == 127).all())
    assert int(scales[2, 7, 1]) < int(scales[2, 7, 0]) - 6
    # the rule is quantize_weight_mxfp4's, expert by expert
    for e in range(E):
        p, s = ops.quantize_weight_mxfp4(w[e])
        assert torch.equal(p, packed[e]) and torch.equal(s, scales[e])
    # round trip: e2m1's widest step is 2 (between 4 and 6) times the block's 2^(byte - 127), and
    # amax / 2^e < 8 rounds to at most 6 + 2: half a step is 2^e, except above 6 where it
    # saturates (error < 2 * 2^e)
    deq = _dequant(packed, scales)
    assert deq.dtype == BF and deq.shape == (E, N, K)
    step = torch.exp2(scales.float() - 127).repeat_interleave(32, -1)
    wf = w.float()
    err = (deq.float() - wf).abs()
    sat = wf.abs() > 6 * step
    assert bool((err[~sat] <= step[~sat]).all()), (err - step).max().item()
    assert bool((err[sat] < 2 * step[sat]).all())
    assert bool((deq[2, 7, 32:64] != 0).any())
    with pytest.raises(ValueError, match="quantize_expert_weights_mxfp4"):
        ops.quantize_expert_weights_mxfp4(w[0])
    with pytest.raises(ValueError, match="quantize_expert_weights_mxfp4"):
        ops.quantize_expert_weights_mxfp4(w[:, :, :48])


# ------------------------------------------------------------------ rounding points
def test_reference_moe_mlp_with_block_scales_is_the_dense_definition():
    """ops.moe_mlp with MXFP4 weights and block scales on the CPU against the definition written
    out per token and slot in fp32 on the dequantised weights, with the bf16 path's rounding
    points."""
    gen = torch.Generator().manual_seed(9)
    T, H, I, E, k = 19, 128, 128, 8, 2
    x = torch.randn(T, H, generator=gen).to(BF)
    wg = (0.1 * torch.randn(E, I, H, generator=gen)).to(BF)
    wu = (0.1 * torch.randn(E, I, H, generator=gen)).to(BF)
    wd = (0.1 * torch.randn(E, H, I, generator=gen)).to(BF)
    logits = torch.randn(T, E, generator=gen).to(BF)
    w_gate_up = torch.stack([ops.swiglu_interleave(torch.cat([wg[e], wu[e]], 0)) for e in range(E)])
    gu4, sgu = ops.quantize_expert_weights_mxfp4(w_gate_up)
    d4, sd = ops.quantize_expert_weights_mxfp4(wd)
    got = ops.moe_mlp(x, logits, ops.ExpertWeights(gu4, sgu), ops.ExpertWeights(d4, sd), k, True)
    dgu = torch.stack([ops.swiglu_deinterleave(d) for d in _dequant(gu4, sgu)]).float()
    dg, du, dd = dgu[:, :I], dgu[:, I:], _dequant(d4, sd).float()
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
    err = (got.float() - want.to(BF).float()).abs().max().item()
    assert err <= 2.0 ** -6 * want.abs().max().item()
    # ... which is the bf16 path on the dequantised weights
    same = ops.moe_mlp(x, logits, _dequant(gu4, sgu), _dequant(d4, sd), k, True)
    assert torch.equal(got, same)
    # both scales, nibbles without a block scale, a block scale without nibbles, wrong shapes /
    # dtype, K % 128
    r = ops.moe_route(logits, k, True)
    with pytest.raises(ValueError, match="not both"):
        ops.moe_grouped_gemm(x, gu4, r, w_scale=torch.ones(E, 2 * I), w_block_scale=sgu)
    with pytest.raises(ValueError, match="w_block_scale"):
        ops.moe_grouped_gemm(x, gu4, r)
    with pytest.raises(ValueError, match="w_block_scale"):
        ops.moe_grouped_gemm(x, w_gate_up, r, w_block_scale=sgu)
    with pytest.raises(ValueError, match="w_block_scale"):
        ops.moe_grouped_gemm(x, gu4, r, w_block_scale=sgu[:, :, :-1])
    with pytest.raises(ValueError, match="w_block_scale"):
        ops.moe_grouped_gemm(x, gu4, r, w_block_scale=sgu[:, :-1])
    with pytest.raises(ValueError, match="w_block_scale"):
        ops.moe_grouped_gemm(x, gu4, r, w_block_scale=sgu.float())
    with pytest.raises(ValueError, match="K % 128"):
        ops.moe_grouped_gemm(x[:, :96], gu4[:, :, :48], r, w_block_scale=sgu[:, :, :3])


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
        out.append((m.w_gate_up.data, m.w_gate_up_block_scale, m.w_down.data,
                    m.w_down_block_scale))
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
def test_mxfp4_experts_mode_at_block_and_stage_level(model_type):
    spec = _tiny(model_type)
    base = CausalLMStage(spec, 0, 2).init_random(7)
    before = _bf16_state(base)
    stages = [CausalLMStage(spec, 0, 2).init_random(7) for _ in range(3)]
    assert stages[0].quantize_experts_mxfp4() is stages[0]
    assert stages[1].block.quantize_experts_mxfp4() is stages[1].block
    assert stages[2].quantize("mxfp4_experts") is stages[2]
    for li, layer in enumerate(stages[0].block.layers):
        m, b = layer.mlp, base.block.layers[li].mlp
        assert isinstance(m, MoEMLP) and m.is_mxfp4 and not m.is_fp8 and not b.is_mxfp4
        assert isinstance(m.w_gate_up, torch.nn.Parameter) and m.w_gate_up.dtype == U8
        assert isinstance(m.w_down, torch.nn.Parameter) and m.w_down.dtype == U8
        assert m.w_gate_up.shape == (8, 256, 64) and m.w_down.shape == (8, 128, 64)
        assert m.w_gate_up_block_scale.shape == (8, 256, 4) and m.w_gate_up_block_scale.dtype == U8
        assert m.w_down_block_scale.shape == (8, 128, 4) and m.w_down_block_scale.dtype == U8
        assert m.w_gate_up_scale is None and m.w_down_scale is None
        # quantised in the stored (interleaved) row order
        p, s = ops.quantize_expert_weights_mxfp4(b.w_gate_up.data)
        assert torch.equal(m.w_gate_up.data, p) and torch.equal(m.w_gate_up_block_scale, s)
        assert isinstance(m.gate.weight, torch.nn.Parameter) and m.gate.weight.dtype == BF
    for other in stages[1:]:
        for a, b in zip(_expert_state(stages[0]), _expert_state(other)):
            for x, y in zip(a, b):
                assert x.dtype == y.dtype and torch.equal(x, y)
    for st in stages:                                   # router, attention, norms, embedding, head
        after = _bf16_state(st)
        assert sorted(after) == sorted(before)
        for k, v in before.items():
            assert after[k].dtype == v.dtype and torch.equal(after[k], v), k
    # a second quantisation changes nothing; fp8 on top of MXFP4, and MXFP4 on top of fp8, raise
    kept = stages[0].block.layers[0].mlp.w_gate_up
    stages[0].quantize_experts_mxfp4()
    assert stages[0].block.layers[0].mlp.w_gate_up is kept
    with pytest.raises(ValueError, match="MXFP4 already"):
        stages[0].quantize_experts_fp8()
    with pytest.raises(ValueError, match="MXFP4 already"):
        stages[0].quantize("fp8_experts")
    assert stages[0].block.layers[0].mlp.w_gate_up is kept
    f8 = CausalLMStage(spec, 0, 2).init_random(7).quantize_experts_fp8()
    with pytest.raises(ValueError, match="fp8 already"):
        f8.quantize_experts_mxfp4()
    with pytest.raises(ValueError, match="fp8 already"):
        f8.quantize("mxfp4_experts")
    assert f8.block.layers[0].mlp.is_fp8 and not f8.block.layers[0].mlp.is_mxfp4

    # hf_dict: the dequantised weights (exact in bf16), loadable into a bf16 stage ...
    deq = CausalLMStage(spec, 0, 2).init_random(7)
    for q, d in zip(stages[0].block.layers, deq.block.layers):
        sd = q.hf_state_dict()
        assert all(v.dtype == BF for v in sd.values())
        with torch.no_grad():
            d.load_hf_state_dict({k: v.clone() for k, v in sd.items()})
        assert torch.equal(d.mlp.w_gate_up, _dequant(q.mlp.w_gate_up, q.mlp.w_gate_up_block_scale))
        assert torch.equal(d.mlp.w_down, _dequant(q.mlp.w_down, q.mlp.w_down_block_scale))
        assert not torch.equal(d.mlp.w_down, base.block.layers[0].mlp.w_down)
        # ... and a quantised module does not load: quantise after loading
        with pytest.raises(RuntimeError, match="quantize_experts_mxfp4"):
            q.load_hf_state_dict(sd)
    # the stage on MXFP4 experts is the same stage on those dequantised bf16 weights
    got = _run_stage(stages[0], PROMPTS, decode_steps=1)
    want = _run_stage(deq, PROMPTS, decode_steps=1)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert want[0].abs().max() > 0.1


# ------------------------------------------------------------------ refusals, CLI, plan
def test_mxfp4_experts_refusals():
    for name in ("tiny-llama", "tiny-gpt2"):
        spec = PRESETS[name]
        stage = CausalLMStage(spec, 0, 1).init_random(0)
        with pytest.raises(ValueError, match="mxfp4_experts.*no experts"):
            stage.quantize("mxfp4_experts")
        with pytest.raises(ValueError, match="mxfp4_experts.*no experts"):
            stage.quantize_experts_mxfp4()
        with pytest.raises(ValueError, match="mxfp4_experts.*no experts"):
            refuse_moe_quantization(spec, "mxfp4_experts")
        with pytest.raises(ValueError, match="fp8_experts.*no experts"):
            refuse_moe_quantization(spec, "fp8_experts")
    for mt in ("qwen3_moe", "mixtral"):
        spec = _tiny(mt)
        refuse_moe_quantization(spec, "mxfp4_experts")
        refuse_moe_quantization(spec, "fp8_experts")
        for mode in ("fp8", True, "int8", "mxfp4"):
            with pytest.raises(ValueError, match="sparse MoE.*fp8_experts.*mxfp4_experts"):
                refuse_moe_quantization(spec, mode)
            with pytest.raises(ValueError, match="sparse MoE"):
                CausalLMStage(spec, 0, 1).init_random(0).quantize(mode)
    for name in ("qwen3-30b-a3b", "mixtral-8x7b"):
        refuse_moe_quantization(PRESETS[name], "mxfp4_experts")
    with pytest.raises(ValueError, match="mxfp4_experts"):       # the list of known modes
        CausalLMStage(_tiny(), 0, 1).init_random(0).quantize("fp3")


def test_cli_fp4_experts_flag():
    ap = argparse.ArgumentParser()
    cli._common(ap)
    a = ap.parse_args(["--model", "qwen3-30b-a3b", "--fp4-experts"])
    assert a.fp4_experts and not (a.fp8 or a.int8 or a.fp4 or a.fp8_experts)
    assert cli.engine_config(a).quantize == "mxfp4_experts"
    assert cli.engine_config(ap.parse_args(["--model", "qwen3-30b-a3b"])).quantize is False
    assert cli.engine_config(
        ap.parse_args(["--model", "qwen3-30b-a3b", "--fp8-experts"])).quantize == "fp8_experts"
    for other in ("--fp8", "--int8", "--fp4", "--fp8-experts"):
        with pytest.raises(SystemExit):
            ap.parse_args(["--fp4-experts", other])
    with pytest.raises(ValueError, match="sparse MoE"):
        cli.engine_config(ap.parse_args(["--model", "qwen3-30b-a3b", "--fp4"]))
    with pytest.raises(ValueError, match="mxfp4_experts.*no experts"):
        cli.engine_config(ap.parse_args(["--model", "llama-3-8b", "--fp4-experts"]))


def _plan(model, argv):
    buf = io.StringIO()
    with redirect_stdout(buf):
        assert cli.main(["plan", "--model", model, "--gpus", "1"] + argv) == 0
    return json.loads(buf.getvalue())


def test_plan_fp4_experts():
    spec = PRESETS["qwen3-30b-a3b"]
    H, I, E, L = spec.hidden_size, spec.moe_intermediate_size, spec.num_experts, spec.num_layers
    assert H % 32 == 0 and I % 32 == 0
    layer = spec.layer_param_count()
    experts = E * 3 * H * I
    # K / 2 + K / 32 bytes per stored weight row: 2 I rows of K = H and H rows of K = I per expert
    per_layer = E * (2 * I * (H // 2 + H // 32) + H * (I // 2 + I // 32)) + 2 * (layer - experts)
    assert per_layer == experts * 17 // 32 + 2 * (layer - experts)
    emb = spec.vocab_size * H * 2
    got = _plan("qwen3-30b-a3b", ["--fp4-experts"])
    assert got["weight_bytes_per_param"] == per_layer / layer
    st = got["stages"][0]
    assert st["weights_gb"] == round((L * per_layer + 2 * emb) / 1e9, 2)
    fp8 = _plan("qwen3-30b-a3b", ["--fp8-experts"])
    bf16 = _plan("qwen3-30b-a3b", [])
    assert st["weights_gb"] < fp8["stages"][0]["weights_gb"] < bf16["stages"][0]["weights_gb"]
    assert (st["kv_capacity_tokens"] > fp8["stages"][0]["kv_capacity_tokens"]
            > bf16["stages"][0]["kv_capacity_tokens"])
    # the other modes' numbers are what they were
    assert bf16["weight_bytes_per_param"] == 2
    assert bf16["stages"][0]["weights_gb"] == round((L * layer * 2 + 2 * emb) / 1e9, 2)
    fp8_layer = experts + 4 * E * (2 * I + H) + 2 * (layer - experts)
    assert fp8["weight_bytes_per_param"] == fp8_layer / layer
    assert fp8["stages"][0]["weights_gb"] == round((L * fp8_layer + 2 * emb) / 1e9, 2)
    d4 = _plan("llama-3-70b", ["--fp4"])
    dense = PRESETS["llama-3-70b"]
    assert d4["weight_bytes_per_param"] == 17 / 32
    assert d4["stages"][0]["weights_gb"] == round(
        (dense.num_layers * int(dense.layer_param_count() * 17 / 32)
         + 2 * dense.vocab_size * dense.hidden_size * 2) / 1e9, 2)
    with pytest.raises(ValueError, match="no experts"):
        _plan("llama-3-70b", ["--fp4-experts"])
