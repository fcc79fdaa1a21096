"""Qwen2-MoE on the CPU reference path: the shared expert (a dense SwiGLU expert beside the routed
ones, scaled by the sigmoid of a gate that is stored as one more router row) and stacks that mix
dense and sparse layers -- parity with the installed HF implementation, config parsing and its
refusals, per-layer parameter counts, the reference ops, checkpoint layouts, expert-only
quantisation and the planner's bytes.  The kernels are pinned by tests/test_moe_shared_gpu.py."""
import io
import json
from contextlib import redirect_stdout

import pytest
import torch

from distributed_llm_inference import cli, ops
from distributed_llm_inference.config import PRESETS, ModelSpec, plan_stages
from distributed_llm_inference.models import CausalLMStage
from distributed_llm_inference.models.llama.modules import LlamaMLP, MoEMLP
from distributed_llm_inference.ops import reference as ref

BF = torch.bfloat16
PROMPTS = [[5, 17, 99, 3, 250, 7, 7, 1], [8, 2, 64]]


def _run_stage(stage, prompts, decode_steps=0):
    """test_moe_cpu.py's: prefill all prompts as one varlen batch, then greedy-decode."""
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


def _check_against_hf(hf, stage_logits, prompts, steps):
    """test_moe_cpu.py's criterion: error < 0.05 max(1, max |logit|)."""
    gen = torch.stack([o.argmax(-1) for o in stage_logits], 1)
    for b, p in enumerate(prompts):
        seq = torch.tensor(p + gen[b, :steps].tolist())[None]
        with torch.no_grad():
            ref_logits = hf(seq).logits[0].float()
        for s in range(steps + 1):
            a, r = stage_logits[s][b], ref_logits[len(p) - 1 + s]
            err = (a - r).abs().max().item()
            assert err < 0.05 * max(1.0, r.abs().max().item()), f"b={b} step={s} err={err}"


def _round_weights(m, router_std=0.5):
    """test_moe_cpu.py's: bf16-representable weights and a router far from uniform (the name
    filter also gives shared_expert_gate that spread, so its sigmoid is away from 1/2)."""
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("gate.weight"):
                p.copy_(router_std * torch.randn(p.shape, generator=g))
            p.copy_(p.to(BF).float())
    return m.eval()


def _hf_qwen2_moe(seed=1, layers=2, **kw):
    pytest.importorskip("transformers")
    from transformers import Qwen2MoeConfig, Qwen2MoeForCausalLM
    torch.manual_seed(seed)
    cfg = Qwen2MoeConfig(vocab_size=256, hidden_size=128, intermediate_size=256,
                         moe_intermediate_size=128, shared_expert_intermediate_size=384,
                         num_hidden_layers=layers, num_attention_heads=4, num_key_value_heads=2,
                         num_experts=8, num_experts_per_tok=2, norm_topk_prob=False,
                         rms_norm_eps=1e-6, max_position_embeddings=4096,
                         tie_word_embeddings=False,
                         rope_parameters={"rope_type": "default", "rope_theta": 1000000.0}, **kw)
    return _round_weights(Qwen2MoeForCausalLM(cfg))


def _tiny(**kw):
    base = dict(name="tiny-q2moe", model_type="qwen2_moe", vocab_size=256, hidden_size=128,
                intermediate_size=256, num_layers=4, num_heads=4, num_kv_heads=2, head_dim=32,
                rms_norm_eps=1e-6, rope_theta=1000000.0, max_position_embeddings=4096,
                bos_token_id=1, eos_token_id=2, attention_bias=True, o_proj_bias=False,
                num_experts=8, num_experts_per_tok=2, moe_intermediate_size=128,
                shared_expert_intermediate_size=384, norm_topk_prob=False,
                decoder_sparse_step=2, mlp_only_layers=(3,))
    base.update(kw)
    return ModelSpec(**base)


# ------------------------------------------------------------------ parity with HF
def test_qwen2_moe_all_sparse_matches_hf():
    from distributed_llm_inference.utils.model import stage_from_hf_model
    hf = _hf_qwen2_moe()
    stage = stage_from_hf_model(hf, 0, hf.config.num_hidden_layers)
    spec = stage.spec
    assert spec.model_type == "qwen2_moe" and not spec.qk_norm and spec.head_dim == 32
    assert spec.attention_bias and not spec.has_o_proj_bias
    assert (spec.num_experts, spec.num_experts_per_tok, spec.moe_intermediate_size,
            spec.shared_expert_intermediate_size, spec.norm_topk_prob) == (8, 2, 128, 384, False)
    assert all(isinstance(layer.mlp, MoEMLP) for layer in stage.block.layers)
    assert stage.block.layers[0].mlp.gate.weight.shape == (9, 128)
    assert spec.param_count() == sum(p.numel() for p in hf.parameters())
    assert spec.param_count() == sum(p.numel() for p in stage.parameters())
    _check_against_hf(hf, _run_stage(stage, PROMPTS, decode_steps=3), PROMPTS, 3)


def test_qwen2_moe_mixed_stack_matches_hf():
    from transformers.models.qwen2_moe.modeling_qwen2_moe import Qwen2MoeSparseMoeBlock
    from distributed_llm_inference.utils.model import stage_from_hf_model
    hf = _hf_qwen2_moe(seed=3, layers=4, decoder_sparse_step=2, mlp_only_layers=[3])
    stage = stage_from_hf_model(hf, 0, 4)
    spec = stage.spec
    assert (spec.decoder_sparse_step, spec.mlp_only_layers) == (2, (3,))
    kinds = [type(layer.mlp) for layer in stage.block.layers]
    assert kinds == [LlamaMLP, MoEMLP, LlamaMLP, LlamaMLP]          # dense, sparse, dense, dense
    assert [layer.is_moe for layer in stage.block.layers] == [False, True, False, False]
    for i, hl in enumerate(hf.model.layers):
        assert spec.is_sparse_layer(i) == isinstance(hl.mlp, Qwen2MoeSparseMoeBlock)
    assert stage.block.layers[0].mlp.intermediate_size == 256
    assert spec.param_count() == sum(p.numel() for p in hf.parameters())
    assert spec.param_count() == sum(p.numel() for p in stage.parameters())
    for i, hl in enumerate(hf.model.layers):
        assert spec.layer_param_count(i) == sum(p.numel() for p in hl.parameters())
    _check_against_hf(hf, _run_stage(stage, PROMPTS, decode_steps=3), PROMPTS, 3)


def test_shared_block_matches_hf_block_in_bf16():
    """The block alone against HF's ``Qwen2MoeSparseMoeBlock`` run in bf16 on 37 rows.  As in
    test_moe_block_matches_hf_block_in_bf16, HF rounds every weighted expert row and accumulates
    in bf16: at most 6 + k roundings for the routed part, plus 7 for the shared MLP, the sigmoid,
    the product and the sum -- 15 2^-9 < 2^-5 at k = 2, relative to the largest term, which is
    taken as max(|routed| + |shared gate|) in fp32 from HF's own sub-modules."""
    hf = _hf_qwen2_moe(seed=7)
    blk = hf.model.layers[0].mlp.to(BF)
    spec = ModelSpec.from_hf_config(hf.config)
    mlp = MoEMLP(spec)
    sd = {k[len("model.layers.0."):]: v.detach() for k, v in hf.state_dict().items()
          if k.startswith("model.layers.0.")}
    with torch.no_grad():
        mlp.load_hf(sd.__getitem__, sd, BF)
    x = torch.randn(37, 128, generator=torch.Generator().manual_seed(0)).to(BF)
    with torch.no_grad():
        want = blk(x[None])[0].float()
        _, rw, sel = blk.gate(x)
        routed = blk.experts(x, sel, rw).float()
        shared = (torch.sigmoid(blk.shared_expert_gate(x)) * blk.shared_expert(x)).float()
    got = mlp(x)
    assert got.dtype == BF and got.shape == (37, 128)
    scale = (routed.abs() + shared.abs()).max().item()
    err = (got.float() - want).abs().max().item()
    print(f"block err {err:.4g}, scale {scale:.4g}, ratio {err / scale:.4g} (bound {2.0 ** -5:.4g})")
    assert err <= 2.0 ** -5 * scale
    assert want.abs().max().item() > 0.01
    assert shared.abs().max().item() > 0.01        # the shared term is a real part of the sum


# ------------------------------------------------------------------ the reference ops
def test_reference_topk_with_the_gate_column():
    g = torch.Generator().manual_seed(5)
    T, E, k, ld = 23, 60, 4, 64
    logits = torch.randn(T, ld, generator=g).to(BF)
    logits[:, E] = torch.linspace(-8, 8, T).to(BF)
    logits[0, E], logits[1, E] = 0.0, -0.0
    logits[:, E + 1:] = 30.0                              # padding: never read
    for renorm in (False, True):
        ids, w, sw = ref.moe_topk(logits, k, renorm, num_experts=E)
        ids0, w0 = ref.moe_topk(logits[:, :E].contiguous(), k, renorm)
        assert torch.equal(ids, ids0) and torch.equal(w, w0)
        assert sw.dtype == torch.float32 and sw.shape == (T,)
        assert torch.equal(sw, torch.sigmoid(logits[:, E]).float())
        assert sw[0] == 0.5 and sw[1] == 0.5
    r = ops.moe_route(logits, k, False, num_experts=E)
    r0 = ops.moe_route(logits[:, :E].contiguous(), k, False)
    assert r0.shared_w is None and torch.equal(r.shared_w, sw)
    for name in ("topk_ids", "topk_w", "expert_count", "expert_offset", "sorted_pairs",
                 "tile_expert", "tile_start", "tile_rows", "n_tiles"):
        assert torch.equal(getattr(r, name), getattr(r0, name)), name
    assert r.expert_count.numel() == E
    with pytest.raises(ValueError, match="num_experts"):
        ops.moe_topk(logits[:, :E].contiguous(), k, False, num_experts=E)
    with pytest.raises(ValueError, match="num_experts"):
        ref.moe_topk(logits[:, :E].contiguous(), k, False, num_experts=E)


def test_reference_combine_with_the_shared_term():
    g = torch.Generator().manual_seed(6)
    T, k, H = 19, 4, 128
    y = torch.randn(T * k, H, generator=g).to(BF)
    w = torch.rand(T, k, generator=g).to(BF).float()
    s = torch.randn(T, H, generator=g).to(BF)
    sw = torch.rand(T, generator=g).to(BF).float()
    plain = ref.moe_combine(y, w)
    zero = ref.moe_combine(y, w, s, torch.zeros(T))
    assert torch.equal(plain.view(torch.int16), zero.view(torch.int16))
    only = ref.moe_combine(y, torch.zeros(T, k), s, sw)
    assert torch.equal(only, (sw[:, None] * s.float()).to(BF))
    # fp32: the slots in order, then the shared term, then one rounding
    acc = torch.zeros(T, H)
    for j in range(k):
        acc += w[:, j, None] * y.view(T, k, H)[:, j].float()
    acc += sw[:, None] * s.float()
    got = ops.moe_combine(y, w, shared=s, shared_w=sw)
    assert got.dtype == BF and torch.equal(got, acc.to(BF))
    assert not torch.equal(got, plain)
    with pytest.raises(ValueError, match="go together"):
        ops.moe_combine(y, w, shared=s)
    with pytest.raises(ValueError, match="go together"):
        ops.moe_mlp(s, s, y, y, k, False, num_experts=8)


# ------------------------------------------------------------------ config
def test_config_round_trip_and_presets():
    q = _tiny()
    d = q.to_hf_dict()
    assert d["model_type"] == "qwen2_moe" and d["architectures"] == ["Qwen2MoeForCausalLM"]
    assert (d["num_experts"], d["num_experts_per_tok"], d["moe_intermediate_size"],
            d["shared_expert_intermediate_size"], d["norm_topk_prob"], d["decoder_sparse_step"],
            d["mlp_only_layers"]) == (8, 2, 128, 384, False, 2, [3])
    back = ModelSpec.from_hf_config(d)
    assert back.replace(name=q.name) == q
    assert back.attention_bias and not back.has_o_proj_bias and not back.qk_norm
    assert [q.is_sparse_layer(i) for i in range(4)] == [False, True, False, False]
    assert json.loads(json.dumps(d)) == d                   # config.json-serialisable
    # sliding-window fields as for qwen2: off unless use_sliding_window
    assert ModelSpec.from_hf_config(dict(d, sliding_window=64)).sliding_window is None
    win = q.replace(sliding_window=64)
    assert ModelSpec.from_hf_config(win.to_hf_dict()).replace(name=q.name) == win
    renorm = q.replace(norm_topk_prob=True, decoder_sparse_step=1, mlp_only_layers=())
    assert ModelSpec.from_hf_config(renorm.to_hf_dict()).replace(name=q.name) == renorm
    # models without experts: no layer is sparse
    assert not any(PRESETS["llama-3-8b"].is_sparse_layer(i) for i in range(32))
    assert all(PRESETS["qwen3-30b-a3b"].is_sparse_layer(i) for i in range(48))

    for name in ("qwen1.5-moe-a2.7b", "qwen2-57b-a14b"):
        p = PRESETS[name]
        assert ModelSpec.from_hf_config(p.to_hf_dict()).replace(name=p.name) == p
        assert all(p.is_sparse_layer(i) for i in range(p.num_layers))
    p = PRESETS["qwen1.5-moe-a2.7b"]
    assert (p.num_layers, p.hidden_size, p.num_heads, p.num_kv_heads, p.head_dim, p.num_experts,
            p.num_experts_per_tok, p.moe_intermediate_size, p.shared_expert_intermediate_size,
            p.intermediate_size, p.vocab_size, p.norm_topk_prob) == (
                24, 2048, 16, 16, 128, 60, 4, 1408, 5632, 5632, 151936, False)
    b = PRESETS["qwen2-57b-a14b"]
    assert (b.num_layers, b.hidden_size, b.num_heads, b.num_kv_heads, b.num_experts,
            b.num_experts_per_tok, b.moe_intermediate_size, b.shared_expert_intermediate_size,
            b.intermediate_size, b.vocab_size) == (28, 3584, 28, 4, 64, 8, 2560, 20480, 18944,
                                                   151936)
    # by hand: attention (q/k/v with bias, o without) + two norms, then the MLP of each kind
    H = 2048
    attn = H * 3 * 2048 + 3 * 2048 + 2048 * H + 2 * H
    sparse = attn + 60 * H + 60 * 3 * H * 1408 + 3 * H * 5632 + H
    assert p.layer_param_count(0) == p.layer_param_count() == sparse
    assert p.expert_param_count(0) == p.expert_param_count() == 60 * 3 * H * 1408
    mixed = p.replace(decoder_sparse_step=2)
    assert not mixed.is_sparse_layer(0) and mixed.is_sparse_layer(1)
    assert mixed.layer_param_count(0) == attn + 3 * H * 5632
    assert mixed.layer_param_count(1) == mixed.layer_param_count() == sparse
    assert mixed.expert_param_count(0) == 0 and mixed.expert_param_count(1) == 60 * 3 * H * 1408
    assert mixed.param_count() == 12 * sparse + 12 * (attn + 3 * H * 5632) + 2 * 151936 * H + H
    assert 14e9 < p.param_count() < 14.6e9
    plan = plan_stages(mixed, 4)
    assert plan[0][0] == 0 and plan[-1][1] == 24


def test_config_refusals():
    d = _tiny().to_hf_dict()
    for bad in (0, 192, -128):
        with pytest.raises(ValueError, match="shared_expert_intermediate_size"):
            ModelSpec.from_hf_config(dict(d, shared_expert_intermediate_size=bad))
    with pytest.raises(ValueError, match="no sparse layer"):
        ModelSpec.from_hf_config(dict(d, mlp_only_layers=[1, 3]))
    with pytest.raises(ValueError, match="no sparse layer"):
        ModelSpec.from_hf_config(dict(d, decoder_sparse_step=5, mlp_only_layers=[]))
    for bad in ([4], [-1], [1, 7]):
        with pytest.raises(ValueError, match="mlp_only_layers"):
            ModelSpec.from_hf_config(dict(d, mlp_only_layers=bad))
    with pytest.raises(ValueError, match="lacks"):
        ModelSpec.from_hf_config({k: v for k, v in d.items()
                                  if k != "shared_expert_intermediate_size"})
    with pytest.raises(ValueError, match="shared_expert_intermediate_size"):
        PRESETS["tiny-llama"].replace(shared_expert_intermediate_size=128)
    # qwen3_moe keeps refusing the two pattern fields
    q3 = ModelSpec(name="t", model_type="qwen3_moe", vocab_size=256, hidden_size=128,
                   intermediate_size=256, num_layers=2, num_heads=4, num_kv_heads=2, head_dim=64,
                   num_experts=8, num_experts_per_tok=2, moe_intermediate_size=128,
                   qk_norm=True).to_hf_dict()
    with pytest.raises(ValueError, match="decoder_sparse_step"):
        ModelSpec.from_hf_config(dict(q3, decoder_sparse_step=2))
    with pytest.raises(ValueError, match="mlp_only_layers"):
        ModelSpec.from_hf_config(dict(q3, mlp_only_layers=[0]))


# ------------------------------------------------------------------ state dicts
def test_state_dict_layouts_and_round_trip():
    spec = _tiny()
    a = CausalLMStage(spec, 0, 4).init_random(5)
    la = a.block.layers[1]
    sd = la.hf_state_dict()
    E, I, H, S = 8, 128, 128, 384
    assert sd["mlp.gate.weight"].shape == (E, H)
    assert sd["mlp.shared_expert_gate.weight"].shape == (1, H)
    assert sd["mlp.shared_expert.gate_proj.weight"].shape == (S, H)
    assert sd["mlp.shared_expert.up_proj.weight"].shape == (S, H)
    assert sd["mlp.shared_expert.down_proj.weight"].shape == (H, S)
    assert sd["mlp.experts.7.down_proj.weight"].shape == (H, I)
    assert sd["self_attn.q_proj.bias"].shape == (128,) and "self_attn.o_proj.bias" not in sd
    assert len([k for k in sd if "experts." in k]) == 3 * E
    assert torch.equal(la.mlp.gate.weight[:E], sd["mlp.gate.weight"])
    assert torch.equal(la.mlp.gate.weight[E:], sd["mlp.shared_expert_gate.weight"])
    dense = a.block.layers[0].hf_state_dict()
    assert dense["mlp.gate_proj.weight"].shape == (256, H) and "mlp.gate.weight" not in dense

    b = CausalLMStage(spec, 0, 4).init_random(6)
    for x, y in zip(a.block.layers, b.block.layers):
        y.load_hf_state_dict({k: v.clone() for k, v in x.hf_state_dict().items()})
    c = CausalLMStage(spec, 0, 4).init_random(7)           # the fused 3-D expert tensors
    for x, y in zip(a.block.layers, c.block.layers):
        per = x.hf_state_dict()
        fused = {k: v.clone() for k, v in per.items() if "experts." not in k}
        if x.is_moe:
            fused["mlp.experts.gate_up_proj"] = torch.stack(
                [torch.cat([per[f"mlp.experts.{e}.gate_proj.weight"],
                            per[f"mlp.experts.{e}.up_proj.weight"]], 0) for e in range(E)])
            fused["mlp.experts.down_proj"] = torch.stack(
                [per[f"mlp.experts.{e}.down_proj.weight"] for e in range(E)])
        y.load_hf_state_dict(fused)
    for other in (b, c):
        other.embed.load_state_dict(a.embed.state_dict())
        other.head.load_state_dict(a.head.state_dict())
        for x, y in zip(a.block.layers, other.block.layers):
            for (n, p), (_, q) in zip(x.named_parameters(), y.named_parameters()):
                assert torch.equal(p, q), n
    ya, yb = _run_stage(a, PROMPTS, decode_steps=1), _run_stage(b, PROMPTS, decode_steps=1)
    assert all(torch.equal(x, y) for x, y in zip(ya, yb))
    for key in ("mlp.shared_expert_gate.weight", "mlp.shared_expert.up_proj.weight"):
        with pytest.raises(KeyError, match=key.replace(".", r"\.")):
            b.block.layers[1].load_hf_state_dict({k: v for k, v in sd.items() if k != key})
    with pytest.raises(ValueError, match="gate.weight"):
        b.block.layers[1].load_hf_state_dict(dict(sd, **{"mlp.gate.weight": la.mlp.gate.weight}))


def test_checkpoint_dir_round_trip(tmp_path):
    pytest.importorskip("safetensors")
    from distributed_llm_inference.utils.model import build_stage, save_random_checkpoint
    spec = _tiny()
    path = str(tmp_path / "ckpt")
    save_random_checkpoint(spec, path, seed=5, shard_layers=1)
    stage = build_stage(path, 0, 4, random_init=False, checkpoint=path)
    want = CausalLMStage(spec, 0, 4).init_random(5)
    assert stage.spec.replace(name=spec.name) == spec
    for x, y in zip(want.block.layers, stage.block.layers):
        assert type(x.mlp) is type(y.mlp)
        for (n, p), (_, q) in zip(x.named_parameters(), y.named_parameters()):
            assert torch.equal(p, q), n
    part = build_stage(path, 1, 3, random_init=False, checkpoint=path)   # sparse + dense
    assert [l.is_moe for l in part.block.layers] == [True, False]
    assert torch.equal(part.block.layers[0].mlp.gate.weight, want.block.layers[1].mlp.gate.weight)


def test_init_random_seeds_every_new_tensor():
    spec = _tiny()
    a = CausalLMStage(spec, 0, 4).init_random(3)
    b = CausalLMStage(spec, 1, 2).init_random(3)     # any split holds the same weights
    m, n = a.block.layers[1].mlp, b.block.layers[0].mlp
    assert m.gate.weight.shape == (9, 128)
    for name in ("gate.weight", "shared_expert.gate_up_proj.weight",
                 "shared_expert.down_proj.weight", "w_gate_up", "w_down"):
        p, q = m.get_parameter(name), n.get_parameter(name)
        assert torch.equal(p, q), name
        assert 0.015 < p.float().std().item() < 0.025, name
    assert m.gate.weight[8].float().abs().max() > 0          # the gate row is seeded too
    other = CausalLMStage(spec, 0, 4).init_random(4).block.layers[1].mlp
    assert not torch.equal(m.shared_expert.down_proj.weight, other.shared_expert.down_proj.weight)
    assert not torch.equal(m.gate.weight[8], other.gate.weight[8])


# ------------------------------------------------------------------ quantisation
@pytest.mark.parametrize("mode", ["fp8_experts", "mxfp4_experts"])
def test_expert_quantisation_on_the_mixed_stack(mode):
    spec = _tiny()
    stage = CausalLMStage(spec, 0, 4).init_random(2)
    before = _run_stage(stage, PROMPTS, decode_steps=1)
    gate = stage.block.layers[1].mlp.gate.weight.clone()
    stage.quantize(mode)
    for layer in stage.block.layers:
        lins = [layer.self_attn.qkv_proj, layer.self_attn.o_proj]
        if layer.is_moe:
            m = layer.mlp
            assert m.is_fp8 if mode == "fp8_experts" else m.is_mxfp4
            assert m.w_gate_up.dtype != BF and m.w_down.dtype != BF
            assert m.gate.weight.dtype == BF and torch.equal(m.gate.weight, gate)
            assert m.gate.weight.shape == (9, 128)
            lins += [m.shared_expert.gate_up_proj, m.shared_expert.down_proj]
        else:
            lins += [layer.mlp.gate_up_proj, layer.mlp.down_proj]
        for lin in lins:                                  # everything but the experts: bf16
            assert lin.weight.dtype == BF and lin.weight.numel() > 0
            assert not (lin.is_fp8 or lin.is_fp4 or lin.is_int8)
    after = _run_stage(stage, PROMPTS, decode_steps=1)
    assert all(torch.isfinite(x).all() for x in after)
    # the quantised experts change the logits a little, not the model
    assert 0 < (after[0] - before[0]).abs().max().item() < 0.25 * before[0].abs().max().item()
    # a range of dense layers only: nothing to quantise, not an error
    dense = CausalLMStage(spec, 2, 4).init_random(2)
    sd = {k: v.clone() for k, v in dense.state_dict().items()}
    dense.quantize(mode)
    assert all(torch.equal(v, sd[k]) for k, v in dense.state_dict().items())
    assert set(dense.state_dict()) == set(sd)


def test_whole_model_quantisation_still_raises():
    for call in ("quantize_fp8", "quantize_int8", "quantize_mxfp4"):
        stage = CausalLMStage(_tiny(), 0, 4).init_random(0)
        with pytest.raises(ValueError, match="sparse MoE"):
            getattr(stage, call)()
        with pytest.raises(ValueError, match="sparse MoE"):
            getattr(stage.block, call)()
    for mode in ("fp8", "int8", "mxfp4"):
        with pytest.raises(ValueError, match="sparse MoE"):
            CausalLMStage(_tiny(), 2, 4).init_random(0).quantize(mode)   # dense layers only, too


# ------------------------------------------------------------------ planner bytes
def _plan(model, argv, gpus=1):
    buf = io.StringIO()
    with redirect_stdout(buf):
        assert cli.main(["plan", "--model", model, "--gpus", str(gpus)] + argv) == 0
    return json.loads(buf.getvalue())


def test_plan_sums_per_layer_bytes(tmp_path):
    spec = PRESETS["qwen1.5-moe-a2.7b"]
    H, I, E, L = spec.hidden_size, spec.moe_intermediate_size, spec.num_experts, spec.num_layers
    emb = spec.vocab_size * H * 2
    experts = E * 3 * H * I
    fp4_experts = E * (2 * I * (H // 2 + H // 32) + H * (I // 2 + I // 32))
    bf16 = _plan("qwen1.5-moe-a2.7b", [])
    want = sum(2 * spec.layer_param_count(i) for i in range(L)) + 2 * emb
    assert bf16["stages"][0]["weights_gb"] == round(want / 1e9, 2)
    fp4 = _plan("qwen1.5-moe-a2.7b", ["--fp4-experts"])
    want4 = sum(fp4_experts + 2 * (spec.layer_param_count(i) - experts) for i in range(L)) + 2 * emb
    assert fp4["stages"][0]["weights_gb"] == round(want4 / 1e9, 2)
    assert want4 < want
    # a mixed stack, from a config.json: dense layers stay bf16 under --fp4-experts, and every
    # stage sums the layers it actually holds
    mixed = spec.replace(decoder_sparse_step=2, mlp_only_layers=(3,))
    path = tmp_path / "config.json"
    path.write_text(json.dumps(mixed.to_hf_dict()))
    env = pytest.MonkeyPatch()
    env.setenv("DLI_HEAD_ROTATION", "0")
    try:
        for argv, layer_bytes in (
                ([], lambda i: 2 * mixed.layer_param_count(i)),
                (["--fp4-experts"], lambda i: (
                    fp4_experts + 2 * (mixed.layer_param_count(i) - experts)
                    if mixed.is_sparse_layer(i) else 2 * mixed.layer_param_count(i)))):
            got = _plan(str(path), argv, gpus=2)
            assert len(got["stages"]) == 2
            for n, st in enumerate(got["stages"]):
                s, e = st["layers"]
                w = sum(layer_bytes(i) for i in range(s, e)) + emb
                assert st["weights_gb"] == round(w / 1e9, 2), (argv, n)
    finally:
        env.undo()
    assert sum(mixed.is_sparse_layer(i) for i in range(L)) == 11
