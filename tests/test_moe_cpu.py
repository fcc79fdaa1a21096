"""Sparse mixture-of-experts models (Qwen3-MoE, Mixtral) on the CPU reference path: config parsing
and its refusals, parity with the installed HF implementations, both checkpoint layouts, the
parameter count, the reference routing op (ids, weights, tie rule, grouping invariants) and the
quantisation refusals.  The kernels are pinned by tests/test_moe_gpu.py."""
import pytest
import torch

from distributed_llm_inference import ops
from distributed_llm_inference.config import PRESETS, ModelSpec, plan_stages
from distributed_llm_inference.models import CausalLMStage
from distributed_llm_inference.models.llama.modules import LlamaMLP, MoEMLP
from distributed_llm_inference.ops import reference as ref

BF = torch.bfloat16


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


def _check_against_hf(hf, stage_logits, prompts, steps):
    """The criterion of test_qwen3_cpu.py::test_qwen3_matches_hf."""
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
    """bf16-representable weights; a router far from uniform, so the top-k is decided by more
    than rounding noise, and q/k norm weights away from their initial 1."""
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("gate.weight"):
                p.copy_(router_std * torch.randn(p.shape, generator=g))
            if n.endswith(("q_norm.weight", "k_norm.weight")):
                p.copy_(1 + 0.3 * torch.randn(p.shape, generator=g))
            p.copy_(p.to(BF).float())
    return m.eval()


def _hf_qwen3_moe(seed=1, norm_topk_prob=True):
    pytest.importorskip("transformers")
    from transformers import Qwen3MoeConfig, Qwen3MoeForCausalLM
    torch.manual_seed(seed)
    cfg = Qwen3MoeConfig(vocab_size=256, hidden_size=128, intermediate_size=256,
                         moe_intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                         num_key_value_heads=2, head_dim=64, num_experts=8, num_experts_per_tok=2,
                         norm_topk_prob=norm_topk_prob, rms_norm_eps=1e-6,
                         max_position_embeddings=4096, tie_word_embeddings=False,
                         rope_parameters={"rope_type": "default", "rope_theta": 1000000.0})
    return _round_weights(Qwen3MoeForCausalLM(cfg))


def _hf_mixtral(seed=2):
    pytest.importorskip("transformers")
    from transformers import MixtralConfig, MixtralForCausalLM
    torch.manual_seed(seed)
    cfg = MixtralConfig(vocab_size=256, hidden_size=128, intermediate_size=128,
                        num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                        num_local_experts=8, num_experts_per_tok=2, rms_norm_eps=1e-5,
                        max_position_embeddings=4096, sliding_window=None,
                        tie_word_embeddings=False,
                        rope_parameters={"rope_type": "default", "rope_theta": 1000000.0})
    return _round_weights(MixtralForCausalLM(cfg))


PROMPTS = [[5, 17, 99, 3, 250, 7, 7, 1], [8, 2, 64]]


def test_qwen3_moe_matches_hf():
    from distributed_llm_inference.utils.model import stage_from_hf_model
    hf = _hf_qwen3_moe()
    stage = stage_from_hf_model(hf, 0, hf.config.num_hidden_layers)
    spec = stage.spec
    assert spec.model_type == "qwen3_moe" and spec.qk_norm and spec.head_dim == 64
    assert (spec.num_experts, spec.num_experts_per_tok, spec.moe_intermediate_size,
            spec.norm_topk_prob) == (8, 2, 128, True)
    assert all(isinstance(layer.mlp, MoEMLP) for layer in stage.block.layers)
    assert spec.param_count() == sum(p.numel() for p in hf.parameters())
    assert spec.param_count() == sum(p.numel() for p in stage.parameters())
    _check_against_hf(hf, _run_stage(stage, PROMPTS, decode_steps=3), PROMPTS, 3)


def test_qwen3_moe_without_renormalisation_matches_hf():
    from distributed_llm_inference.utils.model import stage_from_hf_model
    hf = _hf_qwen3_moe(seed=4, norm_topk_prob=False)
    stage = stage_from_hf_model(hf, 0, 2)
    assert not stage.spec.norm_topk_prob
    _check_against_hf(hf, _run_stage(stage, PROMPTS, decode_steps=1), PROMPTS, 1)


def test_mixtral_matches_hf():
    from distributed_llm_inference.utils.model import stage_from_hf_model
    hf = _hf_mixtral()
    stage = stage_from_hf_model(hf, 0, hf.config.num_hidden_layers)
    spec = stage.spec
    assert spec.model_type == "mixtral" and not spec.qk_norm and spec.head_dim == 32
    assert (spec.num_experts, spec.num_experts_per_tok, spec.moe_intermediate_size,
            spec.norm_topk_prob) == (8, 2, 128, True)
    assert spec.param_count() == sum(p.numel() for p in hf.parameters())
    _check_against_hf(hf, _run_stage(stage, PROMPTS, decode_steps=3), PROMPTS, 3)


def test_moe_block_matches_hf_block_in_bf16():
    """The MoE block alone against HF's ``Qwen3MoeSparseMoeBlock`` run in bf16 on the same rows:
    the router logits are the same bf16 product, so the routing is equal, and what differs is
    rounding -- ours rounds gate, up, silu * up, each expert's down output and the combined sum
    once each, HF in addition rounds every weighted expert row and accumulates the k rows in
    bf16.  At most 6 + k roundings of 2^-9 relative to the largest term: 2^-5 of max |out| is
    a bound with room for cancellation between the k terms."""
    hf = _hf_qwen3_moe(seed=7)
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
    got = mlp(x).float()
    assert got.dtype == torch.float32 and mlp(x).dtype == BF
    assert (got - want).abs().max().item() <= 2.0 ** -5 * want.abs().max().item()
    assert want.abs().max().item() > 0.01


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


def test_config_parse_and_round_trip():
    q = _tiny()
    d = q.to_hf_dict()
    assert d["model_type"] == "qwen3_moe" and d["architectures"] == ["Qwen3MoeForCausalLM"]
    assert (d["num_experts"], d["num_experts_per_tok"], d["moe_intermediate_size"],
            d["norm_topk_prob"], d["head_dim"]) == (8, 2, 128, True, 64)
    assert ModelSpec.from_hf_config(d).replace(name=q.name) == q
    unnorm = q.replace(norm_topk_prob=False)
    assert ModelSpec.from_hf_config(unnorm.to_hf_dict()).replace(name=q.name) == unnorm
    # the hub's key for the expert count, and the name transformers 5.x serialises it under
    alt = dict(d)
    alt["num_local_experts"] = alt.pop("num_experts")
    assert ModelSpec.from_hf_config(alt).num_experts == 8

    m = _tiny("mixtral")
    d = m.to_hf_dict()
    assert d["model_type"] == "mixtral" and d["architectures"] == ["MixtralForCausalLM"]
    assert (d["num_local_experts"], d["num_experts_per_tok"], d["intermediate_size"]) == (8, 2, 128)
    back = ModelSpec.from_hf_config(d)
    assert back.replace(name=m.name) == m
    assert back.moe_intermediate_size == 128 and back.norm_topk_prob and not back.qk_norm
    # sliding_window as for mistral
    win = m.replace(sliding_window=64)
    assert ModelSpec.from_hf_config(win.to_hf_dict()).sliding_window == 64

    for name in ("qwen3-30b-a3b", "mixtral-8x7b"):
        p = PRESETS[name]
        assert ModelSpec.from_hf_config(p.to_hf_dict()).replace(name=p.name) == p
    p = PRESETS["qwen3-30b-a3b"]
    assert (p.num_layers, p.hidden_size, p.num_heads, p.num_kv_heads, p.head_dim, p.num_experts,
            p.num_experts_per_tok, p.moe_intermediate_size) == (48, 2048, 32, 4, 128, 128, 8, 768)
    # router + E x 3 H I per layer: what the planner and the KV-pool sizing see
    attn = 2048 * (32 + 8) * 128 + 32 * 128 * 2048 + 2 * 2048 + 2 * 128
    assert p.layer_param_count() == attn + 2048 * 128 + 128 * 3 * 2048 * 768
    assert 30e9 < p.param_count() < 31e9
    assert 46e9 < PRESETS["mixtral-8x7b"].param_count() < 47e9
    plan = plan_stages(p, 4)
    assert plan[0][0] == 0 and plan[-1][1] == 48


def test_config_refusals():
    d = _tiny().to_hf_dict()
    with pytest.raises(ValueError, match="decoder_sparse_step"):
        ModelSpec.from_hf_config(dict(d, decoder_sparse_step=2))
    with pytest.raises(ValueError, match="mlp_only_layers"):
        ModelSpec.from_hf_config(dict(d, mlp_only_layers=[0]))
    with pytest.raises(ValueError, match="num_experts"):
        ModelSpec.from_hf_config(dict(d, num_experts=257))
    with pytest.raises(ValueError, match="num_experts_per_tok"):
        ModelSpec.from_hf_config(dict(d, num_experts=16, num_experts_per_tok=9))
    with pytest.raises(ValueError, match="multiples of 128"):
        ModelSpec.from_hf_config(dict(d, moe_intermediate_size=192))
    with pytest.raises(ValueError, match="multiples of 128"):
        ModelSpec.from_hf_config(dict(d, hidden_size=192))
    md = _tiny("mixtral").to_hf_dict()
    with pytest.raises(ValueError, match="multiples of 128"):
        ModelSpec.from_hf_config(dict(md, intermediate_size=320))
    with pytest.raises(ValueError, match="num_experts"):
        ModelSpec.from_hf_config(dict(md, num_local_experts=512))
    with pytest.raises(ValueError, match="lacks"):
        ModelSpec.from_hf_config({"model_type": "mixtral"})
    assert ModelSpec.from_hf_config(dict(d, num_experts=256, num_experts_per_tok=8)).num_experts == 256


@pytest.mark.parametrize("model_type", ["qwen3_moe", "mixtral"])
def test_state_dict_layouts_and_round_trip(model_type):
    spec = _tiny(model_type)
    a = CausalLMStage(spec, 0, 2).init_random(5)
    la = a.block.layers[0]
    sd = la.hf_state_dict()
    E, I, H = 8, 128, 128
    if model_type == "mixtral":
        assert sd["block_sparse_moe.gate.weight"].shape == (E, H)
        assert sd["block_sparse_moe.experts.7.w1.weight"].shape == (I, H)
        assert sd["block_sparse_moe.experts.7.w2.weight"].shape == (H, I)
        assert not any(k.startswith("mlp.") for k in sd)
        pre, names = "block_sparse_moe.", ("w1", "w3", "w2")
    else:
        assert sd["mlp.gate.weight"].shape == (E, H)
        assert sd["mlp.experts.0.up_proj.weight"].shape == (I, H)
        pre, names = "mlp.", ("gate_proj", "up_proj", "down_proj")
    assert len([k for k in sd if "experts." in k]) == 3 * E
    # stored rows are the swiglu-interleaved [gate; up] of each expert
    gu3 = torch.cat([sd[f"{pre}experts.3.{names[0]}.weight"],
                     sd[f"{pre}experts.3.{names[1]}.weight"]], 0)
    assert torch.equal(la.mlp.w_gate_up[3], ops.swiglu_interleave(gu3))
    assert torch.equal(la.mlp.w_down[3], sd[f"{pre}experts.3.{names[2]}.weight"])

    # per-expert layout -> another stage: the same model
    b = CausalLMStage(spec, 0, 2).init_random(6)
    for x, y in zip(a.block.layers, b.block.layers):
        y.load_hf_state_dict({k: v.clone() for k, v in x.hf_state_dict().items()})
    # fused 3-D layout (either prefix) -> a third
    c = CausalLMStage(spec, 0, 2).init_random(7)
    for x, y in zip(a.block.layers, c.block.layers):
        per = x.hf_state_dict()
        fused = {k: v.clone() for k, v in per.items() if "experts." not in k}
        fused[pre + "experts.gate_up_proj"] = torch.stack(
            [torch.cat([per[f"{pre}experts.{e}.{names[0]}.weight"],
                        per[f"{pre}experts.{e}.{names[1]}.weight"]], 0) for e in range(E)])
        fused[pre + "experts.down_proj"] = torch.stack(
            [per[f"{pre}experts.{e}.{names[2]}.weight"] for e in range(E)])
        y.load_hf_state_dict(fused)
    for other in (b, c):
        other.embed.load_state_dict(a.embed.state_dict())
        other.head.load_state_dict(a.head.state_dict())
        for x, y in zip(a.block.layers, other.block.layers):
            assert torch.equal(x.mlp.w_gate_up, y.mlp.w_gate_up)
            assert torch.equal(x.mlp.w_down, y.mlp.w_down)
            assert torch.equal(x.mlp.gate.weight, y.mlp.gate.weight)
    ya, yb = _run_stage(a, PROMPTS, decode_steps=1), _run_stage(b, PROMPTS, decode_steps=1)
    assert all(torch.equal(x, y) for x, y in zip(ya, yb))
    missing = {k: v for k, v in sd.items() if "experts.5." not in k}
    with pytest.raises(KeyError, match="experts.5"):
        b.block.layers[0].load_hf_state_dict(missing)
    with pytest.raises(KeyError, match="gate.weight"):
        b.block.layers[0].load_hf_state_dict({k: v for k, v in sd.items() if "gate.weight" not in k})


def test_checkpoint_dir_round_trip(tmp_path):
    pytest.importorskip("safetensors")
    from distributed_llm_inference.utils.model import build_stage, save_random_checkpoint
    spec = _tiny("mixtral")
    path = str(tmp_path / "ckpt")
    save_random_checkpoint(spec, path, seed=5, shard_layers=1)
    stage = build_stage(path, 0, 2, random_init=False, checkpoint=path)
    want = CausalLMStage(spec, 0, 2).init_random(5)
    assert stage.spec.model_type == "mixtral" and stage.spec.num_experts == 8
    for x, y in zip(want.block.layers, stage.block.layers):
        assert torch.equal(x.mlp.w_gate_up, y.mlp.w_gate_up)
        assert torch.equal(x.mlp.w_down, y.mlp.w_down)


def test_init_random_seeds_every_expert_tensor():
    spec = _tiny()
    a = CausalLMStage(spec, 0, 2).init_random(3)
    b = CausalLMStage(spec, 1, 2).init_random(3)     # any split holds the same weights
    m = a.block.layers[1].mlp
    assert torch.equal(m.w_gate_up, b.block.layers[0].mlp.w_gate_up)
    assert torch.equal(m.w_down, b.block.layers[0].mlp.w_down)
    assert torch.equal(m.gate.weight, b.block.layers[0].mlp.gate.weight)
    assert not torch.equal(m.w_gate_up[0], m.w_gate_up[1])
    assert not torch.equal(m.w_down, a.block.layers[0].mlp.w_down)
    assert 0.015 < m.w_gate_up.float().std().item() < 0.025


# ------------------------------------------------------------------ the reference routing op
def _check_grouping(r, T, E, k):
    P = T * k
    ids = r.topk_ids.reshape(-1).long()
    pairs = r.sorted_pairs.long()
    assert sorted(pairs.tolist()) == list(range(P))                # every pair exactly once
    cnt = r.expert_count.long()
    assert int(cnt.sum()) == P and torch.equal(cnt, torch.bincount(ids, minlength=E))
    off = r.expert_offset.long()
    assert off[0] == 0 and torch.equal(off[1:], cnt.cumsum(0))
    for e in range(E):
        seg = pairs[off[e]:off[e + 1]]
        assert bool((ids[seg] == e).all())
        assert bool((seg[1:] > seg[:-1]).all())                    # stable: ascending inside e
    n = int(r.n_tiles)
    assert n == int(((cnt + 31) // 32).sum()) <= ops.moe_tile_capacity(T, E, k) == r.tile_rows.numel()
    te, ts, tr = (t[:n].long() for t in (r.tile_expert, r.tile_start, r.tile_rows))
    assert bool((tr >= 1).all()) and bool((tr <= 32).all())
    pos = 0
    for i in range(n):                                             # tiles partition the ranges
        assert ts[i] == pos and off[te[i]] <= ts[i] and ts[i] + tr[i] <= off[te[i] + 1]
        assert i == 0 or te[i] >= te[i - 1]
        pos += int(tr[i])
    assert pos == P


@pytest.mark.parametrize("T,E,k,renorm", [(1, 8, 2, True), (7, 8, 2, False), (33, 128, 8, True),
                                          (300, 16, 4, True)])
def test_reference_moe_route(T, E, k, renorm):
    g = torch.Generator().manual_seed(T + E)
    # every row a permutation of E distinct bf16 values: torch.topk has one answer
    vals = (torch.arange(E, dtype=torch.float32) - E / 2) / 16
    logits = torch.stack([vals[torch.randperm(E, generator=g)] for _ in range(T)]).to(BF)
    r = ops.moe_route(logits, k, renorm)
    probs = torch.softmax(logits.float(), -1)
    w, ids = torch.topk(probs, k, dim=-1)
    if renorm:
        w = w / w.sum(-1, keepdim=True)
    assert r.topk_ids.dtype == torch.int32 and torch.equal(r.topk_ids.long(), ids)
    assert r.topk_w.dtype == torch.float32 and torch.equal(r.topk_w, w.to(BF).float())
    _check_grouping(r, T, E, k)


def test_reference_moe_route_tie_rule_and_skew():
    # equal logits: the k lowest indices, equal weights
    r = ops.moe_route(torch.zeros(3, 8, dtype=BF), 2, True)
    assert r.topk_ids.tolist() == [[0, 1]] * 3 and r.topk_w.tolist() == [[0.5, 0.5]] * 3
    # a tie across the boundary: the lower index wins, and -0 ties with +0
    lg = torch.tensor([[1.0, 3.0, 2.0, 2.0, 2.0, 0.0], [-0.0, 0.0, -1.0, 0.0, -0.0, -2.0]]).to(BF)
    r = ops.moe_route(lg, 3, False)
    assert r.topk_ids.tolist() == [[1, 2, 3], [0, 1, 3]]
    # everything on one expert: 70 rows -> tiles of 32, 32, 6
    ids = torch.full((70, 1), 5, dtype=torch.int32)
    g = ops.moe_group(ids, torch.ones(70, 1), 8)
    _check_grouping(g, 70, 8, 1)
    assert int(g.n_tiles) == 3 and g.tile_rows[:3].tolist() == [32, 32, 6]
    assert g.tile_expert[:3].tolist() == [5, 5, 5] and g.sorted_pairs.tolist() == list(range(70))


def test_reference_moe_mlp_is_the_dense_definition():
    """ops.moe_mlp on the CPU against the definition written out per token in fp32 with the
    stated rounding points."""
    gen = torch.Generator().manual_seed(9)
    T, H, I, E, k = 19, 128, 128, 8, 2
    x = torch.randn(T, H, generator=gen).to(BF)
    wg = (0.1 * torch.randn(E, I, H, generator=gen)).to(BF)
    wu = (0.1 * torch.randn(E, I, H, generator=gen)).to(BF)
    wd = (0.1 * torch.randn(E, H, I, generator=gen)).to(BF)
    logits = torch.randn(T, E, generator=gen).to(BF)
    w_gate_up = torch.stack([ops.swiglu_interleave(torch.cat([wg[e], wu[e]], 0)) for e in range(E)])
    got = ops.moe_mlp(x, logits, w_gate_up, wd, k, True)
    ids, w = ref.moe_topk(logits, k, True)
    want = torch.zeros(T, H)
    for t in range(T):
        for s in range(k):
            e = int(ids[t, s])
            gate = (x[t].float() @ wg[e].float().t()).to(BF).float()
            up = (x[t].float() @ wu[e].float().t()).to(BF).float()
            h = (torch.nn.functional.silu(gate) * up).to(BF).float()
            want[t] += w[t, s] * (h @ wd[e].float().t()).to(BF).float()
    assert got.dtype == BF
    # the same values up to the summation order inside the products: a bf16 ulp here and there
    assert (got.float() - want.to(BF).float()).abs().max().item() <= 2.0 ** -6 * want.abs().max().item()


def test_quantise_calls_raise_and_dense_models_are_unchanged():
    for mt in ("qwen3_moe", "mixtral"):
        for call in ("quantize_fp8", "quantize_int8", "quantize_mxfp4"):
            stage = CausalLMStage(_tiny(mt), 0, 2).init_random(0)
            with pytest.raises(ValueError, match="sparse MoE"):
                getattr(stage, call)()
            with pytest.raises(ValueError, match="sparse MoE"):
                getattr(stage.block, call)()
        with pytest.raises(ValueError, match="sparse MoE"):
            CausalLMStage(_tiny(mt), 0, 2).init_random(0).quantize("fp8")
    stage = CausalLMStage(_tiny(), 0, 2).init_random(0)
    before = stage.block.layers[0].mlp.w_gate_up.clone()
    stage.block.set_fused_swiglu(True)      # a no-op for the experts
    stage.block.set_fused_swiglu(False)
    assert torch.equal(stage.block.layers[0].mlp.w_gate_up, before)

    for name in ("tiny-llama", "tiny-gpt2", "llama-3-8b", "qwen3-8b", "mistral-7b"):
        assert PRESETS[name].num_experts == 0
    llama = CausalLMStage(PRESETS["tiny-llama"], 0, 2)
    assert isinstance(llama.block.layers[0].mlp, LlamaMLP) and not llama.block.layers[0].is_moe
    assert sorted(llama.block.layers[0].state_dict()) == [
        "input_layernorm.weight", "mlp.down_proj.weight", "mlp.gate_up_proj.weight",
        "post_attention_layernorm.weight", "self_attn.o_proj.weight", "self_attn.qkv_proj.weight"]
    h, i = 4096, 14336
    assert PRESETS["llama-3-8b"].layer_param_count() == h * 6144 + 4096 * h + 3 * h * i + 2 * h
