"""Qwen3 (per-head q/k RMSNorm before RoPE) on the CPU reference path: parity with the installed
HF implementation, config / state-dict round trips, the reference op's composition, init and
presets.  The kernel that fuses the norm into the RoPE / KV write is pinned by
tests/test_qwen3_gpu.py."""
import pytest
import torch

from distributed_llm_inference.config import PRESETS, ModelSpec, plan_stages
from distributed_llm_inference.models import CausalLMStage
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
    gen = torch.stack([o.argmax(-1) for o in stage_logits], 1)
    for b, p in enumerate(prompts):
        seq = torch.tensor(p + gen[b, :steps].tolist())[None]
        with torch.no_grad():
            ref_logits = hf(seq).logits[0].float()
        for s in range(steps + 1):
            a, r = stage_logits[s][b], ref_logits[len(p) - 1 + s]
            err = (a - r).abs().max().item()
            assert err < 0.05 * max(1.0, r.abs().max().item()), f"b={b} step={s} err={err}"


def _hf_qwen3(seed=1):
    """Tiny HF Qwen3: head_dim 64 with 4 heads on hidden 128, so q_size = 256 != hidden."""
    pytest.importorskip("transformers")
    from transformers import Qwen3Config, Qwen3ForCausalLM
    torch.manual_seed(seed)
    cfg = Qwen3Config(vocab_size=256, hidden_size=128, intermediate_size=256, num_hidden_layers=2,
                      num_attention_heads=4, num_key_value_heads=2, head_dim=64, rms_norm_eps=1e-6,
                      max_position_embeddings=4096, tie_word_embeddings=False,
                      rope_parameters={"rope_type": "default", "rope_theta": 1000000.0})
    m = Qwen3ForCausalLM(cfg).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith(("q_norm.weight", "k_norm.weight")):   # HF inits them to 1
                p.normal_(1.0, 0.3)
            p.copy_(p.to(BF).float())
    return m


def test_qwen3_matches_hf():
    """Qwen3 = Llama with per-head q/k RMSNorm before RoPE and an explicit head_dim; prefill of
    two prompts and three decode steps against HF, the criterion of test_qwen2_matches_hf."""
    from distributed_llm_inference.utils.model import stage_from_hf_model
    hf = _hf_qwen3()
    stage = stage_from_hf_model(hf, 0, hf.config.num_hidden_layers)
    spec = stage.spec
    assert spec.model_type == "qwen3" and spec.qk_norm
    assert not spec.attention_bias and not spec.has_o_proj_bias
    assert spec.head_dim == 64 and spec.q_size == 256 != spec.hidden_size
    attn = stage.block.layers[0].self_attn
    assert attn.o_proj.in_features == 256 and attn.q_norm.weight.shape == (64,)
    hf_w = hf.model.layers[1].self_attn.k_norm.weight
    assert torch.equal(stage.block.layers[1].self_attn.k_norm.weight.float(), hf_w.float())
    prompts = [[5, 17, 99, 3, 250, 7, 7, 1], [8, 2, 64]]
    _check_against_hf(hf, _run_stage(stage, prompts, decode_steps=3), prompts, 3)


def _tiny_spec(**kw):
    return ModelSpec(name="tiny-qwen3", model_type="qwen3", qk_norm=True, vocab_size=256,
                     hidden_size=128, intermediate_size=256, num_layers=2, num_heads=4,
                     num_kv_heads=2, head_dim=64, rms_norm_eps=1e-6, rope_theta=1000000.0,
                     max_position_embeddings=4096, bos_token_id=1, eos_token_id=2).replace(**kw)


def _randomise_qk_norms(stage, seed=3):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for layer in stage.block.layers:
            for n in (layer.self_attn.q_norm, layer.self_attn.k_norm):
                n.weight.copy_((1 + 0.3 * torch.randn(n.weight.shape, generator=g)).to(BF))


def test_qwen3_config_and_state_dict_round_trip():
    spec = _tiny_spec()
    d = spec.to_hf_dict()
    assert d["model_type"] == "qwen3" and d["architectures"] == ["Qwen3ForCausalLM"]
    assert d["head_dim"] == 64
    assert ModelSpec.from_hf_config(d).replace(name=spec.name) == spec
    windowed = spec.replace(sliding_window=32)
    assert ModelSpec.from_hf_config(windowed.to_hf_dict()).replace(name=spec.name) == windowed
    for name in ("qwen3-8b", "qwen3-32b", "qwen3-0.6b"):
        p = PRESETS[name]
        assert ModelSpec.from_hf_config(p.to_hf_dict()).replace(name=p.name) == p
    # sliding-window keys are ignored unless use_sliding_window, as for Qwen2
    assert ModelSpec.from_hf_config(dict(d, sliding_window=4096)).sliding_window is None
    # windowed and full-attention layers mixed: one window per model, so refuse
    with pytest.raises(ValueError, match="max_window_layers"):
        ModelSpec.from_hf_config(dict(d, use_sliding_window=True, sliding_window=32,
                                      max_window_layers=1))

    a = CausalLMStage(spec, 0, 2).init_random(5)
    _randomise_qk_norms(a)
    sd = a.block.layers[0].hf_state_dict()
    assert "self_attn.q_norm.weight" in sd and "self_attn.k_norm.weight" in sd
    assert "self_attn.q_proj.bias" not in sd
    b = CausalLMStage(spec, 0, 2).init_random(6)      # other weights everywhere ...
    for la, lb in zip(a.block.layers, b.block.layers):
        lb.load_hf_state_dict({k: v.clone() for k, v in la.hf_state_dict().items()})
    b.embed.load_state_dict(a.embed.state_dict())
    b.head.load_state_dict(a.head.state_dict())
    prompts = [[5, 17, 99, 3, 250, 7, 7, 1], [8, 2, 64]]
    ya, yb = _run_stage(a, prompts, decode_steps=1), _run_stage(b, prompts, decode_steps=1)
    assert all(torch.equal(x, y) for x, y in zip(ya, yb))   # ... the same model after loading
    # a layer state dict without the norm weights is refused, not silently left at 1
    missing = {k: v for k, v in sd.items() if "q_norm" not in k}
    with pytest.raises(KeyError, match="q_norm"):
        b.block.layers[0].load_hf_state_dict(missing)


def test_qwen3_checkpoint_dir_loads_the_norm_weights(tmp_path):
    """A sharded checkpoint directory: config.json is parsed as Qwen3 and the per-layer selective
    loader hands q_norm / k_norm through (a layer state dict without them raises)."""
    pytest.importorskip("safetensors")
    from safetensors.torch import load_file, save_file
    from distributed_llm_inference.utils.model import (build_stage, load_block,
                                                       save_random_checkpoint)
    spec = _tiny_spec()
    path = str(tmp_path / "ckpt")
    save_random_checkpoint(spec, path, seed=5, shard_layers=1)
    # init_random leaves the norm weights at 1: overwrite layer 1's in its shard so they matter
    shard = str(tmp_path / "ckpt" / "model-00002-of-00003.safetensors")
    sd = load_file(shard)
    key = "model.layers.1.self_attn.k_norm.weight"
    assert key in sd and "model.layers.1.self_attn.q_norm.weight" in sd
    sd[key] = (1 + 0.3 * torch.randn(64, generator=torch.Generator().manual_seed(1))).to(BF)
    save_file(sd, shard)
    stage = build_stage(path, 0, 2, random_init=False, checkpoint=path)
    assert stage.spec.qk_norm and stage.spec.model_type == "qwen3"
    assert torch.equal(stage.block.layers[1].self_attn.k_norm.weight, sd[key])
    assert bool((stage.block.layers[0].self_attn.k_norm.weight == 1).all())
    block = load_block(path, [1])
    assert torch.equal(block.layers[0].self_attn.k_norm.weight, sd[key])


def test_reference_rope_cache_with_norms_is_rms_norm_then_rope_cache():
    """ref.rope_cache(..., q_norm, k_norm) == per-head ref.rms_norm of the q and k slices, then
    ref.rope_cache without norms: q, q_sink, K cache and V cache, bit for bit."""
    torch.manual_seed(2)
    nh, nkv, D, T, bs, nblocks, eps = 4, 2, 64, 11, 32, 4, 1e-6
    qkv = torch.randn(T, (nh + 2 * nkv) * D).to(BF)
    qw = (1 + 0.3 * torch.randn(D)).to(BF)
    kw = (1 + 0.3 * torch.randn(D)).to(BF)
    pos = torch.randint(0, 300, (T,), dtype=torch.int32)
    slots = torch.randperm(nblocks * bs)[:T].to(torch.int64)
    slots[4] = -1
    cs = ref.build_cos_sin(D, 512, 1000000.0)
    k0, v0 = torch.randn(nblocks, nkv, bs, D).to(BF), torch.randn(nblocks, nkv, bs // 8, D, 8).to(BF)
    k1, v1, k2, v2 = k0.clone(), v0.clone(), k0.clone(), v0.clone()
    q1, s1 = ref.rope_cache(qkv, pos, slots, cs, nh, nkv, D, k1, v1, 100, True, q_norm=qw,
                            k_norm=kw, norm_eps=eps)
    pre = qkv.clone()
    pre[:, :nh * D] = ref.rms_norm(qkv[:, :nh * D].reshape(T, nh, D), qw, eps)[0].reshape(T, -1)
    pre[:, nh * D:(nh + nkv) * D] = ref.rms_norm(
        qkv[:, nh * D:(nh + nkv) * D].reshape(T, nkv, D), kw, eps)[0].reshape(T, -1)
    assert not torch.equal(pre, qkv)
    q2, s2 = ref.rope_cache(pre, pos, slots, cs, nh, nkv, D, k2, v2, 100, True)
    assert torch.equal(q1, q2) and torch.equal(s1, s2)
    assert torch.equal(k1, k2) and torch.equal(v1, v2)
    assert not torch.equal(k1, k0)
    with pytest.raises(ValueError, match="together"):
        ref.rope_cache(qkv, pos, slots, cs, nh, nkv, D, k1, v1, q_norm=qw)


def test_qwen3_init_presets_and_llama_unchanged():
    stage = CausalLMStage(_tiny_spec(), 0, 2).init_random(0)
    for layer in stage.block.layers:
        a = layer.self_attn
        assert bool((a.q_norm.weight == 1).all()) and bool((a.k_norm.weight == 1).all())
        assert a.q_norm.eps == 1e-6

    p32 = PRESETS["qwen3-32b"]
    assert p32.qk_norm and p32.q_size == 8192 != p32.hidden_size
    plan = plan_stages(p32, 8)
    assert len(plan) == 8 and plan[0][0] == 0 and plan[-1][1] == 64
    assert all(a < b for a, b in plan) and all(x[1] == y[0] for x, y in zip(plan, plan[1:]))
    p06 = PRESETS["qwen3-0.6b"]
    assert p06.tie_word_embeddings and p06.q_size == 2048 != p06.hidden_size
    assert PRESETS["qwen3-8b"].num_layers == 36

    with pytest.raises(ValueError, match="head_dim 96"):
        ModelSpec.from_hf_config(dict(_tiny_spec().to_hf_dict(), head_dim=96))
    with pytest.raises(ValueError, match="qwen3"):    # the supported list names it
        ModelSpec.from_hf_config({"model_type": "qwen3_moe"})

    llama = CausalLMStage(PRESETS["tiny-llama"], 0, 2)
    attn = llama.block.layers[0].self_attn
    assert not PRESETS["tiny-llama"].qk_norm
    assert not hasattr(attn, "q_norm") and not hasattr(attn, "k_norm")
    assert sorted(llama.block.layers[0].state_dict()) == [
        "input_layernorm.weight", "mlp.down_proj.weight", "mlp.gate_up_proj.weight",
        "post_attention_layernorm.weight", "self_attn.o_proj.weight", "self_attn.qkv_proj.weight"]
    assert not any("q_norm" in k for k in llama.block.layers[0].hf_state_dict())
