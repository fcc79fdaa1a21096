"""Int4 group-quantised weights on the CPU: synthetic AWQ / GPTQ checkpoints load integer for
integer and compute what their dequantised twins compute; the refusals; the RTN quantiser, the
nibble packing and the oracle's bound; plan's bytes per parameter."""
import io
import json
from contextlib import redirect_stdout

import pytest
import torch
from safetensors.torch import save_file

from distributed_llm_inference import cli, ops
from distributed_llm_inference.config import ModelSpec, refuse_moe_quantization
from distributed_llm_inference.models.stage import make_block
from distributed_llm_inference.ops.reference import dequant_int4, pack_int4, unpack_int4
from distributed_llm_inference.utils.model import load_block
from test_int4_gpu import int4_case, within_int4_bound

BF = torch.bfloat16
ATOL, RTOL = 2e-2, 2e-2      # tests/test_moe_fp8_block_cpu.py's tolerance
H, I = 256, 512
SPEC = ModelSpec(name="l-int4", vocab_size=512, hidden_size=H, intermediate_size=I, num_layers=1,
                 num_heads=2, num_kv_heads=1, head_dim=128, max_position_embeddings=4096)
AWQ = dict(quant_method="awq", bits=4, group_size=128, zero_point=True, version="GEMM")
GPTQ = dict(quant_method="gptq", bits=4, group_size=128, desc_act=False, sym=False)
PROJ = dict(q=("self_attn.q_proj", H, H), k=("self_attn.k_proj", 128, H),
            v=("self_attn.v_proj", 128, H), o=("self_attn.o_proj", H, H),
            gate=("mlp.gate_proj", I, H), up=("mlp.up_proj", I, H), down=("mlp.down_proj", H, I))
AWQ_ORDER = [0, 2, 4, 6, 1, 3, 5, 7]


def _words(nib):
    """[..., 8] nibbles (nibble i = bits 4 i .. 4 i + 3) -> int32 words."""
    w = (nib.long() << (4 * torch.arange(8))).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def _write(root, name, qcfg, ints):
    """One layer in the hub's layout from the integers ``ints[p] = (q [N, K], s [G, N], z [G, N])``."""
    sd = {"input_layernorm.weight": torch.ones(H, dtype=torch.float16),
          "post_attention_layernorm.weight": torch.full((H,), 0.5, dtype=torch.float16)}
    for p, (key, N, K) in PROJ.items():
        q, s, z = ints[p]
        if qcfg["quant_method"] == "awq":   # columns 8 j + ORDER[i] in nibble i, qweight [K, N / 8]
            qw = _words(q.t().reshape(K, N // 8, 8)[..., AWQ_ORDER])
            qz = _words(z.reshape(-1, N // 8, 8)[..., AWQ_ORDER])
        else:   # qweight [K / 8, N]: k = 8 r + i in nibble i; qzeros sequential, v1 stores z - 1
            qw = _words(q.t().reshape(K // 8, 8, N).transpose(1, 2))
            zs = z if qcfg.get("checkpoint_format") == "gptq_v2" else (z.long() - 1) & 15
            qz = _words(zs.reshape(-1, N // 8, 8))
            sd[key + ".g_idx"] = (torch.arange(K) // 128).to(torch.int32)
        sd.update({key + ".qweight": qw, key + ".qzeros": qz, key + ".scales": s})
    (root / name).mkdir()
    save_file({"model.layers.0." + k: v.contiguous() for k, v in sd.items()},
              str(root / name / "model.safetensors"))
    (root / name / "config.json").write_text(json.dumps(dict(SPEC.to_hf_dict(),
                                                             quantization_config=qcfg)))
    return str(root / name), sd


@pytest.fixture(scope="module")
def ints():
    g = torch.Generator().manual_seed(7)
    return {p: (torch.randint(0, 16, (N, K), generator=g).to(torch.uint8),
                (torch.rand(K // 128, N, generator=g) * 0.01 + 0.002).to(torch.float16),
                torch.randint(0, 16, (K // 128, N), generator=g).to(torch.uint8))
            for p, (_, N, K) in PROJ.items()}


@pytest.mark.parametrize("name,qcfg,quant", [
    ("awq", AWQ, "int4_awq"), ("gptq", GPTQ, "int4_gptq"),
    ("gptq_sym", dict(GPTQ, sym=True), "int4_gptq"),
    ("gptq_v2", dict(GPTQ, checkpoint_format="gptq_v2"), "int4_gptq")])
def test_checkpoint_loads_integers_exactly_and_matches_bf16_twin(tmp_path, ints, name, qcfg, quant):
    path, sd = _write(tmp_path, name, qcfg, ints)
    spec = ModelSpec.from_hf_config(path)
    assert spec.weight_quant == quant
    assert ModelSpec.from_hf_config(spec.to_hf_dict()).int4_checkpoint == spec.int4_checkpoint
    lq = load_block(path, [0]).layers[0]                           # no flag: int4 as stored
    lb = load_block(path, [0], use_quantized="bf16").layers[0]
    cat = {n: [torch.cat([ints[p][i] for p in ps], 0 if i == 0 else 1) for i in range(3)]
           for n, ps in (("qkv", "qkv"), ("o", ["o"]), ("gu", ["gate", "up"]), ("down", ["down"]))}
    lins = dict(qkv=lq.self_attn.qkv_proj, o=lq.self_attn.o_proj, gu=lq.mlp.gate_up_proj,
                down=lq.mlp.down_proj)
    for n, lin in lins.items():
        assert lin.is_int4 and lin.weight.numel() == 0
        for got, want in zip((unpack_int4(lin.weight_int4), lin.weight_int4_scale,
                              lin.weight_int4_zero), cat[n]):
            assert torch.equal(got, want), n
    assert not lb.mlp.down_proj.is_int4 and lb.input_layernorm.weight.dtype == BF
    assert torch.equal(lb.mlp.down_proj.weight, dequant_int4(pack_int4(cat["down"][0]),
                                                             *cat["down"][1:]))
    x = torch.randn(24, H, generator=torch.Generator().manual_seed(2)).to(BF)
    with torch.no_grad():
        got, want = lq.mlp(x).float(), lb.mlp(x).float()
    assert want.abs().max() > 0.5 and bool(((got - want).abs() <= ATOL + RTOL * want.abs()).all())
    # the SwiGLU interleave moves q, s and z together -- at load and afterwards
    lf = make_block(spec, [0]).layers[0]
    lf.mlp.set_fused_swiglu(True)
    lf.load_hf_state_dict(sd, int4=spec.int4_checkpoint)
    lq.mlp.set_fused_swiglu(True)
    ga, gb = lf.mlp.gate_up_proj, lq.mlp.gate_up_proj
    assert torch.equal(unpack_int4(ga.weight_int4), ops.swiglu_interleave(cat["gu"][0]))
    assert torch.equal(ga.weight_int4_scale.t(), ops.swiglu_interleave(cat["gu"][1].t()))
    assert all(torch.equal(getattr(ga, n), getattr(gb, n))
               for n in ("weight_int4", "weight_int4_scale", "weight_int4_zero"))


@pytest.mark.parametrize("field,qcfg", [
    ("bits", dict(AWQ, bits=8)), ("group_size", dict(GPTQ, group_size=64)),
    ("desc_act", dict(GPTQ, desc_act=True)), ("version", dict(AWQ, version="gemv")),
    ("zero_point", dict(AWQ, zero_point=False))])
def test_config_refusals(field, qcfg):
    with pytest.raises(ValueError, match=field):
        ModelSpec.from_hf_config(dict(SPEC.to_hf_dict(), quantization_config=qcfg))


def test_loader_and_mode_refusals(tmp_path, ints):
    path, sd = _write(tmp_path, "gptq", GPTQ, ints)
    sd["mlp.up_proj.g_idx"] = sd["mlp.up_proj.g_idx"].flip(0)
    with pytest.raises(ValueError, match="g_idx"):
        make_block(SPEC, [0]).layers[0].load_hf_state_dict(sd, int4="gptq")
    with pytest.raises(ValueError, match="fp8.*int4"):
        load_block(path, [0], use_quantized="fp8")
    moe = ModelSpec(name="m", model_type="qwen3_moe", qk_norm=True, num_experts=4,
                    num_experts_per_tok=2, moe_intermediate_size=128, head_dim=128)
    with pytest.raises(ValueError, match="int4"):
        refuse_moe_quantization(moe, "int4")


@pytest.mark.parametrize("field,kw", [
    ("K % 128", dict(K=192)), ("N % 32", dict(N=48)),
    ("scale must be \\[K / 128, N\\]", dict(s_shape=(64, 2))),
    ("scale must be float16", dict(s_dtype=torch.float32)),
    ("zero must be uint8", dict(z_dtype=torch.int32)),
    ("x must be bfloat16", dict(x_dtype=torch.float32)), ("bias", dict(bias_n=32))])
def test_shape_refusals(field, kw):
    N, K = kw.get("N", 64), kw.get("K", 256)
    x = torch.zeros(4, K, dtype=kw.get("x_dtype", BF))
    scale = torch.ones(kw.get("s_shape", (K // 128, N)), dtype=kw.get("s_dtype", torch.float16))
    zero = torch.zeros(K // 128, N, dtype=kw.get("z_dtype", torch.uint8))
    bias = torch.zeros(kw["bias_n"], dtype=BF) if "bias_n" in kw else None
    with pytest.raises(ValueError, match=field):
        ops.linear_int4(x, torch.zeros(N, K // 2, dtype=torch.uint8), scale, zero, bias)


def test_quantiser_round_trip_and_packing():
    g = torch.Generator().manual_seed(5)
    q = torch.randint(0, 16, (32, 256), generator=g).to(torch.uint8)
    assert torch.equal(unpack_int4(pack_int4(q)), q)
    word = pack_int4(torch.arange(8)[None]).view(torch.int32).item()   # nibble p = element ORDER[p]
    assert [(word >> (4 * p)) & 15 for p in range(8)] == AWQ_ORDER
    w = torch.randn(64, 384, generator=g) * torch.exp2(torch.randint(-8, 3, (64, 1), generator=g))
    w[3, :128] = 0.25                                                  # a constant group: s = 1
    wq, s, z = ops.quantize_int4(w.to(BF))
    sf = s.float().t().repeat_interleave(128, 1)
    assert s[0, 3] == 1 and z.max() <= 15 and unpack_int4(wq).max() <= 15
    # |dequant - w| <= s / 2, plus 15 steps of fp16's 2^-11 rounding of s
    err = (dequant_int4(wq, s, z, torch.float32) - w.to(BF).float()).abs()
    assert bool((err <= sf * (0.5 + 15 * 2.0 ** -11)).all())


@pytest.mark.parametrize("N,K", [(128, 128), (256, 1024)])
def test_cpu_oracle_within_the_gpu_bound(N, K):
    case = int4_case("real", N, K)
    for M in (1, 32):
        y = ops.linear_int4(case[4][:M], *case[:4]).double()
        assert within_int4_bound(y, case, M, K, True)


def test_plan_counts_int4_bytes():
    buf = io.StringIO()
    with redirect_stdout(buf):
        assert cli.main(["plan", "--model", "llama-3-70b", "--gpus", "1", "--int4"]) == 0
    assert json.loads(buf.getvalue())["weight_bytes_per_param"] == 1 / 2 + 3 / 128
