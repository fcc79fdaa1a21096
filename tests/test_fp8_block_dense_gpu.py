"""Dense block-scaled fp8 linears (ops.linear_fp8_block: gemm_fp8_block_small.hip at 1-32 rows,
gemm_fp8_block_tile.hip beyond): an exact scale-index probe, the fp64 reference on real-valued
operands, the SwiGLU epilogue, the mode end to end, and the host's shape refusals."""
import pytest
import torch

from distributed_llm_inference import ops
from distributed_llm_inference.config import CacheConfig, ModelSpec, ServeConfig
from distributed_llm_inference.models import CausalLMStage
from distributed_llm_inference.models.common import Linear
from distributed_llm_inference.ops.reference import expand_fp8_block_scale
from distributed_llm_inference.runtime.engine import EngineConfig, LLMEngine
from distributed_llm_inference.runtime.sequence import SamplingParams

BF, FP8 = torch.bfloat16, torch.float8_e4m3fn
SMALL_M, TILE_M = (1, 2, 3, 16, 17, 32), (33, 128, 129, 257)
MAX_M = 257
# Qwen3-shaped: per-head q/k RMSNorm, no biases; qkv 384, o 256, gate|up 1024, down 256 x 512
SPEC = ModelSpec(name="q3", model_type="qwen3", vocab_size=1000, hidden_size=256,
                 intermediate_size=512, num_layers=2, num_heads=8, num_kv_heads=2, head_dim=32,
                 rope_theta=10000.0, max_position_embeddings=4096, qk_norm=True)
_CASES = {}


def _case(kind, N, K):
    """(w8 [N, K], scale [N / 16, K / 128], bias [N], x [MAX_M, K] bf16, fp64 product without
    bias [MAX_M, N], fp64 sum of |x| |w| s [MAX_M, N]), built once per shape and never modified.
    "probe": weights in {0, +-1, +-2}, scale 2^(3 group + block - 36) -- distinct per (group, block),
    the blocks of a group one binade apart -- x with +-1 / +-2 at two k per block and a bias that is
    a small multiple of the group's smallest scale: every partial sum is an integer below 2^6
    times a power of two, exact in fp32 and in bf16.  "real": a seeded normal weight whose 16 x 128
    blocks span 2^-10 .. 2^2, quantised by ops.quantize_expert_weights_fp8_block."""
    if (kind, N, K) in _CASES:
        return _CASES[kind, N, K]
    g = torch.Generator().manual_seed(1000 * N + K)
    gn, gk = N // 16, K // 128
    if kind == "probe":
        w8 = torch.randint(-2, 3, (N, K), generator=g).float().to(FP8)
        ex = 3 * torch.arange(gn)[:, None] + torch.arange(gk)[None, :] - 36
        scale = torch.exp2(ex.float())
        x = torch.zeros(MAX_M, gk, 128)
        pos = torch.rand(MAX_M, gk, 128, generator=g).argsort(-1)[..., :2]
        x.scatter_(-1, pos, torch.tensor([1., -1., 2., -2.])[
            torch.randint(0, 4, (MAX_M, gk, 2), generator=g)])
        x = x.reshape(MAX_M, K).to(BF)
        bias = (torch.randint(-3, 4, (N,), generator=g).float()
                * scale[:, 0].repeat_interleave(16)).to(BF)
    else:
        w = torch.randn(N, K, generator=g) * expand_fp8_block_scale(
            torch.exp2(torch.randint(-10, 3, (gn, gk), generator=g).float()))
        w8, scale = (t[0] for t in ops.quantize_expert_weights_fp8_block(w[None]))
        x = torch.randn(MAX_M, K, generator=g).to(BF)
        bias = torch.randn(N, generator=g).to(BF)
    wd = w8.double() * expand_fp8_block_scale(scale).double()
    _CASES[kind, N, K] = (w8, scale, bias, x, x.double() @ wd.t(), x.double().abs() @ wd.abs().t())
    return _CASES[kind, N, K]


def _run(case, M, with_bias, dev, swiglu=False):
    w8, scale, bias, x = (t.to(dev) for t in case[:4])
    return ops.linear_fp8_block(x[:M].contiguous(), w8, scale, bias if with_bias else None,
                                swiglu=swiglu).double().cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("M", SMALL_M + TILE_M)
@pytest.mark.parametrize("N,K", [(128, 128), (384, 128), (128, 384), (384, 384)])
def test_scale_index_probe_exact(gpu, M, N, K):
    """A wrong group or block index, a wrong clamp or a missed partial tile changes an exact
    answer."""
    case = _case("probe", N, K)
    with_bias = (M + N // 128 + K // 128) % 2 == 0
    want = case[4][:M] + (case[2].double() if with_bias else 0)
    assert torch.equal(_run(case, M, with_bias, gpu), want)


def _within_bound(y, case, M, K, with_bias):
    """|y - y64| <= 2^-8 |y64| (one bf16 rounding) + K 2^-23 sum_k |x| |w| s (fp32 accumulation,
    loose); a bias adds its magnitude to the sum of the second term."""
    y64 = case[4][:M] + (case[2].double() if with_bias else 0)
    mag = case[5][:M] + (case[2].double().abs() if with_bias else 0)
    err, tol = (y - y64).abs(), 2.0 ** -8 * y64.abs() + K * 2.0 ** -23 * mag
    print(f"max err / bound = {(err / tol.clamp_min(1e-300)).max().item():.3f}")
    return bool((err <= tol).all())


@pytest.mark.gpu
@pytest.mark.parametrize("M", SMALL_M + TILE_M)
@pytest.mark.parametrize("N,K", [(128, 128), (256, 128), (128, 1024), (256, 1024)])
def test_matches_fp64_reference(gpu, M, N, K):
    with_bias = (M + N // 128) % 2 == 0
    case = _case("real", N, K)
    assert _within_bound(_run(case, M, with_bias, gpu), case, M, K, with_bias)


@pytest.mark.parametrize("N,K", [(128, 128), (256, 1024)])
def test_cpu_oracle_within_the_same_bound(N, K):
    """The bound of test_matches_fp64_reference holds for the reference alone."""
    case = _case("real", N, K)
    for M in (1, 32, MAX_M):
        assert _within_bound(_run(case, M, True, "cpu"), case, M, K, True)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [5, 32, 200])
def test_swiglu_epilogue_bit_equal(gpu, M):
    """Same kernel, same accumulation order: the fused epilogue is ops.swiglu_interleaved of the
    plain output (gate and up rounded to bf16, then silu(gate) * up rounded once)."""
    case = _case("real", 256, 1024)
    plain = _run(case, M, False, gpu).to(BF).to(gpu)
    assert torch.equal(_run(case, M, False, gpu, swiglu=True),
                       ops.swiglu_interleaved(plain).double().cpu())


def _stage_logits(stage, prompts):
    pool = stage.make_pool(128, block_size=64)
    sids = list(range(len(prompts)))
    for s, p in zip(sids, prompts):
        pool.manager.append(s, len(p))
    meta = pool.build_metadata(sids, [len(p) for p in prompts])
    meta.logits_rows = (torch.cumsum(torch.tensor([len(p) for p in prompts]), 0) - 1).to(stage.device)
    ids = torch.tensor([t for p in prompts for t in p], dtype=torch.int32, device=stage.device)
    return stage(ids, meta, pool).float().cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("lens", [(2,), (12, 8), (100, 50)])
def test_stage_gpu_matches_cpu(gpu, monkeypatch, lens):
    """2, 20 and 150 rows: every projection of both layers runs the small / the tile kernel on the
    GPU (gate|up with its SwiGLU epilogue) and the op's oracle on the CPU stage; the tolerance of
    tests/test_fp8_small_gpu.py::test_fp8_small_stage_gpu_matches_cpu."""
    prompts = [[(7 * i + 3 * j) % 1000 for j in range(n)] for i, n in enumerate(lens)]
    cpu = CausalLMStage(SPEC, 0, 2).init_random(3)
    g = CausalLMStage(SPEC, 0, 2, device=gpu).init_random(3)
    g.load_state_dict({k: v.to(gpu) for k, v in cpu.state_dict().items()})
    cpu.quantize("fp8_block")
    g.quantize("fp8_block")
    g.block.set_fused_swiglu(True)
    lins = [m for m in g.block.modules() if isinstance(m, Linear)]
    assert len(lins) == 8 and all(m.is_fp8_block and not m.is_fp8 for m in lins)
    x = _stage_logits(cpu, prompts)
    rows, real = [], ops.linear_fp8_block
    monkeypatch.setattr(ops, "linear_fp8_block",
                        lambda *a, **kw: (rows.append(a[0].shape[0]), real(*a, **kw))[1])
    y = _stage_logits(g, prompts)
    assert rows == [sum(lens)] * 8, rows             # QKV, O, gate|up, down x 2 layers
    err = (x - y).abs().max().item()
    assert err < 0.03 * max(1.0, x.abs().max().item()), err


@pytest.mark.gpu
def test_engine_graph_decode_equals_eager(gpu):
    """Prefill chunks of 37 and 130 rows on the tile kernel, decode steps of 4 rows on the small
    kernel, eagerly and captured into the bucket's hipGraph: token for token the same."""
    def engine(graphs):
        cfg = EngineConfig(model="q3", pp=1, seed=5, quantize="fp8_block",
                           cache=CacheConfig(num_blocks=256, block_size=64, max_chunk=256),
                           serve=ServeConfig(max_batch_size=8, max_num_batched_tokens=512,
                                             max_seq_len=1024, use_graphs=graphs,
                                             graph_batch_sizes=[1, 2, 4, 8]))
        return LLMEngine(SPEC, device="cuda:0", cfg=cfg)
    prompts = [list(range(3, 40)), [7, 8, 9], list(range(200, 330)), [11]]
    p = SamplingParams(max_tokens=10, ignore_eos=True)
    eng = engine(False)
    lins = [m for m in eng.executors[0].stage.block.modules() if isinstance(m, Linear)]
    assert lins and all(m.is_fp8_block for m in lins)
    a = [s.output for s in eng.generate(prompts, p)]
    b = [s.output for s in engine(True).generate(prompts, p)]
    assert all(len(o) == 10 for o in a) and a == b


@pytest.mark.parametrize("field,kw", [
    ("K % 128", dict(K=192)),
    ("N % 128", dict(N=192)),
    ("scale must be \\[N / 16, K / 128\\]", dict(scale_shape=(1, 2))),   # the checkpoint's 128 rows
    ("x must be bfloat16", dict(x_dtype=torch.float32)),
    ("w8 must be float8_e4m3fn", dict(w_dtype=torch.uint8)),
    ("scale must be float32", dict(s_dtype=BF)),
    ("bias", dict(bias_n=64)),
])
def test_shape_refusals(field, kw):
    N, K = kw.get("N", 128), kw.get("K", 256)
    x = torch.zeros(4, K, dtype=kw.get("x_dtype", BF))
    w8 = torch.zeros(N, K).to(kw.get("w_dtype", FP8))
    scale = torch.ones(kw.get("scale_shape", (N // 16, K // 128)), dtype=kw.get("s_dtype",
                                                                                 torch.float32))
    bias = torch.zeros(kw["bias_n"], dtype=BF) if "bias_n" in kw else None
    with pytest.raises(ValueError, match=field):
        ops.linear_fp8_block(x, w8, scale, bias)
