"""Int4 group-quantised weights on the GPU (ops.linear_int4, gemm_int4.hip: the weight-streaming
MFMA kernel at 1-32 rows, the dequantiser + bf16 GEMM path beyond): an exact probe, the fp64
reference on real-valued operands, the SwiGLU epilogue, the dequantiser, and the mode end to end."""
import pytest
import torch

from distributed_llm_inference import ops
from distributed_llm_inference.config import CacheConfig, ServeConfig
from distributed_llm_inference.models import CausalLMStage
from distributed_llm_inference.models.common import Linear
from distributed_llm_inference.ops.reference import dequant_int4, pack_int4
from distributed_llm_inference.runtime.engine import EngineConfig, LLMEngine
from distributed_llm_inference.runtime.sequence import SamplingParams
from test_fp8_block_dense_gpu import SPEC, _stage_logits

BF = torch.bfloat16
ROWS = (1, 2, 3, 16, 17, 32, 33, 130)
MAX_M = 130
C_WIDENED = 143   # the kernel is built in the offset form: the widened weight is 128 + q <= 143
_CASES = {}


def int4_case(kind, N, K):
    """(wq, scale, zero, bias [N], x [MAX_M, K] bf16, fp64 weight [N, K], fp64 per-k scale [N, K]),
    built once per shape and never modified.  "probe": q and z random in 0..15, scale
    2^(row % 16 + 7 group - 14) -- a power of two in fp16's normal range, distinct over the rows of
    an A tile and over the groups of a row (fp16's 30 normal binades cannot tell 16 rows x 3 groups
    all apart) -- x with +-1 / +-2 at two k per group, a bias that is a small multiple of the row's
    smallest scale: every partial sum, the offset form's sum_k (128 + q) x included, is an integer
    below 2^11 times a power of two and a row's terms span 14 binades, so fp32 is exact in any order.
    "real": a seeded normal weight whose groups span 2^-8 .. 2^2, quantised by ops.quantize_int4."""
    if (kind, N, K) in _CASES:
        return _CASES[kind, N, K]
    g = torch.Generator().manual_seed(1000 * N + K)
    G = K // 128
    if kind == "probe":
        wq = pack_int4(torch.randint(0, 16, (N, K), generator=g))
        zero = torch.randint(0, 16, (G, N), generator=g).to(torch.uint8)
        ex = (torch.arange(N) % 16)[None, :] + 7 * torch.arange(G)[:, None] - 14
        scale = torch.exp2(ex.float()).to(torch.float16)
        x = torch.zeros(MAX_M, G, 128)
        pos = torch.rand(MAX_M, G, 128, generator=g).argsort(-1)[..., :2]
        x.scatter_(-1, pos, torch.tensor([1., -1., 2., -2.])[
            torch.randint(0, 4, (MAX_M, G, 2), generator=g)])
        x = x.reshape(MAX_M, K).to(BF)
        bias = (torch.randint(-3, 4, (N,), generator=g).float() * scale[0].float()).to(BF)
    else:
        w = torch.randn(N, K, generator=g) * torch.exp2(
            torch.randint(-8, 3, (N, G), generator=g).float()).repeat_interleave(128, 1)
        wq, scale, zero = ops.quantize_int4(w)
        x = torch.randn(MAX_M, K, generator=g).to(BF)
        bias = torch.randn(N, generator=g).to(BF)
    _CASES[kind, N, K] = (wq, scale, zero, bias, x,
                          dequant_int4(wq, scale, zero, torch.float64),
                          scale.double().t().repeat_interleave(128, 1))
    return _CASES[kind, N, K]


def _run(case, M, with_bias, dev, swiglu=False):
    wq, scale, zero, bias, x = (t.to(dev) for t in case[:5])
    return ops.linear_int4(x[:M].contiguous(), wq, scale, zero, bias if with_bias else None,
                           swiglu=swiglu).double().cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("N,K", [(128, 128), (384, 128), (128, 384), (160, 256)])
def test_probe_exact(gpu, M, N, K):
    """A wrong nibble position, group, row, zero point or clamp changes an exact answer: fp32 is
    exact on this case, so the kernel's result is the fp64 one rounded to bf16 once."""
    case = int4_case("probe", N, K)
    with_bias = (M + N // 32 + K // 128) % 2 == 0
    want = case[4][:M].double() @ case[5].t() + (case[3].double() if with_bias else 0)
    assert torch.equal(_run(case, M, with_bias, gpu), want.to(BF).double())


def within_int4_bound(y, case, M, K, with_bias):
    """M <= 32: |y - y64| <= 2^-8 |y64| (one bf16 rounding) + K 2^-23 C sum_k |x_k| s_k (fp32
    accumulation, loose; C = 143 is the largest widened weight of the offset form, 128 + q).
    M > 32, the dequantise path: y64 is the product with the bf16-rounded weight, and the bf16
    GEMM's own K 2^-23 sum_k |x_k| |w_k| takes the second term's place."""
    x = case[4][:M].double()
    b = case[3].double() if with_bias else torch.zeros(())
    if M <= 32:
        y64, mag = x @ case[5].t() + b, C_WIDENED * (x.abs() @ case[6].t()) + b.abs()
    else:
        wb = case[5].to(BF).double()
        y64, mag = x @ wb.t() + b, x.abs() @ wb.abs().t() + b.abs()
    err, tol = (y - y64).abs(), 2.0 ** -8 * y64.abs() + K * 2.0 ** -23 * mag
    print(f"max err / bound = {(err / tol.clamp_min(1e-300)).max().item():.3f}")
    return bool((err <= tol).all())


@pytest.mark.gpu
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("N,K", [(128, 128), (256, 1024)])
def test_matches_fp64_reference(gpu, M, N, K):
    with_bias = (M + N // 128) % 2 == 0
    case = int4_case("real", N, K)
    assert within_int4_bound(_run(case, M, with_bias, gpu), case, M, K, with_bias)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [5, 32])
def test_swiglu_epilogue_bit_equal(gpu, M):
    """Same kernel, same accumulation order: the fused epilogue is ops.swiglu_interleaved of the
    plain output (gate and up rounded to bf16, then silu(gate) * up rounded once)."""
    case = int4_case("real", 256, 1024)
    plain = _run(case, M, False, gpu).to(BF).to(gpu)
    assert torch.equal(_run(case, M, False, gpu, swiglu=True),
                       ops.swiglu_interleaved(plain).double().cpu())


@pytest.mark.gpu
@pytest.mark.parametrize("kind,N,K", [("probe", 160, 256), ("real", 256, 1024)])
def test_dequantiser_equals_reference(gpu, kind, N, K):
    wq, scale, zero = (t.to(gpu) for t in int4_case(kind, N, K)[:3])
    out = torch.full((N, K), float("nan"), dtype=BF, device=gpu)
    ops.native().linear_int4(out, None, wq, scale, zero)
    assert torch.equal(out.cpu(), dequant_int4(wq.cpu(), scale.cpu(), zero.cpu()))


@pytest.mark.gpu
@pytest.mark.parametrize("lens", [(2,), (12, 8), (100, 50)])
def test_stage_gpu_matches_cpu(gpu, monkeypatch, lens):
    """2, 20 and 150 rows: all 8 projections run ops.linear_int4 -- kernels on the GPU, the oracle
    on the CPU; tests/test_fp8_block_dense_gpu.py::test_stage_gpu_matches_cpu's tolerance."""
    prompts = [[(7 * i + 3 * j) % 1000 for j in range(n)] for i, n in enumerate(lens)]
    cpu = CausalLMStage(SPEC, 0, 2).init_random(3)
    g = CausalLMStage(SPEC, 0, 2, device=gpu).init_random(3)
    g.load_state_dict({k: v.to(gpu) for k, v in cpu.state_dict().items()})
    cpu.quantize("int4")
    g.quantize("int4")
    g.block.set_fused_swiglu(True)
    lins = [m for m in g.block.modules() if isinstance(m, Linear)]
    assert len(lins) == 8 and all(m.is_int4 for m in lins)
    x = _stage_logits(cpu, prompts)
    rows, real = [], ops.linear_int4
    monkeypatch.setattr(ops, "linear_int4",
                        lambda *a, **kw: (rows.append(a[0].shape[0]), real(*a, **kw))[1])
    y = _stage_logits(g, prompts)
    assert rows == [sum(lens)] * 8, rows             # QKV, O, gate|up, down x 2 layers
    err = (x - y).abs().max().item()
    assert err < 0.03 * max(1.0, x.abs().max().item()), err


@pytest.mark.gpu
def test_engine_graph_decode_equals_eager(gpu):
    """Prefill chunks of 37 and 130 rows (dequantise path), decode steps of 4 rows (streaming
    kernel), eagerly and captured into the bucket's hipGraph: token for token the same."""
    def engine(graphs):
        cfg = EngineConfig(model="q3", pp=1, seed=5, quantize="int4",
                           cache=CacheConfig(num_blocks=256, block_size=64, max_chunk=256),
                           serve=ServeConfig(max_batch_size=8, max_num_batched_tokens=512,
                                             max_seq_len=1024, use_graphs=graphs,
                                             graph_batch_sizes=[1, 2, 4, 8]))
        return LLMEngine(SPEC, device="cuda:0", cfg=cfg)
    prompts = [list(range(3, 40)), [7, 8, 9], list(range(200, 330)), [11]]
    p = SamplingParams(max_tokens=10, ignore_eos=True)
    eng = engine(False)
    lins = [m for m in eng.executors[0].stage.block.modules() if isinstance(m, Linear)]
    assert lins and all(m.is_int4 for m in lins)
    a = [s.output for s in eng.generate(prompts, p)]
    b = [s.output for s in engine(True).generate(prompts, p)]
    assert all(len(o) == 10 for o in a) and a == b
