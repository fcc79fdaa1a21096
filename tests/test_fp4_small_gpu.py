"""The MXFP4 weight-streaming MFMA kernel for 3-32 bf16 rows (gemm_fp4_small.hip) on the GPU: its
operand layout bit for bit, the fp32 oracle of the format with guarded outputs, determinism, the
SwiGLU epilogue against the unfused order, the host checks, and the path end to end (Linear,
stage, engine with hipGraph decode) behind KernelPolicy.fp4_small_m."""
import pytest
import torch

from distributed_llm_inference import ops
from distributed_llm_inference.config import CacheConfig, KernelPolicy, ModelSpec, ServeConfig
from distributed_llm_inference.models import CausalLMStage
from distributed_llm_inference.models.common import Linear
from distributed_llm_inference.ops import reference as ref
from distributed_llm_inference.runtime.engine import EngineConfig, LLMEngine
from distributed_llm_inference.runtime.sequence import SamplingParams

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
G = 4096          # guard elements on each side of a guarded output
SENT = -12345.0

# tests/test_mxfp4_gpu.py's SPEC
SPEC = ModelSpec(name="t", vocab_size=1000, hidden_size=256, intermediate_size=512, num_layers=4,
                 num_heads=8, num_kv_heads=2, head_dim=32, rope_theta=10000.0,
                 max_position_embeddings=4096)


def _close(a, b, atol, rtol=0.0, msg=""):
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol)
    assert not bad.any(), f"{msg} max err {err.max().item():.4g} at {bad.nonzero()[:5].tolist()}"


def _wide_weight(n, k, seed, lo=-14, hi=-3):
    """Random weights whose per-block magnitudes span 2^lo .. 2^hi (block exponents differ from
    block to block and row to row, so a scale read from the wrong place shows)."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, k // 32, 32, generator=g)
    ex = torch.randint(lo, hi + 1, (n, k // 32, 1), generator=g).float()
    return (w * torch.exp2(ex)).reshape(n, k)


def _spy(monkeypatch, name):
    calls, real = [], getattr(ops, name)

    def wrapped(*a, **kw):
        calls.append(a[0].shape[0])
        return real(*a, **kw)
    monkeypatch.setattr(ops, name, wrapped)
    return calls


# ------------------------------------------------------------------------------------- layout
_LAYOUT = {}


def _layout_case(N, K):
    """(packed, scales, x [32, K] fp64, exact product [32, N] fp64), built once per (N, K)."""
    if (N, K) not in _LAYOUT:
        g = torch.Generator().manual_seed(1000 * N + K)
        packed = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.uint8)
        codes = torch.cat([packed & 15, packed >> 4]).unique()
        assert codes.numel() == 16                          # every e2m1 code occurs
        n = torch.arange(N).reshape(N, 1)
        blk = torch.arange(K // 32).reshape(1, K // 32)
        scales = (126 + (2 * n + blk) % 3).to(torch.uint8)     # differs block to block, row to row
        # integers in [-4, 4], no symmetry in row or k
        x = torch.randint(-4, 5, (32, K), generator=g).double()
        x[:, 0] = torch.arange(32).double() % 9 - 4
        want = x @ ref.dequantize_mxfp4(packed, scales).double().t()
        assert want.abs().max() < 2 ** 16
        _LAYOUT[(N, K)] = (packed, scales, x, want)
    return _LAYOUT[(N, K)]


@pytest.mark.parametrize("M", [3, 16, 17, 32])
@pytest.mark.parametrize("N", [16, 48])
@pytest.mark.parametrize("K", [128, 384, 1024])
def test_small_gemm_fp4_layout_bit_exact(gpu, K, N, M):
    """Every product is a multiple of 2^-2 (e2m1 is a multiple of 1/2, the block scales are 1/2,
    1 and 2, x is an integer) and |sum| < 2^16, so every partial sum is exact in fp32 in any
    order: the result is the exact product rounded once to bf16, whatever the lane maps -- as
    long as they are the right ones.  K = 128 leaves all but one K-split wave without work,
    K = 384 splits unevenly; N = 16 / 48 leave the workgroup's second weight tile absent."""
    packed, scales, x, want = _layout_case(N, K)
    y = ops.small_gemm_fp4(x[:M].to(BF).to(gpu), packed.to(gpu), scales.to(gpu))
    assert y.shape == (M, N) and y.dtype == BF
    assert torch.equal(y.cpu(), want[:M].to(BF))


# ------------------------------------------------------------------------------------- oracle
_ORACLE = {}


def _oracle_case(N, K, gpu):
    """(packed, scales, dequantised fp32 weight, x [32, K], bias) on the GPU, once per (N, K)."""
    if (N, K) not in _ORACLE:
        packed, scales = ops.quantize_weight_mxfp4(_wide_weight(N, K, N + K))
        wd = ref.dequantize_mxfp4(packed, scales).float()      # the CPU oracle's weight
        g = torch.Generator().manual_seed(K + 1)
        x = torch.randn(32, K, generator=g).to(BF)
        bias = (torch.randn(N, generator=g) * 0.1).to(BF)
        _ORACLE[(N, K)] = tuple(t.to(gpu) for t in (packed, scales, wd, x, bias))
    return _ORACLE[(N, K)]


@pytest.mark.parametrize("M", [3, 5, 16, 17, 31, 32])
@pytest.mark.parametrize("N,K", [(48, 128), (80, 1152), (32, 8192)])
@pytest.mark.parametrize("with_bias", [False, True])
def test_small_gemm_fp4_against_fp32_oracle(gpu, with_bias, N, K, M):
    """The fp32 product of the bf16 rows and the dequantised weight.  The kernel adds one bf16
    store rounding and its own fp32 summation order, far inside the GEMV test's tolerance.  The
    output sits between guards that must keep their sentinel; x is its own M x K allocation."""
    packed, scales, wd, x32, bias = _oracle_case(N, K, gpu)
    x = torch.empty(M * K, dtype=BF, device=gpu).view(M, K)
    x.copy_(x32[:M])
    b = bias if with_bias else None
    want = x.float() @ wd.t() + (bias.float() if with_bias else 0.0)
    buf = torch.full((G + M * N + G,), SENT, dtype=BF, device=gpu)
    out = buf[G:G + M * N].view(M, N)
    y = ops.small_gemm_fp4(x, packed, scales, b, out=out)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr()
    assert bool((buf[:G] == SENT).all()), "write before the output"
    assert bool((buf[G + M * N:] == SENT).all()), "write after the output"
    _close(y, want, 2e-2, 2e-2, f"small fp4 M={M} N={N} K={K} bias={with_bias}")


def test_small_gemm_fp4_deterministic(gpu):
    M, N, K = 7, 64, 2048
    packed, scales = ops.quantize_weight_mxfp4(_wide_weight(N, K, 11).to(gpu))
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(12)).to(BF).to(gpu)
    a = ops.small_gemm_fp4(x, packed, scales)
    b = ops.small_gemm_fp4(x, packed, scales)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("M", [4, 20])
def test_small_gemm_fp4_swiglu_equals_unfused(gpu, M):
    """The SwiGLU epilogue rounds gate and up to bf16 before silu(gate) * up: the bits of
    ops.swiglu_interleaved on the plain product; and the CPU branch within the oracle tolerance."""
    I, K = 128, 512
    g = torch.Generator().manual_seed(20 + M)
    w = ops.swiglu_interleave((torch.randn(2 * I, K, generator=g) * 0.05).to(BF))
    packed, scales = ops.quantize_weight_mxfp4(w)
    x = torch.randn(M, K, generator=g).to(BF)
    pg, sg, xg = packed.to(gpu), scales.to(gpu), x.to(gpu)
    fused = ops.small_gemm_fp4(xg, pg, sg, swiglu=True)
    assert fused.shape == (M, I)
    unfused = ops.swiglu_interleaved(ops.small_gemm_fp4(xg, pg, sg))
    assert torch.equal(fused.view(torch.int16), unfused.view(torch.int16))
    _close(fused, ops.small_gemm_fp4(x, packed, scales, swiglu=True), 2e-2, 2e-2, "swiglu vs cpu")


def test_small_gemm_fp4_rejects_bad_shapes(gpu):
    def case(M, N, K, sk=None, bias=False, swiglu=False):
        x = torch.zeros(M, K, device=gpu, dtype=BF)
        packed = torch.zeros(N, K // 2, dtype=torch.uint8, device=gpu)
        scales = torch.full((N, (sk or K) // 32), 127, dtype=torch.uint8, device=gpu)
        b = torch.zeros(N, device=gpu, dtype=BF) if bias else None
        return ops.small_gemm_fp4(x, packed, scales, b, swiglu=swiglu)

    assert case(3, 32, 128).shape == (3, 32)                # the smallest good one
    assert case(3, 64, 128, swiglu=True).shape == (3, 32)
    for kw in (dict(M=2, N=32, K=128), dict(M=33, N=32, K=128), dict(M=3, N=32, K=96),
               dict(M=3, N=24, K=128), dict(M=3, N=48, K=128, swiglu=True),
               dict(M=3, N=64, K=128, swiglu=True, bias=True),
               dict(M=3, N=32, K=256, sk=128)):
        with pytest.raises(RuntimeError):
            case(**kw)


# ------------------------------------------------------------------------------------- dispatch
def test_linear_dispatch_gpu(gpu, monkeypatch):
    K = N = 1024
    lin = Linear(K, N, device=gpu)
    lin.weight.data.copy_(_wide_weight(N, K, 9).to(BF))
    lin.quantize_mxfp4()
    g = torch.Generator().manual_seed(13)
    x = torch.randn(17, K, generator=g).to(BF).to(gpu)
    off17 = lin(x)
    small = _spy(monkeypatch, "small_gemm_fp4")
    deq = _spy(monkeypatch, "dequantize_mxfp4")
    gemv = _spy(monkeypatch, "skinny_gemm_fp4")
    wd = ref.dequantize_mxfp4(lin.weight_fp4.cpu(), lin.weight_block_scale.cpu()).float().to(gpu)
    with ops.kernel_policy(fp4_small_m=16):
        for m in (3, 16):
            y = lin(x[:m].contiguous())
            assert small[-1] == m and deq == [] and gemv == []
            _close(y, x[:m].float() @ wd.t(), 2e-2, 2e-2, f"Linear rows={m}")
            yd = lin(x[:m].contiguous(), defer_reduce=True)
            assert isinstance(yd, torch.Tensor) and torch.equal(yd, y)
        n_small = len(small)
        lin(x[:2].contiguous())
        assert gemv == [2] and len(small) == n_small and deq == []
        on17 = lin(x)
        assert len(small) == n_small and len(deq) == 1      # 17 rows: the flag-off path
        assert torch.equal(on17, off17)


def _stage_logits(stage, prompts):
    pool = stage.make_pool(128, block_size=64)
    sids = list(range(len(prompts)))
    for s, p in zip(sids, prompts):
        pool.manager.append(s, len(p))
    meta = pool.build_metadata(sids, [len(p) for p in prompts])
    meta.logits_rows = (torch.cumsum(torch.tensor([len(p) for p in prompts]), 0) - 1).to(stage.device)
    ids = torch.tensor([t for p in prompts for t in p], dtype=torch.int32, device=stage.device)
    return stage(ids, meta, pool).float().cpu()


def test_fp4_small_stage_gpu_matches_cpu(gpu, monkeypatch):
    """12 prompt rows: every projection of every layer takes the new kernel on the GPU and its
    CPU arithmetic on the CPU stage (same policy, same branch)."""
    prompts = [[1, 2, 3, 4, 5], [6, 7, 8, 9], [10, 11, 12]]
    cpu = CausalLMStage(SPEC, 0, 4).init_random(3)
    g = CausalLMStage(SPEC, 0, 4, device=gpu).init_random(3)
    g.load_state_dict({k: v.to(gpu) for k, v in cpu.state_dict().items()})
    cpu.quantize("mxfp4")
    g.quantize("mxfp4")
    with ops.kernel_policy(fp4_small_m=16):
        x = _stage_logits(cpu, prompts)
        small = _spy(monkeypatch, "small_gemm_fp4")
        deq = _spy(monkeypatch, "dequantize_mxfp4")
        y = _stage_logits(g, prompts)
    assert len(small) == 4 * 4 and set(small) == {12}, small    # QKV, O, gate|up, down x 4 layers
    assert deq == []
    err = (x - y).abs().max().item()
    assert err < 0.03 * max(1.0, x.abs().max().item()), err


def _engine(graphs):
    cfg = EngineConfig(model="t", pp=1, seed=5, quantize="mxfp4",
                       kernels=KernelPolicy().with_overrides("fp4_small_m=8"),
                       cache=CacheConfig(num_blocks=256, block_size=64, max_chunk=256),
                       serve=ServeConfig(max_batch_size=8, max_num_batched_tokens=512,
                                         max_seq_len=1024, use_graphs=graphs,
                                         graph_batch_sizes=[1, 2, 4, 8]))
    return LLMEngine(SPEC, device="cuda:0", cfg=cfg)


PROMPTS = [list(range(3, 40)), [7, 8, 9], list(range(200, 330)), [11]]


def test_fp4_small_engine_graph_decode_equals_eager(gpu, monkeypatch):
    """4 sequences in flight: every decode step's 4 rows run on the new kernel, eagerly and
    captured into the bucket's hipGraph (it allocates from the caching allocator only and never
    touches the dequantise scratch); the 171-row prefill keeps the dequantise path."""
    small = _spy(monkeypatch, "small_gemm_fp4")
    deq = _spy(monkeypatch, "dequantize_mxfp4")
    p = SamplingParams(max_tokens=10, ignore_eos=True)
    eng = _engine(graphs=False)
    lins = [m for m in eng.executors[0].stage.block.modules() if isinstance(m, Linear)]
    assert lins and all(m.is_fp4 for m in lins)
    assert ops.policy().fp4_small_m == 8
    del small[:], deq[:]                                # start-up warm-ups do not count
    a = [s.output for s in eng.generate(PROMPTS, p)]
    # 9 decode steps follow the prefill's first token: 4 layers x (QKV, O, gate|up, down)
    assert small.count(4) >= 9 * 4 * 4, small
    assert 0 < len(deq) <= 16 * len(PROMPTS), deq       # the prefill step(s) only
    b = [s.output for s in _engine(graphs=True).generate(PROMPTS, p)]
    assert all(len(o) == 10 for o in a) and a == b
