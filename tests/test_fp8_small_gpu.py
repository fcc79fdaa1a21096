"""The fp8 weight-streaming MFMA kernel for 3-32 bf16 rows (gemm_fp8_small.hip) on the GPU: its
operand layout bit for bit, the fp32 oracle with guarded outputs, determinism, the SwiGLU epilogue
against the unfused order, the host checks, and the path end to end (Linear, stage, engine with
hipGraph decode) behind KernelPolicy.fp8_small_m."""
import pytest
import torch

from distributed_llm_inference import ops
from distributed_llm_inference.config import CacheConfig, KernelPolicy, ModelSpec, ServeConfig
from distributed_llm_inference.models import CausalLMStage
from distributed_llm_inference.models.common import Linear
from distributed_llm_inference.runtime.engine import EngineConfig, LLMEngine
from distributed_llm_inference.runtime.sequence import SamplingParams

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
FP8 = torch.float8_e4m3fn
G = 4096          # guard elements on each side of a guarded output
SENT = -12345.0

# tests/test_fp4_small_gpu.py's SPEC
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
    """Random weights whose row magnitudes span 2^lo .. 2^hi, so the per-row scales differ by
    orders of magnitude and a scale read from the wrong row shows."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, k, generator=g)
    ex = torch.randint(lo, hi + 1, (n, 1), generator=g).float()
    return w * torch.exp2(ex)


def _spy(monkeypatch, name):
    calls, real = [], getattr(ops, name)

    def wrapped(*a, **kw):
        src = a[0].parts if isinstance(a[0], ops.SplitKPartials) else a[0]
        calls.append(src.shape[0])
        return real(*a, **kw)
    monkeypatch.setattr(ops, name, wrapped)
    return calls


# ------------------------------------------------------------------------------------- layout
_LAYOUT = {}


def _layout_case(N, K):
    """(W8 [N, K] e4m3fn, row scales [N], x [32, K] fp64, exact product [32, N] fp64), built once
    per (N, K)."""
    if (N, K) not in _LAYOUT:
        g = torch.Generator().manual_seed(1000 * N + K)
        byte = torch.randint(0, 256, (N, K), generator=g, dtype=torch.uint8)
        # magnitude codes 0x00 .. 0x48 = 0 .. 4.0 (so no NaN code 0x7f / 0xff), any sign
        byte = (byte & 0x80) | ((byte & 0x7F) % 0x49)
        w8 = byte.view(FP8)
        wd = w8.float().double()
        assert bool(torch.isfinite(wd).all()) and wd.abs().max() == 4.0
        assert (byte & 0x7F).unique().numel() == 0x49       # every code up to 4.0 occurs
        n = torch.arange(N)
        scale = torch.exp2(((2 * n + n // 16) % 3 - 1).float())    # 0.5, 1, 2, row to row
        # integers in [-4, 4], no symmetry in row or k
        x = torch.randint(-4, 5, (32, K), generator=g).double()
        x[:, 0] = torch.arange(32).double() % 9 - 4
        raw = x @ wd.t()
        # every product is a multiple of 2^-9 (e4m3's smallest subnormal times an integer): a sum
        # below 2^15 in magnitude has at most 24 significant bits
        assert raw.abs().max() < 2 ** 15
        assert (x.abs() @ wd.abs().t()).max() < 2 ** 15     # ... and so has every partial sum
        _LAYOUT[(N, K)] = (w8, scale, x, raw * scale.double())
    return _LAYOUT[(N, K)]


@pytest.mark.parametrize("M", [3, 16, 17, 32])
@pytest.mark.parametrize("N", [16, 48])
@pytest.mark.parametrize("K", [128, 384, 1024])
def test_small_gemm_fp8_layout_bit_exact(gpu, K, N, M):
    """Every product is a multiple of 2^-9 (|w| <= 4 in e4m3, x an integer in [-4, 4]) and every
    partial sum is below 2^15, so each is exact in fp32 in any order, and the power-of-two row
    scale keeps it exact: the result is the exact product rounded once to bf16, whatever the lane
    maps -- as long as they are the right ones.  K = 128 leaves all but one K-split wave without
    work, K = 384 splits unevenly; N = 16 / 48 leave the workgroup's second weight tile absent."""
    w8, scale, x, want = _layout_case(N, K)
    y = ops.small_gemm_fp8(x[:M].to(BF).to(gpu), w8.to(gpu), scale.to(gpu))
    assert y.shape == (M, N) and y.dtype == BF
    assert torch.equal(y.cpu(), want[:M].to(BF))


# ------------------------------------------------------------------------------------- oracle
_ORACLE = {}


def _oracle_case(N, K, gpu):
    """(W8, row scales [1, N], dequantised fp32 weight, x [32, K], bias) on the GPU, once per
    (N, K)."""
    if (N, K) not in _ORACLE:
        w8, ws = ops.quantize_weight_fp8(_wide_weight(N, K, N + K))
        assert ws.max() / ws.min() > 100
        wd = w8.float() * ws.reshape(-1, 1)                  # the CPU oracle's weight
        g = torch.Generator().manual_seed(K + 1)
        x = torch.randn(32, K, generator=g).to(BF)
        bias = (torch.randn(N, generator=g) * 0.1).to(BF)
        _ORACLE[(N, K)] = tuple(t.to(gpu) for t in (w8, ws, wd, x, bias))
    return _ORACLE[(N, K)]


@pytest.mark.parametrize("M", [3, 5, 16, 17, 31, 32])
@pytest.mark.parametrize("N,K", [(48, 128), (80, 1152), (32, 8192)])
@pytest.mark.parametrize("with_bias", [False, True])
def test_small_gemm_fp8_against_fp32_oracle(gpu, with_bias, N, K, M):
    """The fp32 product of the bf16 rows and the dequantised weight.  The kernel adds one bf16
    store rounding and its own fp32 summation order, far inside the fp8 GEMV test's tolerance.
    The output sits between guards that must keep their sentinel; x is its own M x K allocation."""
    w8, ws, wd, x32, bias = _oracle_case(N, K, gpu)
    x = torch.empty(M * K, dtype=BF, device=gpu).view(M, K)
    x.copy_(x32[:M])
    b = bias if with_bias else None
    want = x.float() @ wd.t() + (bias.float() if with_bias else 0.0)
    buf = torch.full((G + M * N + G,), SENT, dtype=BF, device=gpu)
    out = buf[G:G + M * N].view(M, N)
    y = ops.small_gemm_fp8(x, w8, ws, b, out=out)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr()
    assert bool((buf[:G] == SENT).all()), "write before the output"
    assert bool((buf[G + M * N:] == SENT).all()), "write after the output"
    _close(y, want, 2e-2, 2e-2, f"small fp8 M={M} N={N} K={K} bias={with_bias}")


def test_small_gemm_fp8_deterministic(gpu):
    M, N, K = 7, 64, 2048
    w8, ws = ops.quantize_weight_fp8(_wide_weight(N, K, 11).to(gpu))
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(12)).to(BF).to(gpu)
    a = ops.small_gemm_fp8(x, w8, ws)
    b = ops.small_gemm_fp8(x, w8, ws)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("M", [3, 16, 17, 32])
def test_small_gemm_fp8_swiglu_equals_unfused(gpu, M):
    """The SwiGLU epilogue scales gate and up by their own rows' scales and rounds each to bf16
    before silu(gate) * up: ops.swiglu_interleaved on the plain product, bit for bit; and the CPU
    branch within the oracle tolerance."""
    I, K = 128, 512
    g = torch.Generator().manual_seed(20 + M)
    w = torch.randn(2 * I, K, generator=g) * 0.05 * torch.exp2(
        torch.randint(-3, 4, (2 * I, 1), generator=g).float())
    w8, ws = ops.quantize_weight_fp8(ops.swiglu_interleave(w.to(BF)))
    x = torch.randn(M, K, generator=g).to(BF)
    wg, sg, xg = w8.to(gpu), ws.to(gpu), x.to(gpu)
    fused = ops.small_gemm_fp8(xg, wg, sg, swiglu=True)
    assert fused.shape == (M, I)
    unfused = ops.swiglu_interleaved(ops.small_gemm_fp8(xg, wg, sg))
    assert torch.equal(fused, unfused)
    _close(fused, ops.small_gemm_fp8(x, w8, ws, swiglu=True), 2e-2, 2e-2, "swiglu vs cpu")


def test_small_gemm_fp8_rejects_bad_shapes(gpu):
    def case(M, N, K, wk=None, ns=None, bias=False, swiglu=False, wdtype=FP8, xdtype=BF):
        x = torch.zeros(M, K, device=gpu, dtype=xdtype)
        w8 = torch.zeros(N, wk or K, dtype=torch.uint8, device=gpu).view(wdtype)
        ws = torch.ones(ns or N, dtype=torch.float32, device=gpu)
        b = torch.zeros(N, device=gpu, dtype=BF) if bias else None
        return ops.small_gemm_fp8(x, w8, ws, b, swiglu=swiglu)

    assert case(3, 32, 128).shape == (3, 32)                # the smallest good one
    assert case(3, 64, 128, swiglu=True).shape == (3, 32)
    for kw in (dict(M=2, N=32, K=128), dict(M=33, N=32, K=128), dict(M=3, N=32, K=96),
               dict(M=3, N=24, K=128), dict(M=3, N=48, K=128, swiglu=True),
               dict(M=3, N=64, K=128, swiglu=True, bias=True),
               dict(M=3, N=32, K=256, wk=128), dict(M=3, N=32, K=128, ns=16),
               dict(M=3, N=32, K=128, wdtype=torch.uint8),
               dict(M=3, N=32, K=128, xdtype=torch.float16)):
        with pytest.raises(RuntimeError):
            case(**kw)
    x = torch.zeros(3, 128, device=gpu, dtype=BF)
    w8 = torch.zeros(32, 256, dtype=torch.uint8, device=gpu).view(FP8)
    with pytest.raises(RuntimeError):                       # a strided weight view
        ops.small_gemm_fp8(x, w8[:, :128], torch.ones(32, device=gpu))


# ------------------------------------------------------------------------------------- dispatch
def test_linear_dispatch_gpu(gpu, monkeypatch):
    K = N = 1024
    lin = Linear(K, N, bias=True, device=gpu)
    lin.weight.data.copy_(_wide_weight(N, K, 9).to(BF))
    lin.bias.data.copy_((torch.randn(N, generator=torch.Generator().manual_seed(8)) * 0.1).to(BF))
    lin.quantize_fp8()
    cpu = Linear(K, N, bias=True)
    cpu.weight_fp8, cpu.weight_scale = lin.weight_fp8.cpu(), lin.weight_scale.cpu()
    cpu.bias.data.copy_(lin.bias.data.cpu())
    g = torch.Generator().manual_seed(13)
    x = torch.randn(17, K, generator=g).to(BF)
    xg = x.to(gpu)
    off17 = lin(xg)
    with ops.kernel_policy(fp8_small_m=16):                 # the CPU branch: same policy, same op
        want = {m: cpu(x[:m].contiguous()) for m in (3, 16)}
    small = _spy(monkeypatch, "small_gemm_fp8")
    quant = _spy(monkeypatch, "quant_rowwise")
    gemv = _spy(monkeypatch, "skinny_gemm_fp8")
    with ops.kernel_policy(fp8_small_m=16):
        for m in (3, 16):
            y = lin(xg[:m].contiguous())
            assert small[-1] == m and quant == [] and gemv == []
            _close(y, want[m], 2e-2, 2e-2, f"Linear rows={m}")
            yd = lin(xg[:m].contiguous(), defer_reduce=True)
            assert isinstance(yd, torch.Tensor) and torch.equal(yd, y)
        n_small = len(small)
        lin(xg[:2].contiguous())
        assert gemv == [2] and len(small) == n_small and quant == []
        on17 = lin(xg)
        assert len(small) == n_small and quant == [17]      # 17 rows: the flag-off path
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


def test_fp8_small_stage_gpu_matches_cpu(gpu, monkeypatch):
    """12 prompt rows: every projection of every layer takes the new kernel on the GPU (gate|up
    with its SwiGLU epilogue: the GPU stage's rows are interleaved as the engine leaves them) and
    its CPU arithmetic on the CPU stage (same policy, same branch); the row quantiser never runs."""
    prompts = [[1, 2, 3, 4, 5], [6, 7, 8, 9], [10, 11, 12]]
    cpu = CausalLMStage(SPEC, 0, 4).init_random(3)
    g = CausalLMStage(SPEC, 0, 4, device=gpu).init_random(3)
    g.load_state_dict({k: v.to(gpu) for k, v in cpu.state_dict().items()})
    cpu.quantize("fp8")
    g.quantize("fp8")
    g.block.set_fused_swiglu(True)
    assert all(layer.mlp.fused_swiglu for layer in g.block.layers)
    with ops.kernel_policy(fp8_small_m=16):
        x = _stage_logits(cpu, prompts)
        small = _spy(monkeypatch, "small_gemm_fp8")
        quant = _spy(monkeypatch, "quant_rowwise")
        y = _stage_logits(g, prompts)
    assert len(small) == 4 * 4 and set(small) == {12}, small    # QKV, O, gate|up, down x 4 layers
    assert quant == []
    err = (x - y).abs().max().item()
    assert err < 0.03 * max(1.0, x.abs().max().item()), err


def _engine(graphs, max_batch=8, buckets=(1, 2, 4, 8)):
    cfg = EngineConfig(model="t", pp=1, seed=5, quantize="fp8",
                       kernels=KernelPolicy().with_overrides("fp8_small_m=8"),
                       cache=CacheConfig(num_blocks=256, block_size=64, max_chunk=256),
                       serve=ServeConfig(max_batch_size=max_batch, max_num_batched_tokens=512,
                                         max_seq_len=1024, use_graphs=graphs,
                                         graph_batch_sizes=list(buckets)))
    return LLMEngine(SPEC, device="cuda:0", cfg=cfg)


PROMPTS = [list(range(3, 40)), [7, 8, 9], list(range(200, 330)), [11]]


def test_fp8_small_engine_graph_decode_equals_eager(gpu, monkeypatch):
    """4 sequences in flight: every decode step's 4 rows run on the new kernel, eagerly and
    captured into the bucket's hipGraph; the 171-row prefill keeps the parent's fp8 route.  A
    batch of 2 still decodes on the GEMV and a batch of 12 is past fp8_small_m=8."""
    small = _spy(monkeypatch, "small_gemm_fp8")
    gemv = _spy(monkeypatch, "skinny_gemm_fp8")
    quant = _spy(monkeypatch, "quant_rowwise")
    p = SamplingParams(max_tokens=10, ignore_eos=True)
    eng = _engine(graphs=False)
    lins = [m for m in eng.executors[0].stage.block.modules() if isinstance(m, Linear)]
    assert lins and all(m.is_fp8 for m in lins)
    assert ops.policy().fp8_small_m == 8
    del small[:], gemv[:]                               # start-up warm-ups do not count
    a = [s.output for s in eng.generate(PROMPTS, p)]
    # 9 decode steps follow the prefill's first token: 4 layers x (QKV, O, gate|up, down)
    assert small.count(4) >= 9 * 4 * 4, small
    del small[:], gemv[:]
    two = [s.output for s in eng.generate(PROMPTS[:2], p)]
    assert all(len(o) == 10 for o in two)
    # 2 rows: the fp8 GEMV, as before (O, gate|up, down; QKV is the fused RoPE GEMV); the new
    # kernel sees a prefill at the most
    assert gemv.count(2) >= 9 * 4 * 3, gemv
    assert len(small) <= 2 * 4 * 4, small
    b = [s.output for s in _engine(graphs=True).generate(PROMPTS, p)]
    assert all(len(o) == 10 for o in a) and a == b
    eng12 = _engine(graphs=False, max_batch=16, buckets=(1, 2, 4, 8, 16))
    del small[:], quant[:]
    twelve = [s.output for s in eng12.generate([[5 + i, 9] for i in range(12)], p)]
    assert all(len(o) == 10 for o in twelve)
    assert 12 not in small and 12 in quant                  # 12 rows: past the limit, quantised
