"""MXFP4 weights on the GPU: the dequantiser and the weight-streaming GEMV (gemv.hip) against the
CPU oracle of the format, the fused epilogues / prologue against their unfused order, and the
mode end to end (Linear, stage, engine)."""
import pytest
import torch

from distributed_llm_inference import ops
from distributed_llm_inference.config import CacheConfig, ModelSpec, ServeConfig
from distributed_llm_inference.models import CausalLMStage
from distributed_llm_inference.models import common
from distributed_llm_inference.models.common import Linear
from distributed_llm_inference.models.llama.modules import LlamaMLP
from distributed_llm_inference.ops import reference as ref
from distributed_llm_inference.runtime.engine import EngineConfig, LLMEngine
from distributed_llm_inference.runtime.sequence import SamplingParams

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
G = 4096          # guard elements on each side of a guarded output
SENT = -12345.0

# tests/test_engine_gpu.py's SPEC
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


@pytest.mark.parametrize("N,K", [(2051, 8192), (7, 96)])
def test_dequantize_matches_cpu_reference(gpu, N, K):
    """Every nibble code under block exponents 2^-20 .. 2^10: pins the nibble order of the
    hardware convert and the scale indexing; also into a larger (scratch-like) buffer."""
    g = torch.Generator().manual_seed(N)
    packed = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.uint8)
    scales = torch.randint(107, 138, (N, K // 32), generator=g, dtype=torch.uint8)
    want = ref.dequantize_mxfp4(packed, scales)
    got = ops.dequantize_mxfp4(packed.to(gpu), scales.to(gpu))
    assert got.dtype == BF and got.shape == (N, K)
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))   # bits, -0 included
    buf = torch.full((N * K + 2 * G,), SENT, dtype=BF, device=gpu)
    got2 = ops.dequantize_mxfp4(packed.to(gpu), scales.to(gpu), out=buf[G:])
    torch.cuda.synchronize()
    assert got2.data_ptr() == buf[G:].data_ptr() and torch.equal(got2, got)
    assert bool((buf[:G] == SENT).all()) and bool((buf[G + N * K:] == SENT).all())


def test_quantiser_on_gpu_equals_cpu(gpu):
    w = _wide_weight(96, 256, 1, -20, 10)
    pc, sc = ops.quantize_weight_mxfp4(w)
    pg, sg = ops.quantize_weight_mxfp4(w.to(gpu))
    assert torch.equal(pg.cpu(), pc) and torch.equal(sg.cpu(), sc)


_ORACLE = {}


def _gemv_case(K, gpu):
    """(packed, scales, dequantised fp32 weight, x [2, K], bias) on the GPU, built once per K."""
    if K not in _ORACLE:
        N = 2051
        w = _wide_weight(N, K, K)
        packed, scales = ops.quantize_weight_mxfp4(w)
        wd = ref.dequantize_mxfp4(packed, scales).float()      # the CPU oracle's weight
        g = torch.Generator().manual_seed(K + 1)
        x = torch.randn(2, K, generator=g).to(BF)
        bias = (torch.randn(N, generator=g) * 0.1).to(BF)
        _ORACLE[K] = tuple(t.to(gpu) for t in (packed, scales, wd, x, bias))
    return _ORACLE[K]


@pytest.mark.parametrize("K", [96, 8192, 10240, 28672])
@pytest.mark.parametrize("M", [1, 2])
def test_skinny_gemm_fp4_against_fp32_oracle(gpu, M, K):
    """K = 96: less than one wave instruction; 8192: exactly one unroll group; 10240: a group
    and a partial one; 28672: a real down-projection K.  N is odd (the last wave has one live
    row).  The output sits between guard rows that must keep their sentinel."""
    packed, scales, wd, x2, bias = _gemv_case(K, gpu)
    N, x = packed.shape[0], x2[:M].contiguous()
    want = x.float() @ wd.t() + bias.float()
    buf = torch.full((G + M * N + G,), SENT, dtype=BF, device=gpu)
    out = buf[G:G + M * N].view(M, N)
    y = ops.skinny_gemm_fp4(x, packed, scales, bias, out=out)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr()
    assert bool((buf[:G] == SENT).all()), "write before the output"
    assert bool((buf[G + M * N:] == SENT).all()), "write after the output"
    _close(y, want, 2e-2, 2e-2, f"skinny fp4 M={M} K={K}")
    _close(ops.skinny_gemm_fp4(x, packed, scales), x.float() @ wd.t(), 2e-2, 2e-2, "no bias")


def test_skinny_gemm_fp4_rejects_bad_shapes(gpu):
    packed = torch.zeros(64, 48, dtype=torch.uint8, device=gpu)
    scales = torch.full((64, 3), 127, dtype=torch.uint8, device=gpu)
    with pytest.raises(RuntimeError):    # M > 2
        ops.skinny_gemm_fp4(torch.zeros(3, 96, device=gpu, dtype=BF), packed, scales)
    with pytest.raises(RuntimeError):    # K does not match the packed weight
        ops.skinny_gemm_fp4(torch.zeros(1, 64, device=gpu, dtype=BF), packed, scales)
    with pytest.raises(RuntimeError):    # scales of another K
        ops.skinny_gemm_fp4(torch.zeros(1, 96, device=gpu, dtype=BF), packed, scales[:, :2].contiguous())
    with pytest.raises(RuntimeError):    # swiglu needs 32 | N
        ops.skinny_gemm_fp4(torch.zeros(1, 96, device=gpu, dtype=BF), packed[:48], scales[:48], swiglu=True)


@pytest.mark.parametrize("M", [1, 2])
def test_skinny_gemm_fp4_swiglu(gpu, M):
    torch.manual_seed(7 * M)
    I, K = 1024, 4096
    w = torch.randn(2 * I, K, device=gpu) * 0.02
    wi = ops.swiglu_interleave(w.to(BF))
    packed, scales = ops.quantize_weight_mxfp4(wi)
    wd = ref.dequantize_mxfp4(packed.cpu(), scales.cpu()).float().to(gpu)
    x = torch.randn(M, K, device=gpu, dtype=BF)
    y = ops.skinny_gemm_fp4(x, packed, scales, swiglu=True)
    gu = x.float() @ wd.t()
    want = ops.swiglu_interleaved(gu.to(BF).cpu()).float()
    assert y.shape == (M, I)
    _close(y.float().cpu(), want, 2e-2, 2e-2, "skinny fp4 swiglu")


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("swiglu", [False, True])
@pytest.mark.parametrize("resid", [False, True])
def test_skinny_gemm_fp4_fused_norm_bit_identical(gpu, M, swiglu, resid):
    torch.manual_seed(M * 31 + swiglu * 7 + resid)
    N, K = (2048 if swiglu else 1536), 8192
    x = torch.randn(M, K, device=gpu, dtype=BF)
    res = torch.randn(M, K, device=gpu, dtype=BF) if resid else None
    res0 = res.clone() if resid else None
    nw = (1 + 0.1 * torch.randn(K, device=gpu)).to(BF)
    w = (torch.randn(N, K, device=gpu) * 0.02).to(BF)
    packed, scales = ops.quantize_weight_mxfp4(w)
    f = lambda xx, **kw: ops.skinny_gemm_fp4(xx, packed, scales, swiglu=swiglu, **kw)  # noqa: E731
    r_sep = res.clone() if resid else None
    normed, _ = ops.rms_norm(x, nw, 1e-5, residual=r_sep)      # r_sep <- x + res in place
    want = f(normed)
    r_out = torch.empty_like(x) if resid else None
    got = f(x, norm=ops.RowNorm(nw, 1e-5, res, r_out))
    torch.cuda.synchronize()
    assert torch.equal(got, want), (got.float() - want.float()).abs().max().item()
    if resid:
        assert torch.equal(r_out, r_sep)
        assert torch.equal(res, res0)   # res_in untouched (not aliased)


@pytest.mark.parametrize("kv_fp8", [False, True])
@pytest.mark.parametrize("M", [1, 2])
def test_skinny_gemm_fp4_qkv_rope_matches_gemv_then_rope_cache(gpu, kv_fp8, M):
    torch.manual_seed(11 * M + kv_fp8)
    nh, nkv, D, bs, K, nblk = 8, 2, 128, 64, 2048, 4
    N = (nh + 2 * nkv) * D
    x = torch.randn(M, K, device=gpu, dtype=BF)
    w = (torch.randn(N, K, device=gpu) * 0.02).to(BF)
    packed, scales = ops.quantize_weight_mxfp4(w)
    cs = ref.build_cos_sin(D, 4096, 500000.0, None, device=gpu)
    pos = torch.tensor([37, 4000][:M], device=gpu, dtype=torch.int32)
    slots = torch.tensor([5, -1][:M] if M == 2 else [70], device=gpu, dtype=torch.int64)
    kdt = torch.float8_e4m3fn if kv_fp8 else BF
    nw = (1 + 0.1 * torch.randn(K, device=gpu)).to(BF)
    for norm in (None, ops.RowNorm(nw, 1e-5)):
        caches = []
        for _ in range(2):
            kc = torch.zeros(nblk, nkv, bs, D, device=gpu).to(kdt)
            vc = torch.zeros(nblk, nkv, bs // 8, D, 8, device=gpu).to(kdt)
            caches.append((kc, vc))
        xin = x if norm is None else norm.apply(x)
        qkv = ops.skinny_gemm_fp4(xin, packed, scales)
        q_ref, _ = ops.rope_cache(qkv, pos, slots, cs, nh, nkv, D, *caches[0], k_scale=0.5,
                                  v_scale=0.25)
        q = ops.skinny_gemm_qkv_rope(x, packed, None, None, pos, slots, cs, nh, nkv, D, *caches[1],
                                     k_scale=0.5, v_scale=0.25, norm=norm, block_scale=scales)
        torch.cuda.synchronize()
        assert torch.equal(q, q_ref)
        assert bool(caches[1][0].view(torch.uint8).any())      # something was written
        for a, b in zip(caches[0], caches[1]):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    with pytest.raises(ValueError):   # the format is named, never inferred
        ops.skinny_gemm_qkv_rope(x, packed, torch.ones(N, device=gpu), None, pos, slots, cs, nh,
                                 nkv, D, *caches[1], block_scale=scales)


def _same(a, b):
    if isinstance(a, ops.SplitKPartials) or isinstance(b, ops.SplitKPartials):
        return (isinstance(a, ops.SplitKPartials) and isinstance(b, ops.SplitKPartials)
                and torch.equal(a.parts, b.parts))
    return torch.equal(a, b)


def test_large_m_path_is_the_bf16_path(gpu):
    """Beyond the GEMV's rows an MXFP4 Linear dequantises and runs the unchanged bf16 path: the
    same bits as a bf16 Linear holding the dequantised weight -- hipBLASLt at M = 4, the tile GEMM
    (its un-reduced split-K partials included) at M = 384 -- and the same for LlamaMLP with the
    SwiGLU epilogue."""
    torch.manual_seed(3)
    K, N = 1024, 1024
    a = Linear(K, N, device=gpu)
    a.weight.data.copy_(_wide_weight(N, K, 9).to(BF))
    b = Linear(K, N, device=gpu)
    a.quantize_mxfp4()
    b.weight.data.copy_(ref.dequantize_mxfp4(a.weight_fp4.cpu(), a.weight_block_scale.cpu()))
    took_tile = False
    for M in (4, 384):
        x = torch.randn(M, K, device=gpu, dtype=BF)
        assert a.tile_splits(x) == b.tile_splits(x)
        for defer in (False, True):
            ya, yb = a(x, defer_reduce=defer), b(x, defer_reduce=defer)
            took_tile |= isinstance(ya, ops.SplitKPartials)
            assert _same(ya, yb), (M, defer)
    assert took_tile          # M = 384 went to the tile GEMM and returned its partials
    spec = SPEC.replace(hidden_size=512, intermediate_size=1024)
    ma, mb = LlamaMLP(spec, device=gpu), LlamaMLP(spec, device=gpu)
    for lin, seed in ((ma.gate_up_proj, 1), (ma.down_proj, 2)):
        lin.weight.data.copy_((_wide_weight(lin.out_features, lin.in_features, seed, -8, -4)).to(BF))
        lin.quantize_mxfp4()
    ma.set_fused_swiglu(True)
    assert ma.fused_swiglu
    mb.gate_up_proj.weight.data.copy_(ma.gate_up_proj.dense_weight())
    mb.down_proj.weight.data.copy_(ma.down_proj.dense_weight())
    mb.fused_swiglu = True
    for M in (4, 384):
        x = torch.randn(M, 512, device=gpu, dtype=BF)
        for defer in (False, True):
            assert _same(ma(x, defer_reduce=defer), mb(x, defer_reduce=defer)), (M, defer)


def _stage_logits(stage, prompts):
    pool = stage.make_pool(128, block_size=64)
    sids = list(range(len(prompts)))
    for s, p in zip(sids, prompts):
        pool.manager.append(s, len(p))
    meta = pool.build_metadata(sids, [len(p) for p in prompts])
    meta.logits_rows = (torch.cumsum(torch.tensor([len(p) for p in prompts]), 0) - 1).to(stage.device)
    ids = torch.tensor([t for p in prompts for t in p], dtype=torch.int32, device=stage.device)
    return stage(ids, meta, pool).float().cpu()


def test_mxfp4_stage_gpu_matches_cpu(gpu):
    prompts = [list(range(1, 70)), [5, 6, 7]]
    cpu = CausalLMStage(SPEC, 0, 4).init_random(3)
    g = CausalLMStage(SPEC, 0, 4, device=gpu).init_random(3)
    g.load_state_dict({k: v.to(gpu) for k, v in cpu.state_dict().items()})
    cpu.quantize("mxfp4")
    g.quantize("mxfp4")
    for lc, lg in zip(cpu.block.layers, g.block.layers):      # identical MXFP4 weights
        assert torch.equal(lc.mlp.down_proj.weight_fp4, lg.mlp.down_proj.weight_fp4.cpu())
        assert torch.equal(lc.self_attn.qkv_proj.weight_block_scale,
                           lg.self_attn.qkv_proj.weight_block_scale.cpu())
    x, y = _stage_logits(cpu, prompts), _stage_logits(g, prompts)
    err = (x - y).abs().max().item()
    assert err < 0.03 * max(1.0, x.abs().max().item()), err


def _engine(graphs):
    cfg = EngineConfig(model="t", pp=1, seed=5, quantize="mxfp4",
                       cache=CacheConfig(num_blocks=256, block_size=64, max_chunk=256),
                       serve=ServeConfig(max_batch_size=8, max_num_batched_tokens=512,
                                         max_seq_len=1024, use_graphs=graphs,
                                         graph_batch_sizes=[1, 2, 4, 8]))
    return LLMEngine(SPEC, device="cuda:0", cfg=cfg)


PROMPTS = [list(range(3, 40)), [7, 8, 9], list(range(200, 330)), [11]]


@pytest.mark.parametrize("nprompts", [2, 4])
def test_mxfp4_engine_graph_decode_equals_eager(gpu, monkeypatch, nprompts):
    """2 prompts: the decode step's 2 rows run on the fp4 GEMVs (fused norms, RoPE epilogue);
    4 prompts: M = 4 takes the dequantise path.  Counted on the eager engine (the graph engine
    also captures the buckets it does not use)."""
    calls = {"gemv": 0, "qkv": 0, "deq": 0}
    real_gemv, real_qkv, real_deq = ops.skinny_gemm_fp4, ops.skinny_gemm_qkv_rope, ops.dequantize_mxfp4

    def spy(name, fn):
        def wrapped(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return wrapped

    monkeypatch.setattr(ops, "skinny_gemm_fp4", spy("gemv", real_gemv))
    monkeypatch.setattr(ops, "skinny_gemm_qkv_rope", spy("qkv", real_qkv))
    monkeypatch.setattr(ops, "dequantize_mxfp4", spy("deq", real_deq))
    p = SamplingParams(max_tokens=10, ignore_eos=True)
    prompts = PROMPTS[:nprompts]
    eng = _engine(graphs=False)
    lins = [m for m in eng.executors[0].stage.block.modules() if isinstance(m, Linear)]
    assert lins and all(m.is_fp4 for m in lins)
    assert all(l.mlp.fused_swiglu for l in eng.executors[0].stage.block.layers)
    calls.update(gemv=0, qkv=0, deq=0)               # start-up warm-ups do not count
    a = [s.output for s in eng.generate(prompts, p)]
    # 16 projections per step; 9 decode steps follow the prefill's first token
    if nprompts == 2:
        # per decode step and layer: QKV (RoPE epilogue), O, gate|up, down on the GEMV
        assert calls["qkv"] >= 9 * 4 and calls["gemv"] >= 9 * 4 * 3, calls
        assert 0 < calls["deq"] <= 16 * nprompts, calls     # the prefill step(s) only
    else:
        assert calls["gemv"] == 0 and calls["qkv"] == 0, calls
        assert calls["deq"] >= 9 * 16 + 16, calls           # prefill + every decode step
    b = [s.output for s in _engine(graphs=True).generate(prompts, p)]
    assert all(len(o) == 10 for o in a) and a == b


def _stage_bytes(stage):
    seen, total = set(), 0
    for t in list(stage.parameters()) + list(stage.buffers()):
        if t.data_ptr() not in seen and t.numel():
            seen.add(t.data_ptr())
            total += t.numel() * t.element_size()
    return total


def test_mxfp4_stage_takes_fewer_bytes_than_fp8(gpu, monkeypatch):
    monkeypatch.setattr(common, "MXFP4_SCRATCH", common._Mxfp4Scratch())   # this stage's alone
    s8 = CausalLMStage(SPEC, 0, 4, device=gpu).init_random(3).quantize_fp8()
    s4 = CausalLMStage(SPEC, 0, 4, device=gpu).init_random(3).quantize_mxfp4()
    scratch = common.MXFP4_SCRATCH.nbytes(gpu)
    largest = max(m.in_features * m.out_features for m in s4.block.modules() if isinstance(m, Linear))
    assert scratch == 2 * largest                 # one buffer, sized to the largest weight
    layers8 = _stage_bytes(s8.block)
    layers4 = _stage_bytes(s4.block)
    assert layers4 + scratch < layers8, (layers4, scratch, layers8)
    assert _stage_bytes(s4) + scratch < _stage_bytes(s8)
    n = sum(m.in_features * m.out_features for m in s4.block.modules() if isinstance(m, Linear))
    fp4 = sum(m.weight_fp4.numel() + m.weight_block_scale.numel()
              for m in s4.block.modules() if isinstance(m, Linear))
    assert fp4 * 32 == n * 17                     # 17/32 byte per parameter
