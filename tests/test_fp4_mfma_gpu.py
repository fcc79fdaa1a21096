"""The MFMA-native MXFP4 path (``KernelPolicy.fp4_mfma``) on the GPU: the MX fp8 activation
quantiser (quant.hip) bit for bit against its torch rule, the fp4 x fp8 block-scaled tile GEMM
(gemm_fp4.hip) bit for bit on exactly representable data and within the fp8 tile GEMM's bound on
random data, and the mode through ``Linear``, ``LlamaMLP``, a stage and the engine."""
import pytest
import torch

from distributed_llm_inference import ops
from distributed_llm_inference.config import CacheConfig, KernelPolicy, ModelSpec, ServeConfig
from distributed_llm_inference.models import CausalLMStage
from distributed_llm_inference.models.common import Linear
from distributed_llm_inference.models.llama.modules import LlamaMLP
from distributed_llm_inference.ops import reference as ref
from distributed_llm_inference.runtime.engine import EngineConfig, LLMEngine
from distributed_llm_inference.runtime.sequence import SamplingParams

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
FP8 = torch.float8_e4m3fn
G = 4096          # guard elements on each side of a guarded output
SENT = -12345.0

# every projection eligible (N % 256 == 0, K % 128 == 0): qkv 512, o 256, gate|up 1024, down 256
SPEC = ModelSpec(name="t", vocab_size=1000, hidden_size=256, intermediate_size=512, num_layers=4,
                 num_heads=8, num_kv_heads=4, head_dim=32, rope_theta=10000.0,
                 max_position_embeddings=4096)


def _wide_weight(n, k, seed, lo=-14, hi=-3):
    """Random weights whose per-block magnitudes span 2^lo .. 2^hi (tests/test_mxfp4_gpu.py)."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, k // 32, 32, generator=g)
    ex = torch.randint(lo, hi + 1, (n, k // 32, 1), generator=g).float()
    return (w * torch.exp2(ex)).reshape(n, k)


def _mx_from_exponents(q, e):
    """MxFp8 from e4m3 ``q`` [M, K] and int exponents ``e`` [M, K / 128] (mx_off layout)."""
    M, K = q.shape
    nb = (M + 63) // 64
    sc = torch.full((K // 128, nb * 64), 127, dtype=torch.uint8)
    r = torch.arange(M)
    sc[:, (r // 64) * 64 + (r % 16) * 4 + (r % 64) // 16] = (e + 127).to(torch.uint8).t()
    return ops.MxFp8(q, sc.view(-1))


def _to(a, dev):
    return ops.MxFp8(a.q.to(dev), a.sc.to(dev))


# ------------------------------------------------------------------------------- G1: quantiser
def _quant_input(M, K, seed):
    """bf16 rows whose per-block magnitudes span 2^-20 .. 2^10, with an all-zero block, a block
    whose amax / 448 is an exact power of two and one that hits the exponent clamp (amax 2^-131:
    k = -139 clamps to -126)."""
    g = torch.Generator().manual_seed(seed)
    nkb = K // 128
    x = torch.randn(M, nkb, 128, generator=g)
    x = x * torch.exp2(torch.randint(-20, 11, (M, nkb, 1), generator=g).float())
    x[0, 0] = 0.0
    x[M // 2, nkb // 2] = torch.randn(128, generator=g).clamp(-1, 1) * 3.0
    x[M // 2, nkb // 2, 5] = -448.0 * 2.0 ** -7          # amax = 3.5: amax / 448 = 2^-7 exactly
    x[M - 1, nkb - 1] = torch.randn(128, generator=g).clamp(-1, 1) * 2.0 ** -131
    x[M - 1, nkb - 1, 77] = 2.0 ** -131
    if M * nkb == 1:      # a single block: keep the power-of-two case, the others need more blocks
        x[0, 0] = torch.randn(128, generator=g).clamp(-1, 1) * 3.0
        x[0, 0, 9] = 448.0 * 2.0 ** -6
    return x.reshape(M, K).to(BF)


@pytest.mark.parametrize("K", [128, 384, 8192])
@pytest.mark.parametrize("M", [1, 3, 64, 70, 257])
def test_quant_mx_bit_exact(gpu, M, K):
    x = _quant_input(M, K, M * 131 + K)
    want = ops.mx_quantize(x)
    nsc = K // 128 * ((M + 63) // 64) * 64
    assert want.sc.numel() == nsc
    qbuf = torch.full((G + M * K + G,), 0xAB, dtype=torch.uint8, device=gpu)
    sbuf = torch.full((G + nsc + G,), 0xAB, dtype=torch.uint8, device=gpu)
    q, sc = qbuf[G:G + M * K].view(M, K), sbuf[G:G + nsc]
    ops.native().quant_mx(q, sc, x.to(gpu))
    torch.cuda.synchronize()
    for buf, n in ((qbuf, M * K), (sbuf, nsc)):
        assert bool((buf[:G] == 0xAB).all()) and bool((buf[G + n:] == 0xAB).all()), "guard written"
    assert torch.equal(sc.cpu(), want.sc), "scale bytes (pad rows hold 127)"
    assert torch.equal(q.cpu(), want.q.view(torch.uint8)), "e4m3 bytes"
    # the pad rows [M, 64 nb) of every block column hold 127 (checked above through the oracle;
    # here against the layout itself)
    e = ops.MxFp8(q, sc).exponents().cpu()
    assert torch.equal(e, want.exponents())
    assert int((sc == 127).sum()) >= nsc - M * (K // 128)
    # the front-end returns the same thing
    a = ops.quant_mx(x.to(gpu))
    assert a.q.dtype == FP8 and torch.equal(a.q.view(torch.uint8), q) and torch.equal(a.sc, sc)


def test_quant_mx_rejects_bad_shapes(gpu):
    with pytest.raises((ValueError, RuntimeError)):
        ops.quant_mx(torch.zeros(4, 96, dtype=BF, device=gpu))
    with pytest.raises((ValueError, RuntimeError)):
        ops.quant_mx(torch.zeros(4, 128, dtype=torch.float32, device=gpu))
    with pytest.raises(RuntimeError):   # a scale array of another M
        ops.native().quant_mx(torch.empty(4, 128, dtype=torch.uint8, device=gpu),
                              torch.empty(128, dtype=torch.uint8, device=gpu),
                              torch.zeros(4, 128, dtype=BF, device=gpu))


# ------------------------------------------------------------------------------- G2: layout
def _exact_case(M, N, K, seed):
    """Operands whose every product is a multiple of 2^-2 of magnitude <= 96, so any summation
    order is exact in fp32 at K <= 1024.  Asymmetric everywhere: all 16 nibble codes, weight scale
    bytes in {126, 127, 128} per (row, 32-block), activations integers in [-4, 4] with scale bytes
    in {127, 128} per (row, 128-block)."""
    g = torch.Generator().manual_seed(seed)
    packed = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.uint8)
    packed[0, :8] = torch.tensor([0x10, 0x32, 0x54, 0x76, 0x98, 0xBA, 0xDC, 0xFE], dtype=torch.uint8)
    scales = torch.randint(126, 129, (N, K // 32), generator=g, dtype=torch.uint8)
    xi = torch.randint(-4, 5, (M, K), generator=g).float()
    e = torch.randint(0, 2, (M, K // 128), generator=g)
    a = _mx_from_exponents(xi.to(FP8), e)
    codes = torch.cat([packed & 15, packed >> 4]).unique()
    assert codes.numel() == 16
    wd = ref.dequantize_mxfp4(packed, scales).double()
    ad = a.dequantize().double()
    assert torch.equal(ad, xi.double() * torch.exp2(e.double()).repeat_interleave(128, dim=1))
    # the precondition of bit-exactness, on this data: products are multiples of 1/4, <= 96, and
    # even the sum of magnitudes stays far inside fp32's 24 bits
    assert float(wd.abs().max()) <= 12 and float(ad.abs().max()) <= 8
    assert torch.equal(wd * 4, (wd * 4).round()) and torch.equal(ad, ad.round())
    assert float((ad.abs() @ wd.abs().t()).max()) * 4 < 2 ** 23
    want = (ad @ wd.t()).float().to(BF)
    return a, packed, scales, want


@pytest.mark.parametrize("K", [128, 384, 1024])
@pytest.mark.parametrize("N", [256, 768])
@pytest.mark.parametrize("M", [3, 17, 256, 300])
def test_gemm_fp4_layout_bit_exact(gpu, M, N, K):
    a, packed, scales, want = _exact_case(M, N, K, M * 7 + N + K)
    ag, pg, sg = _to(a, gpu), packed.to(gpu), scales.to(gpu)
    tail = 256 * N + G      # rows M .. 255 of the last tile would land here
    for splits in (1, 2, 3):
        if splits > K // 128:
            continue
        # epilogue 0 (split-K: fp32 slabs reduced inside the launch sequence)
        cbuf = torch.full((G + M * N + tail,), SENT, dtype=BF, device=gpu)
        out = cbuf[G:G + M * N].view(M, N)
        ws = (torch.empty(splits * M * N, dtype=torch.float32, device=gpu) if splits > 1 else None)
        ops.native().gemm_fp4(out, ag.q, ag.sc, pg, sg, splits, 0, ws)
        torch.cuda.synchronize()
        assert bool((cbuf[:G] == SENT).all()), "write before C"
        assert bool((cbuf[G + M * N:] == SENT).all()), "write after C (rows past M stored?)"
        assert torch.equal(out.cpu(), want), (splits, (out.cpu().float() - want.float()).abs().max())
        assert torch.equal(ops.gemm_fp4_mx(ag, pg, sg, splits=splits).cpu(), want)
        if splits == 1:
            continue
        # epilogue 1: the slabs alone, between guards, then the reduce pass
        pbuf = torch.full((G + splits * M * N + tail,), SENT, dtype=torch.float32, device=gpu)
        parts = pbuf[G:G + splits * M * N]
        dummy = torch.empty(M, 0, dtype=BF, device=gpu)
        ops.native().gemm_fp4(dummy, ag.q, ag.sc, pg, sg, splits, 1, parts)
        red = torch.empty(M, N, dtype=BF, device=gpu)
        ops.native().splitk_reduce(red, parts.view(splits, M, N))
        torch.cuda.synchronize()
        assert bool((pbuf[:G] == SENT).all()) and bool((pbuf[G + splits * M * N:] == SENT).all())
        assert torch.equal(red.cpu(), want), splits
        y = ops.gemm_fp4_mx(ag, pg, sg, splits=splits, defer_reduce=True)
        assert isinstance(y, ops.SplitKPartials) and y.parts.dtype == torch.float32
        assert torch.equal(y.materialize().cpu(), want)


# ------------------------------------------------------------------------------- G3: random data
_RANDOM = {}


def _random_case(M, N, K, gpu):
    """(MxFp8 activations, packed, scales, fp32 reference product) on the GPU, built once."""
    key = (M, N, K)
    if key not in _RANDOM:
        packed, scales = ops.quantize_weight_mxfp4(_wide_weight(N, K, N + K, -8, -4))
        g = torch.Generator().manual_seed(M + K)
        x = torch.randn(M, K, generator=g).to(BF)
        a = ops.quant_mx(x.to(gpu))
        want = ops.mx_quantize(x).dequantize() @ ref.dequantize_mxfp4(packed, scales).float().t()
        _RANDOM[key] = (a, packed.to(gpu), scales.to(gpu), want)
    return _RANDOM[key]


SHAPES = [(100, 768, 1024), (512, 1024, 8192), (33, 256, 384)]


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_fp4_random_against_fp32_oracle(gpu, M, N, K):
    a, packed, scales, want = _random_case(M, N, K, gpu)
    bound = 2e-2 * float(want.abs().max())
    for splits in sorted({1, ops.tile_gemm_splits_fp4(M, N, K)}):
        y = ops.gemm_fp4_mx(a, packed, scales, splits=splits)
        assert y.dtype == BF and y.shape == (M, N)
        err = float((y.float().cpu() - want).abs().max())
        print(f"gemm_fp4 M={M} N={N} K={K} splits={splits}: max err {err:.4g} bound {bound:.4g}")
        assert err < bound, (splits, err, bound)


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_fp4_swiglu_epilogue(gpu, M, N, K):
    """The weight rows are taken to be in swiglu_interleave order; the reference applies
    ops.silu_mul to the bf16-rounded product with its columns put back into [gate | up] order."""
    a, packed, scales, want = _random_case(M, N, K, gpu)
    gu = ops.swiglu_deinterleave(want.to(BF).t().contiguous()).t().contiguous()
    h = ops.silu_mul(gu).float()
    buf = torch.full((G + M * (N // 2) + G,), SENT, dtype=BF, device=gpu)
    out = buf[G:G + M * (N // 2)].view(M, N // 2)
    y = ops.gemm_fp4_mx(a, packed, scales, swiglu=True, out=out)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr()
    assert bool((buf[:G] == SENT).all()) and bool((buf[G + M * (N // 2):] == SENT).all())
    err, bound = float((y.float().cpu() - h).abs().max()), 2e-2 * float(h.abs().max())
    print(f"gemm_fp4 swiglu M={M} N={N} K={K}: max err {err:.4g} bound {bound:.4g}")
    assert err < bound, (err, bound)


def test_gemm_fp4_rejects_bad_shapes(gpu):
    def operands(M, N, K):
        a = ops.MxFp8(torch.zeros(M, K, device=gpu).to(FP8),
                      torch.full((max(K // 128, 1) * 64,), 127, dtype=torch.uint8, device=gpu))
        return (a, torch.zeros(N, K // 2, dtype=torch.uint8, device=gpu),
                torch.full((N, K // 32), 127, dtype=torch.uint8, device=gpu))

    for M, N, K, splits in [(4, 384, 128, 1), (4, 256, 96, 1), (4, 256, 256, 3), (4, 256, 384, 4),
                            (4, 256, 512, 3)]:   # 4 k-tiles do not go 3 ways (2 + 2 + 0)
        a, p, s = operands(M, N, K)
        with pytest.raises((ValueError, RuntimeError)):
            ops.gemm_fp4_mx(a, p, s, splits=splits)
        out = torch.empty(M, N, dtype=BF, device=gpu)
        ws = torch.empty(max(splits, 1) * M * N, dtype=torch.float32, device=gpu)
        with pytest.raises(RuntimeError):
            ops.native().gemm_fp4(out, a.q, a.sc, p, s, splits, 0, ws)
    a, p, s = operands(4, 256, 256)
    with pytest.raises((ValueError, RuntimeError)):      # SwiGLU takes whole-K tiles
        ops.gemm_fp4_mx(a, p, s, splits=2, swiglu=True)
    with pytest.raises(RuntimeError):                    # scales of another M
        ops.native().gemm_fp4(torch.empty(4, 256, dtype=BF, device=gpu), a.q, a.sc[:32].contiguous(),
                              p, s, 1, 0, None)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------- G4: modules
def _spy(monkeypatch):
    calls = {"fp4": 0, "deq": 0}
    real_fp4, real_deq = ops.gemm_fp4_mx, ops.dequantize_mxfp4

    def fp4(*a, **kw):
        calls["fp4"] += 1
        return real_fp4(*a, **kw)

    def deq(*a, **kw):
        calls["deq"] += 1
        return real_deq(*a, **kw)

    monkeypatch.setattr(ops, "gemm_fp4_mx", fp4)
    monkeypatch.setattr(ops, "dequantize_mxfp4", deq)
    return calls


def _dense(y):
    return (y.materialize() if isinstance(y, ops.SplitKPartials) else y).float().cpu()


def test_linear_and_mlp_take_the_mfma_path(gpu, monkeypatch):
    K, N = 1024, 1024
    cl = Linear(K, N)
    cl.weight.data.copy_(_wide_weight(N, K, 9).to(BF))
    gl = Linear(K, N, device=gpu)
    gl.weight.data.copy_(cl.weight.data)
    cl.quantize_mxfp4()
    gl.quantize_mxfp4()
    spec = SPEC.replace(hidden_size=512, intermediate_size=1024)
    cm, gm = LlamaMLP(spec), LlamaMLP(spec, device=gpu)
    for a, b, seed in ((cm.gate_up_proj, gm.gate_up_proj, 1), (cm.down_proj, gm.down_proj, 2)):
        a.weight.data.copy_(_wide_weight(a.out_features, a.in_features, seed, -8, -4).to(BF))
        b.weight.data.copy_(a.weight.data)
        a.quantize_mxfp4()
        b.quantize_mxfp4()
    cm.set_fused_swiglu(True)
    gm.set_fused_swiglu(True)
    assert gm.fused_swiglu and torch.equal(gm.gate_up_proj.weight_fp4.cpu(), cm.gate_up_proj.weight_fp4)
    with ops.kernel_policy(fp4_mfma=True):
        for M in (4, 384):
            g = torch.Generator().manual_seed(M)
            x = torch.randn(M, K, generator=g).to(BF)
            xm = torch.randn(M, 512, generator=g).to(BF)
            want, want_m = cl(x).float(), cm(xm).float()
            calls = _spy(monkeypatch)
            deferred = False
            for defer in (False, True):
                y = gl(x.to(gpu), defer_reduce=defer)
                deferred |= isinstance(y, ops.SplitKPartials)
                err, bound = float((_dense(y) - want).abs().max()), 2e-2 * float(want.abs().max())
                assert err < bound, (M, defer, err, bound)
                ym = gm(xm.to(gpu), defer_reduce=defer)
                err, bound = float((_dense(ym) - want_m).abs().max()), 2e-2 * float(want_m.abs().max())
                assert err < bound, ("mlp", M, defer, err, bound)
            assert deferred                       # the split-K partials reach the caller
            assert calls["fp4"] == 2 * 3 and calls["deq"] == 0, calls
            monkeypatch.undo()
    # flag off: the same modules are back on the dequantise path
    calls = _spy(monkeypatch)
    gl(torch.zeros(4, K, dtype=BF, device=gpu))
    assert calls["fp4"] == 0 and calls["deq"] == 1, calls


# ------------------------------------------------------------------------------- G5: stage
def _stage_logits(stage, prompts):
    pool = stage.make_pool(128, block_size=64)
    sids = list(range(len(prompts)))
    for s, p in zip(sids, prompts):
        pool.manager.append(s, len(p))
    meta = pool.build_metadata(sids, [len(p) for p in prompts])
    meta.logits_rows = (torch.cumsum(torch.tensor([len(p) for p in prompts]), 0) - 1).to(stage.device)
    ids = torch.tensor([t for p in prompts for t in p], dtype=torch.int32, device=stage.device)
    return stage(ids, meta, pool).float().cpu()


def _rel(a, b):
    return float((a - b).norm() / a.norm())


def test_fp4_mfma_stage(gpu, monkeypatch):
    """GPU against CPU with the flag on (two pipelines that round alike but sum differently), and
    flag on against flag off on the GPU: the new path adds fp8 activation rounding only, so it
    must sit closer to the dequantise path than fp8 weights sit to bf16 (which pays the same
    activation rounding plus its weight rounding).  Measured on an MI355X (seed 3): see
    docs/kernels.md "MXFP4 weights"."""
    prompts = [list(range(1, 70)), [5, 6, 7]]
    seed = 3
    cpu = CausalLMStage(SPEC, 0, 4).init_random(seed)
    state = {k: v.to(gpu) for k, v in cpu.state_dict().items()}

    def gpu_stage(mode):
        s = CausalLMStage(SPEC, 0, 4, device=gpu).init_random(seed)
        s.load_state_dict(state)
        return s.quantize(mode) if mode else s

    bf16 = _stage_logits(gpu_stage(None), prompts)
    fp8 = _stage_logits(gpu_stage("fp8"), prompts)
    cpu.quantize("mxfp4")
    g4 = gpu_stage("mxfp4")
    off = _stage_logits(g4, prompts)
    calls = _spy(monkeypatch)
    with ops.kernel_policy(fp4_mfma=True):
        on = _stage_logits(g4, prompts)
        assert calls["fp4"] == 4 * len(g4.block.layers) and calls["deq"] == 0, calls
        on_cpu = _stage_logits(cpu, prompts)
    d_cpu, d_flag, d_fp8 = _rel(on_cpu, on), _rel(off, on), _rel(bf16, fp8)
    print(f"fp4_mfma stage: gpu vs cpu {d_cpu:.4f}, flag on vs off {d_flag:.4f}, "
          f"fp8 vs bf16 {d_fp8:.4f}, mxfp4 off / on vs bf16 {_rel(bf16, off):.4f} / {_rel(bf16, on):.4f}")
    assert d_cpu < 0.08, d_cpu
    assert d_flag < d_fp8, (d_flag, d_fp8)


# ------------------------------------------------------------------------------- G6: engine
def _engine(graphs):
    cfg = EngineConfig(model="t", pp=1, seed=5, quantize="mxfp4",
                       kernels=KernelPolicy().with_overrides("fp4_mfma=1"),
                       cache=CacheConfig(num_blocks=256, block_size=64, max_chunk=256),
                       serve=ServeConfig(max_batch_size=8, max_num_batched_tokens=512,
                                         max_seq_len=1024, use_graphs=graphs,
                                         graph_batch_sizes=[1, 2, 4, 8]))
    return LLMEngine(SPEC, device="cuda:0", cfg=cfg)


PROMPTS = [list(range(3, 40)), [7, 8, 9], list(range(200, 330)), [11]]


@pytest.mark.parametrize("nprompts", [2, 4])
def test_fp4_mfma_engine_graph_decode_equals_eager(gpu, monkeypatch, nprompts):
    """4 prompts: every decode step's M = 4 products run on the fp4 MFMA GEMM, captured into the
    decode graph; 2 prompts: the decode rows stay on the fp4 GEMVs.  Neither dequantises a weight
    after start-up.  Counted on the eager engine (the graph engine also captures the buckets it
    does not use)."""
    calls = _spy(monkeypatch)
    calls.update(gemv=0, qkv=0)
    real_gemv, real_qkv = ops.skinny_gemm_fp4, ops.skinny_gemm_qkv_rope

    def gemv(*a, **kw):
        calls["gemv"] += 1
        return real_gemv(*a, **kw)

    def qkv(*a, **kw):
        calls["qkv"] += 1
        return real_qkv(*a, **kw)

    monkeypatch.setattr(ops, "skinny_gemm_fp4", gemv)
    monkeypatch.setattr(ops, "skinny_gemm_qkv_rope", qkv)
    p = SamplingParams(max_tokens=10, ignore_eos=True)
    prompts = PROMPTS[:nprompts]
    eng = _engine(graphs=False)
    assert ops.policy().fp4_mfma
    lins = [m for m in eng.executors[0].stage.block.modules() if isinstance(m, Linear)]
    assert lins and all(m.is_fp4 for m in lins)
    assert all(l.mlp.fused_swiglu for l in eng.executors[0].stage.block.layers)
    calls.update(fp4=0, deq=0, gemv=0, qkv=0)        # start-up warm-ups do not count
    a = [s.output for s in eng.generate(prompts, p)]
    assert calls["deq"] == 0, calls
    if nprompts == 2:
        # per decode step and layer: QKV (RoPE epilogue), O, gate|up, down on the GEMV
        assert calls["qkv"] >= 9 * 4 and calls["gemv"] >= 9 * 4 * 3, calls
        assert 0 < calls["fp4"] <= 16 * nprompts, calls       # the prefill step(s) only
    else:
        assert calls["gemv"] == 0 and calls["qkv"] == 0, calls
        assert calls["fp4"] >= 9 * 16 + 16, calls             # prefill + every decode step
    b = [s.output for s in _engine(graphs=True).generate(prompts, p)]
    assert all(len(o) == 10 for o in a) and a == b
