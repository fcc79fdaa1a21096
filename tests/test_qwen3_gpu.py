"""Qwen3 on the GPU: the per-head q/k RMSNorm fused into the RoPE / KV-write kernel
(csrc/kernels/rope_cache.hip, the QKN instantiations of rope_cache_kernel_v8) against the torch
reference, bit-identity of its split-K partial inputs, out-of-bounds canaries, shape rejection,
and Qwen3-shaped stages on the HIP kernels against the CPU reference path.

Run on an MI355X: ``python -m pytest tests/test_qwen3_gpu.py -m gpu``.
"""
import functools

import pytest
import torch

from distributed_llm_inference import ops
from distributed_llm_inference.config import PRESETS
from distributed_llm_inference.models import CausalLMStage
from distributed_llm_inference.ops import reference as ref

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F8 = torch.float8_e4m3fn
EPS = 1e-6
G = 4096  # guard elements on each side
SENT = -12345.0


def _close(a, b, atol, rtol=0.0, msg=""):
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol)
    assert not bad.any(), f"{msg} max err {err.max().item():.4g} at {bad.nonzero()[:5].tolist()}"


def _make_cache(nblocks, nkv, bs, D, dev):
    k = torch.randn(nblocks, nkv, bs, D, device=dev, dtype=BF)
    v = torch.randn(nblocks, nkv, bs // 8, D, 8, device=dev, dtype=BF)
    return k, v


def _guarded(shape, dtype, dev, fill=SENT):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((G + n + G,), fill, dtype=dtype, device=dev)
    return buf, buf[G:G + n].view(*shape)


def _norm_weights(D, dev):
    """q_norm / k_norm weights from N(1, 0.3): far enough from 1 that leaving them out, or
    swapping them, fails every comparison below."""
    return ((1 + 0.3 * torch.randn(D, device=dev)).to(BF),
            (1 + 0.3 * torch.randn(D, device=dev)).to(BF))


# ------------------------------------------------------------------ 5. kernel vs reference
# (16, 8, 128): 32 heads in all = 4 full workgroups of 8 heads, the last one all-v;
# (2, 1, 256): gpr = 16 lanes per head, 3 q/k heads = 48 items in a partly filled wave, and
# (32, 8, 128) / D = 256 with 8 heads per workgroup take one / two loop trips
SHAPES = [(32, 8, 128), (16, 8, 128), (4, 2, 64), (4, 2, 32), (2, 1, 256)]


@pytest.mark.parametrize("nh,nkv,D", SHAPES)
@pytest.mark.parametrize("window", [0, 100])
@pytest.mark.parametrize("fp8", [False, True])
def test_rope_cache_qk_norm_matches_reference(gpu, nh, nkv, D, window, fp8):
    torch.manual_seed(1)
    T, bs, nblocks = 37, 64, 16
    ks, vs = (0.5, 0.25) if fp8 else (1.0, 1.0)
    qkv = torch.randn(T, (nh + 2 * nkv) * D, device=gpu, dtype=BF)
    qw, kw = _norm_weights(D, gpu)
    pos = torch.randint(0, 300, (T,), device=gpu, dtype=torch.int32)
    slots = torch.randperm(nblocks * bs, device=gpu)[:T].to(torch.int64)
    slots[3] = -1  # a token that is not written
    cs = ref.build_cos_sin(D, 512, 1000000.0, device=gpu)
    k1, v1 = _make_cache(nblocks, nkv, bs, D, gpu)
    if fp8:
        k1, v1 = (k1.float() / ks).to(F8), (v1.float() / vs).to(F8)
    k2, v2 = k1.clone().cpu(), v1.clone().cpu()
    q, qs = ops.rope_cache(qkv, pos, slots, cs, nh, nkv, D, k1, v1, window=window,
                           want_sink=window > 0, k_scale=ks, v_scale=vs, q_norm=qw, k_norm=kw,
                           norm_eps=EPS)
    q_r, qs_r = ref.rope_cache(qkv.cpu(), pos.cpu(), slots.cpu(), cs.cpu(), nh, nkv, D, k2, v2,
                               window, window > 0, ks, vs, qw.cpu(), kw.cpu(), EPS)
    _close(q, q_r, 2e-2, 1e-2, "q")
    if window:
        _close(qs, qs_r, 2e-2, 1e-2, "q_sink")
    else:
        assert qs is None
    if fp8:
        # dequantised K within one e4m3 step (3 mantissa bits) of the reference's dequantised K
        _close(k1.float() * ks, k2.float() * ks, 1e-2, 0.125, "k_cache (fp8)")
        assert torch.equal(v1.cpu().view(torch.uint8), v2.view(torch.uint8))
    else:
        _close(k1, k2, 2e-2, 1e-2, "k_cache")
        _close(v1, v2, 0.0, 0.0, "v_cache")


# ------------------------------------------------------------------ 6. split-K partials
@pytest.mark.parametrize("nh,nkv,D", [(32, 8, 128), (4, 2, 32)])
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("S,parts_bf16", [(3, False), (2, True)])
def test_rope_cache_qk_norm_from_splitk_partials_bit_identical(gpu, nh, nkv, D, fp8, S,
                                                               parts_bf16):
    """fp32 (S = 3) and bf16 (S = 2) split-K partials through the QK-norm kernel == the
    materialised bf16 input through the same kernel: q, q_sink and both caches, bit for bit."""
    torch.manual_seed(4)
    T, bs, nblocks = 29, 64, 8
    parts = torch.randn(S, T, (nh + 2 * nkv) * D, device=gpu)
    if parts_bf16:
        parts = parts.to(BF)
    qw, kw = _norm_weights(D, gpu)
    pos = torch.randint(0, 300, (T,), device=gpu, dtype=torch.int32)
    slots = torch.randperm(nblocks * bs, device=gpu)[:T].to(torch.int64)
    slots[5] = -1
    cs = ref.build_cos_sin(D, 512, 1000000.0, device=gpu)
    k1, v1 = _make_cache(nblocks, nkv, bs, D, gpu)
    if fp8:
        k1, v1 = k1.to(F8), v1.to(F8)
    k2, v2 = k1.clone(), v1.clone()
    qkv = ops.SplitKPartials(parts).materialize()
    kw_args = dict(window=100, want_sink=True, k_scale=0.5, v_scale=0.25, q_norm=qw, k_norm=kw,
                   norm_eps=EPS)
    q1, qs1 = ops.rope_cache(qkv, pos, slots, cs, nh, nkv, D, k1, v1, **kw_args)
    q2, qs2 = ops.rope_cache(ops.SplitKPartials(parts), pos, slots, cs, nh, nkv, D, k2, v2,
                             **kw_args)
    assert torch.equal(q1, q2) and torch.equal(qs1, qs2)
    assert torch.equal(k1.view(torch.uint8), k2.view(torch.uint8))
    assert torch.equal(v1.view(torch.uint8), v2.view(torch.uint8))
    # and the norm was applied: the un-normalised kernel gives another q
    q0, _ = ops.rope_cache(qkv, pos, slots, cs, nh, nkv, D, k2.clone(), v2.clone())
    assert not torch.equal(q0, q1)


# ------------------------------------------------------------------ 7. canaries
def test_rope_cache_qk_norm_writes_only_its_slots(gpu):
    nh, nkv, D, bs, nblocks, T = 8, 2, 128, 64, 12, 50
    qkv = torch.randn(T, (nh + 2 * nkv) * D, device=gpu, dtype=BF)
    qw, kw = _norm_weights(D, gpu)
    pos = torch.arange(T, device=gpu, dtype=torch.int32)
    # the tokens land in blocks 3 and 7 only; every other block must stay at the sentinel
    slots = torch.cat([torch.arange(3 * bs, 3 * bs + 32), torch.arange(7 * bs + 5, 7 * bs + 23)])
    slots = slots.to(torch.int64).to(gpu)
    kc = torch.full((nblocks, nkv, bs, D), SENT, device=gpu, dtype=BF)
    vc = torch.full((nblocks, nkv, bs // 8, D, 8), SENT, device=gpu, dtype=BF)
    cs = ref.build_cos_sin(D, 256, 1000000.0, device=gpu)
    qbuf, q_out = _guarded((T, nh, D), BF, gpu)
    ops.rope_cache(qkv, pos, slots, cs, nh, nkv, D, kc, vc, q_out=q_out, q_norm=qw, k_norm=kw,
                   norm_eps=EPS)
    torch.cuda.synchronize()
    s = torch.tensor(SENT, dtype=BF)
    n = T * nh * D
    assert bool((qbuf[:G].cpu() == s).all()), "rope q_out: write before the output"
    assert bool((qbuf[G + n:].cpu() == s).all()), "rope q_out: write after the output"
    assert not bool((q_out.cpu() == s).any()), "rope q_out: an element was not written"
    written = torch.zeros(nblocks * bs, dtype=torch.bool)
    written[slots.cpu()] = True
    k_slot = kc.cpu().permute(0, 2, 1, 3).reshape(nblocks * bs, -1)
    v_slot = vc.cpu().permute(0, 2, 4, 1, 3).reshape(nblocks * bs, -1)
    for name, c in (("k_cache", k_slot), ("v_cache", v_slot)):
        untouched = (c == s).all(-1)
        assert bool(untouched[~written].all()), f"{name}: write outside the slot mapping"
        assert not bool(untouched[written].any()), f"{name}: a mapped slot was not written"


# ------------------------------------------------------------------ 8. rejection
def test_rope_cache_qk_norm_rejects_unsupported_shapes(gpu):
    """head_dim 96 (6 lanes per head: no butterfly), a weight of the wrong length, one weight
    without the other, and a row stride off the 16-byte path all raise before any launch: q_out
    and the caches keep their sentinel."""
    nh, nkv, T, bs, nblocks = 4, 2, 5, 64, 2
    pos = torch.arange(T, device=gpu, dtype=torch.int32)
    slots = torch.arange(T, device=gpu, dtype=torch.int64)

    def attempt(D, wlen, match, k_norm=True, pad=0, exc=RuntimeError):
        width = (nh + 2 * nkv) * D
        qkv = torch.randn(T, width + pad, device=gpu, dtype=BF)[:, :width]
        kc = torch.full((nblocks, nkv, bs, D), SENT, device=gpu, dtype=BF)
        vc = torch.full((nblocks, nkv, bs // 8, D, 8), SENT, device=gpu, dtype=BF)
        q_out = torch.full((T, nh, D), SENT, device=gpu, dtype=BF)
        cs = ref.build_cos_sin(D, 64, 1000000.0, device=gpu)
        w = torch.ones(wlen, device=gpu, dtype=BF)
        with pytest.raises(exc, match=match):
            ops.rope_cache(qkv, pos, slots, cs, nh, nkv, D, kc, vc, q_out=q_out, q_norm=w,
                           k_norm=w.clone() if k_norm else None, norm_eps=EPS)
        torch.cuda.synchronize()
        s = torch.tensor(SENT, dtype=BF, device=gpu)
        for t in (q_out, kc, vc):
            assert bool((t == s).all()), "a rejected call wrote something"

    attempt(96, 96, "head_dim")
    attempt(128, 64, "head_dim elements")
    attempt(128, 128, "together", k_norm=False, exc=ValueError)
    attempt(128, 128, "head_dim", pad=4)   # row stride % 8 != 0: the 4-element kernel's case


# ------------------------------------------------------------------ 9, 10. stages, GPU vs CPU
def _randomise_qk_norms(stage, seed=3):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for layer in stage.block.layers:
            for n in (layer.self_attn.q_norm, layer.self_attn.k_norm):
                n.weight.copy_((1 + 0.3 * torch.randn(n.weight.shape, generator=g)).to(BF))


PROMPTS = [list(range(1, 90)), [5, 6, 7], list(range(100, 117)), [9, 8, 7, 6, 5]]


@functools.lru_cache(maxsize=None)
def _cpu_stage(preset):
    spec = PRESETS[preset].replace(num_layers=2, vocab_size=4096)
    cpu = CausalLMStage(spec, 0, 2).init_random(7)
    _randomise_qk_norms(cpu)
    return cpu


@functools.lru_cache(maxsize=None)
def _gpu_stage(preset):
    cpu = _cpu_stage(preset)
    g = CausalLMStage(cpu.spec, 0, 2, device="cuda:0")
    g.load_state_dict({k: v.to("cuda:0") for k, v in cpu.state_dict().items()})
    g.block.set_fused_swiglu(True)   # as the engine runs decode; enables the 1-2 row GEMV layer
    return g


def _run(stage, prompts, steps, kv_fp8, tokens=None, spy=None):
    """Prefill ``prompts`` as one varlen batch, then ``steps`` decode steps fed ``tokens[i]``
    (default: this run's argmax); returns the logits of every call."""
    kw = dict(kv_dtype=F8, k_scale=0.5, v_scale=0.25) if kv_fp8 else {}
    pool = stage.make_pool(64, block_size=64, **kw)
    dev = stage.device
    sids = list(range(len(prompts)))
    for s, p in zip(sids, prompts):
        pool.manager.append(s, len(p))
    meta = pool.build_metadata(sids, [len(p) for p in prompts])
    meta.logits_rows = (torch.cumsum(torch.tensor([len(p) for p in prompts]), 0) - 1).to(dev)
    ids = torch.tensor([t for p in prompts for t in p], dtype=torch.int32, device=dev)
    outs = [stage(ids, meta, pool).float().cpu()]
    for i in range(steps):
        toks = tokens[i] if tokens is not None else outs[-1].argmax(-1)
        for s in sids:
            pool.manager.append(s, 1)
        meta = pool.build_metadata(sids, [1] * len(sids))
        if spy is not None:
            spy.clear()
        outs.append(stage(toks.to(torch.int32).to(dev), meta, pool).float().cpu())
    return outs


@functools.lru_cache(maxsize=None)
def _cpu_run(preset, nseq, steps, kv_fp8):
    return _run(_cpu_stage(preset), PROMPTS[:nseq], steps, kv_fp8)


class _Spy:
    """ops.native() with the two RoPE entry points recorded: (name, q_norm given, input dtype,
    input rank) per call."""

    def __init__(self, calls):
        self._mod, self._calls = ops.native(), calls

    def __getattr__(self, k):
        f = getattr(self._mod, k)
        if k not in ("rope_cache", "skinny_gemm_qkv_rope"):
            return f

        def wrapped(*a, **kw):
            normed = k == "rope_cache" and len(a) > 13 and a[13] is not None
            self._calls.append((k, normed, a[0].dim()))
            return f(*a, **kw)
        return wrapped


@pytest.mark.parametrize("nseq,kv_fp8", [(2, False), (4, False), (2, True)])
def test_qwen3_8b_layers_gpu_match_cpu(gpu, monkeypatch, nseq, kv_fp8):
    """Two real-size qwen3-8b layers on the HIP kernels vs the CPU reference path: prefill (89-
    and 3-token prompts first), then two decode steps fed the CPU run's tokens.  Two rows decode on
    the GEMV layer with the unfused RoPE kernel; four rows feed it the QKV split-K partials."""
    preset = "qwen3-8b"
    ref_outs = _cpu_run(preset, nseq, 2, kv_fp8)
    tokens = [o.argmax(-1) for o in ref_outs[:-1]]
    calls = []
    spy = _Spy(calls)
    monkeypatch.setattr(ops, "native", lambda: spy)
    # four rows: below 128 rows the projections go to the library by default; kept on the tile
    # GEMM, its QKV product is split over K and handed over un-reduced
    with ops.kernel_policy(**(dict(library_gemms=False) if nseq == 4 else {})):
        outs = _run(_gpu_stage(preset), PROMPTS[:nseq], 2, kv_fp8, tokens=tokens, spy=calls)
    for step, (a, b) in enumerate(zip(ref_outs, outs)):
        rel = ((a - b).norm() / a.norm()).item()
        print(f"nseq={nseq} kv_fp8={kv_fp8} step={step} rel={rel:.5f}")
        assert rel < 0.03, (step, rel)
    # the last decode step: one normalising RoPE launch per layer, never the GEMV's RoPE epilogue
    assert [c[:2] for c in calls] == [("rope_cache", True)] * 2, calls
    if nseq == 4:   # the tile GEMM's un-reduced partials [S, T, N] went into the kernel
        assert all(c[2] == 3 for c in calls), calls


def test_qwen3_06b_layers_gpu_match_cpu(gpu):
    """qwen3-0.6b's shape (tied embeddings, q_size 2048 != hidden 1024): prefill and one decode
    step, GPU vs CPU."""
    preset = "qwen3-0.6b"
    spec = _cpu_stage(preset).spec
    assert spec.tie_word_embeddings and spec.q_size != spec.hidden_size
    ref_outs = _cpu_run(preset, 2, 1, False)
    outs = _run(_gpu_stage(preset), PROMPTS[:2], 1, False,
                tokens=[o.argmax(-1) for o in ref_outs[:-1]])
    for step, (a, b) in enumerate(zip(ref_outs, outs)):
        rel = ((a - b).norm() / a.norm()).item()
        print(f"0.6b step={step} rel={rel:.5f}")
        assert rel < 0.03, (step, rel)
