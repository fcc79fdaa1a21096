"""The grouped MFMA tile GEMM on quantised experts (csrc/kernels/moe_tile.hip, fp8 and MXFP4
instantiations) on the GPU: bit equality with the bf16 tile kernel on the widened weights (the
main check: the quantised kernels run the bf16 kernel's MFMAs in its order), both epilogues
against an fp32 oracle on the dequantised weights and against the 32-row weight-streaming kernel
on explicit ids whose row counts sit on every edge of the 128-row tiling (sentinel rows around
the outputs), row independence under a token permutation, determinism and the host checks, the
MoE block (Qwen2-MoE's shared expert included) and the engine under
``KernelPolicy.moe_tile_rows_q``, and hipGraph replay with changing routing."""
import copy

import pytest
import torch

import moe_tile_cases as mc
from distributed_llm_inference import ops
from distributed_llm_inference.config import CacheConfig, KernelPolicy, ModelSpec, ServeConfig
from distributed_llm_inference.models.llama.modules import MoEMLP
from distributed_llm_inference.runtime.engine import EngineConfig, LLMEngine
from distributed_llm_inference.runtime.sequence import SamplingParams

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
FP8 = torch.float8_e4m3fn
U8 = torch.uint8
SENT = -12345.0
GROWS = 8          # sentinel rows before and after a guarded [rows, width] output
ATOL, RTOL = 2e-2, 2e-2     # tests/test_moe_gpu.py's: the same numerics class
E, K = mc.E, mc.K_TOP
SHAPES = [(256, 128), (1152, 384)]
FMTS = ["fp8", "mxfp4"]
SCALE_KW = {"fp8": "w_scale", "mxfp4": "w_block_scale"}


def _close(a, b, atol, rtol=0.0, msg=""):
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    assert not bad.any(), f"{msg} max err {err.max().item():.4g} at {bad.nonzero()[:5].tolist()}"


def _bits(t):
    return t.contiguous().view(torch.int16)


def _guarded_rows(rows, width, gpu):
    buf = torch.full((GROWS + rows + GROWS, width), SENT, dtype=BF, device=gpu)
    return buf, buf[GROWS:]          # the op sees [rows + GROWS, width]; it may write `rows` rows


def _assert_guards(buf, rows, what):
    assert bool((buf[:GROWS] == SENT).all()), f"{what}: write before the output"
    assert bool((buf[GROWS + rows:] == SENT).all()), f"{what}: write past row P"


def _dequant(fmt, w, s):
    """fp32 [E, N, K] of quantised experts on the CPU."""
    if fmt == "fp8":
        return w.float() * s[:, :, None]
    return torch.stack([ops.dequantize_mxfp4(w[e], s[e]).float() for e in range(w.shape[0])])


# ------------------------------------------------------------------ bit equality with bf16 tiles
def _pow2_scale(N):
    """scale[e, n] = 2^-p, p in 0..7 changing with the row inside a lane's four (n % 4), with the
    16-row fragment, with the 128-row block of a workgroup and with the expert."""
    n = torch.arange(N)
    e = torch.arange(E)[:, None]
    p = ((n % 4) + 3 * ((n // 16) % 4) + 5 * (n // 128) + e) % 8
    for a, b in ((0, 1), (0, 16), (16, 32), (0, 128)):
        assert p[0, a] != p[0, b]
    assert p[0, 0] != p[1, 0]
    return torch.exp2(-p.float())


def _e4m3(shape, g):
    """e4m3 values drawn directly: normals, subnormals and zeros of both signs."""
    w8 = (2.0 * torch.randn(shape, generator=g)).to(FP8)
    assert bool(w8.float().isfinite().all())
    return w8


def _both_products(H, I):
    return ((False, (2 * I, H)), (True, (H, I)))


def _compare_with_bf16_tiles(gpu, r, xin, wq, scale, wb, fmt, down, P, what):
    """The quantised tile kernel on (wq, scale) against the bf16 tile kernel on wb, guard rows
    included, bit for bit."""
    N = wb.shape[1]
    width = N if down else N // 2
    b1, v1 = _guarded_rows(P, width, gpu)
    b2, v2 = _guarded_rows(P, width, gpu)
    want = ops.moe_grouped_gemm(xin, wb.to(gpu), r, down=down, out=v1, tiles=True)
    with ops.kernel_policy(moe_tile_rows_q=64):
        got = ops.moe_grouped_gemm(xin, wq.to(gpu), r, down=down, out=v2, tiles=True,
                                   **{SCALE_KW[fmt]: scale.to(gpu)})
    torch.cuda.synchronize()
    _assert_guards(b1, P, what + " (bf16)")
    _assert_guards(b2, P, what + f" ({fmt})")
    assert bool(want[:P].float().isfinite().all()) and want[:P].float().abs().max() > 1
    assert torch.equal(_bits(got[:P]), _bits(want[:P])), what
    assert torch.equal(_bits(b2), _bits(b1)), what


@pytest.mark.parametrize("H,I", SHAPES)
def test_fp8_tiles_bit_equal_to_bf16_tiles_under_pow2_scales(gpu, H, I):
    """With scale 2^-p the bf16 weight (w8 * scale) is exact, every product and every partial sum
    of the bf16 tile kernel is the fp8 tile kernel's times 2^-p, and the epilogue's acc * scale
    restores it before the rounding (gate and up each before theirs): the outputs are equal bit
    for bit -- as long as the fp8 kernel reads the bytes in the bf16 kernel's k order through its
    own swizzle and takes the scale of the right expert and row."""
    g = torch.Generator().manual_seed(11 * H + I)
    ids = mc.explicit_ids()
    T = ids.shape[0]
    P = T * K
    x = torch.randn(T, H, generator=g).to(BF)
    tw = torch.rand(T, K, generator=g).to(BF).float()
    r = ops.moe_group(ids.to(gpu), tw.to(gpu), E)
    for down, (N, Kd) in _both_products(H, I):
        w8 = _e4m3((E, N, Kd), g)
        scale = _pow2_scale(N)
        deq = w8.float() * scale[:, :, None]
        wb = deq.to(BF)
        assert torch.equal(wb.float(), deq)          # 4 significant bits times a power of two
        xin = (torch.randn(P, Kd, generator=g).to(BF) if down else x).to(gpu)
        _compare_with_bf16_tiles(gpu, r, xin, w8, scale, wb, "fp8", down, P,
                                 f"{'down' if down else 'gate|up'} H={H} I={I}")


@pytest.mark.parametrize("H,I", SHAPES)
def test_mxfp4_tiles_bit_equal_to_bf16_tiles_on_dequantised_weights(gpu, H, I):
    """Any nibbles, any block scales (here drawn directly, 2^-8 .. 2^3, so that they differ
    between the two 32-blocks of a k-step, between neighbouring rows and between experts): the
    widening is exact, so the MXFP4 tile kernel equals the bf16 tile kernel on
    ops.dequantize_mxfp4 of the same bytes, bit for bit."""
    g = torch.Generator().manual_seed(13 * H + I)
    ids = mc.explicit_ids()
    T = ids.shape[0]
    P = T * K
    x = torch.randn(T, H, generator=g).to(BF)
    tw = torch.rand(T, K, generator=g).to(BF).float()
    r = ops.moe_group(ids.to(gpu), tw.to(gpu), E)
    for down, (N, Kd) in _both_products(H, I):
        w4 = torch.randint(0, 256, (E, N, Kd // 2), generator=g, dtype=torch.int32).to(U8)
        bs = torch.randint(119, 131, (E, N, Kd // 32), generator=g, dtype=torch.int32).to(U8)
        bs[0, 0, 0], bs[0, 0, 1], bs[0, 1, 0], bs[1, 0, 0] = 120, 125, 129, 122
        assert bool((bs[:, :, 0::2] != bs[:, :, 1::2]).any())      # inside a k-step of 64
        assert bool((bs[:, 0::2] != bs[:, 1::2]).any())            # neighbouring rows
        wb = torch.stack([ops.dequantize_mxfp4(w4[e], bs[e]) for e in range(E)])
        assert wb.dtype == BF and bool(wb.float().isfinite().all())
        xin = (torch.randn(P, Kd, generator=g).to(BF) if down else x).to(gpu)
        _compare_with_bf16_tiles(gpu, r, xin, w4, bs, wb, "mxfp4", down, P,
                                 f"{'down' if down else 'gate|up'} H={H} I={I}")


# ------------------------------------------------------------------------------ general scales
_CASES = {}


def _gemm_case(fmt, H, I):
    """Inputs and the fp32 oracle of one (format, H, I), computed once: weights from
    ops.quantize_expert_weights_fp8 / _mxfp4; per pair, fp32 products of the bf16 rows with the
    dequantised weights, no intermediate rounding, one expert at a time."""
    if (fmt, H, I) not in _CASES:
        g = torch.Generator().manual_seed(H + I)
        ids = mc.explicit_ids()
        T = ids.shape[0]
        x = torch.randn(T, H, generator=g).to(BF)
        wg = (torch.randn(E, I, H, generator=g) / H ** 0.5).to(BF)
        wu = (torch.randn(E, I, H, generator=g) / H ** 0.5).to(BF)
        wd = (torch.randn(E, H, I, generator=g) / I ** 0.5).to(BF)
        w = torch.rand(T, K, generator=g).to(BF).float()
        wgu = torch.stack([ops.swiglu_interleave(torch.cat([wg[j], wu[j]], 0)) for j in range(E)])
        quant = (ops.quantize_expert_weights_fp8 if fmt == "fp8"
                 else ops.quantize_expert_weights_mxfp4)
        qgu, sgu = quant(wgu)
        qd, sd = quant(wd)
        dgu = torch.stack([ops.swiglu_deinterleave(m) for m in _dequant(fmt, qgu, sgu)])
        dd = _dequant(fmt, qd, sd)
        h = torch.zeros(T, K, I)
        y = torch.zeros(T, K, H)
        for e in range(E):
            t, s = (ids == e).nonzero(as_tuple=True)
            if t.numel() == 0:
                continue
            xe = x[t].float()
            he = torch.nn.functional.silu(xe @ dgu[e, :I].t()) * (xe @ dgu[e, I:].t())
            h[t, s] = he
            y[t, s] = he @ dd[e].t()
        _CASES[(fmt, H, I)] = dict(ids=ids, x=x, w=w, qgu=qgu, sgu=sgu, qd=qd, sd=sd, dd=dd,
                                   h=h.reshape(T * K, I), y=y.reshape(T * K, H))
    return _CASES[(fmt, H, I)]


def _run_both(c, fmt, gpu, tiles):
    """gate|up and down of case ``c`` into guarded outputs; returns (routing, h [P, I], y [P, H])."""
    T = c["ids"].shape[0]
    P = T * K
    I, H = c["h"].shape[1], c["y"].shape[1]
    kw = SCALE_KW[fmt]
    r = ops.moe_group(c["ids"].to(gpu), c["w"].to(gpu), E)
    with ops.kernel_policy(moe_tile_rows_q=64):
        hbuf, hview = _guarded_rows(P, I, gpu)
        h = ops.moe_grouped_gemm(c["x"].to(gpu), c["qgu"].to(gpu), r, out=hview, tiles=tiles,
                                 **{kw: c["sgu"].to(gpu)})
        torch.cuda.synchronize()
        _assert_guards(hbuf, P, "gate|up")
        ybuf, yview = _guarded_rows(P, H, gpu)
        y = ops.moe_grouped_gemm(h[:P].contiguous(), c["qd"].to(gpu), r, down=True, out=yview,
                                 tiles=tiles, **{kw: c["sd"].to(gpu)})
        torch.cuda.synchronize()
        _assert_guards(ybuf, P, "down")
    return r, h[:P], y[:P]


@pytest.mark.parametrize("H,I", SHAPES)
@pytest.mark.parametrize("fmt", FMTS)
def test_quantised_tiles_against_fp32_oracle_and_the_streaming_kernel(gpu, fmt, H, I):
    """Experts with 0, 1, 127, 128, 129, 300, 33 and 82 rows, general scales.  (256, 128): the
    down product has two k-steps; (1152, 384): 9 blocks of weight rows, three 256-row interleave
    groups, 18 / 6 k-steps.  Both kernels match the oracle and each other within the oracle
    tolerance (not bit for bit: the K summation order differs)."""
    c = _gemm_case(fmt, H, I)
    P = c["ids"].numel()
    r, ht, yt = _run_both(c, fmt, gpu, tiles=True)
    _, hs, ys = _run_both(c, fmt, gpu, tiles=False)
    assert r.expert_count.cpu().tolist() == list(mc.COUNTS)
    pairs = r.sorted_pairs.cpu().long()
    for name, h, y in (("tiles", ht, yt), ("streaming", hs, ys)):
        _close(h, c["h"][pairs], ATOL, RTOL, f"{fmt} {name} gate|up H={H} I={I}")
        _close(y, c["y"], ATOL, RTOL, f"{fmt} {name} down H={H} I={I}")
    _close(ht, hs, ATOL, RTOL, "gate|up tiles vs streaming")
    _close(yt, ys, ATOL, RTOL, "down tiles vs streaming")
    # ... and exactly the product of the rows the tile kernel read
    e_of_pair = c["ids"].reshape(-1).long()
    hp = torch.empty(P, I)
    hp[pairs] = ht.float().cpu()
    want = torch.empty(P, H)
    for e in range(E):
        want[e_of_pair == e] = hp[e_of_pair == e] @ c["dd"][e].t()
    _close(yt, want, ATOL, RTOL, "down/h")
    # on the same h rows the two down kernels differ by summation order only
    with ops.kernel_policy(moe_tile_rows_q=64):
        yt2 = ops.moe_grouped_gemm(hs.contiguous(), c["qd"].to(gpu), r, down=True, tiles=True,
                                   **{SCALE_KW[fmt]: c["sd"].to(gpu)})
    _close(yt2, ys, ATOL, RTOL, "down on equal h")
    assert float(yt.float().abs().max()) > 0.5


@pytest.mark.parametrize("fmt", FMTS)
def test_quantised_tiles_rows_are_independent(gpu, fmt):
    """A permutation of the tokens moves every pair to another row of another tile (and other
    pairs into the masked tails): each pair's gate|up and down results stay bit for bit."""
    c = _gemm_case(fmt, 256, 128)
    T = c["ids"].shape[0]
    perm = torch.randperm(T, generator=torch.Generator().manual_seed(9))
    assert not torch.equal(perm, torch.arange(T))
    c2 = dict(c, ids=c["ids"][perm].contiguous(), x=c["x"][perm].contiguous(), w=c["w"][perm])
    r1, h1, y1 = _run_both(c, fmt, gpu, tiles=True)
    r2, h2, y2 = _run_both(c2, fmt, gpu, tiles=True)
    assert not torch.equal(r1.sorted_pairs, r2.sorted_pairs)

    def by_pair(r, h):
        out = torch.empty_like(h)
        out[r.sorted_pairs.long()] = h
        return out.view(T, K, -1).cpu()

    hp1, hp2 = by_pair(r1, h1), by_pair(r2, h2)
    assert torch.equal(_bits(hp2), _bits(hp1[perm]))                 # token perm[t] is now t
    assert torch.equal(_bits(y2.view(T, K, -1).cpu()), _bits(y1.view(T, K, -1).cpu()[perm]))


def test_quantised_tiles_deterministic_and_host_checks(gpu):
    nat = ops.native()
    c8, c4 = _gemm_case("fp8", 256, 128), _gemm_case("mxfp4", 256, 128)
    r = ops.moe_group(c8["ids"].to(gpu), c8["w"].to(gpu), E)
    x = c8["x"].to(gpu)
    T = x.shape[0]
    w8, s8, d8, ds8 = (c8[n].to(gpu) for n in ("qgu", "sgu", "qd", "sd"))
    w4, s4, d4, ds4 = (c4[n].to(gpu) for n in ("qgu", "sgu", "qd", "sd"))
    tabs = (r.sorted_pairs, r.expert_count, r.expert_offset)
    with ops.kernel_policy(moe_tile_rows_q=64):
        for w, s, d, ds, kw in ((w8, s8, d8, ds8, "w_scale"), (w4, s4, d4, ds4, "w_block_scale")):
            a = ops.moe_grouped_gemm(x, w, r, tiles=True, **{kw: s})
            b = ops.moe_grouped_gemm(x, w, r, tiles=True, **{kw: s})
            assert torch.equal(_bits(a), _bits(b))
            ya = ops.moe_grouped_gemm(a, d, r, down=True, tiles=True, **{kw: ds})
            yb = ops.moe_grouped_gemm(a, d, r, down=True, tiles=True, **{kw: ds})
            assert torch.equal(_bits(ya), _bits(yb))
        # through the front end
        with pytest.raises(RuntimeError, match="K % 64"):
            ops.moe_grouped_gemm(x[:, :96].contiguous(), w8[:, :, :96].contiguous(), r,
                                 w_scale=s8, tiles=True)
        with pytest.raises(RuntimeError, match="N % 128"):
            ops.moe_grouped_gemm(x, w8[:, :192].contiguous(), r, w_scale=s8[:, :192].contiguous(),
                                 tiles=True)
        with pytest.raises(RuntimeError, match="N % 128"):
            ops.moe_grouped_gemm(x, w4[:, :192].contiguous(), r,
                                 w_block_scale=s4[:, :192].contiguous(), tiles=True)
        for w, s, kw in ((w8, s8, "w_scale"), (w4, s4, "w_block_scale")):
            with pytest.raises(RuntimeError, match="out"):
                ops.moe_grouped_gemm(x, w, r, out=torch.empty(799, 128, dtype=BF, device=gpu),
                                     tiles=True, **{kw: s})
    # the native entries themselves
    out = torch.empty(T * K, 128, dtype=BF, device=gpu)
    nat.moe_tile_gemm(out, x, w8, *tabs, T, K, 0, s8)
    nat.moe_tile_gemm(out, x, w4, *tabs, T, K, 0, s4)
    with pytest.raises(RuntimeError, match="w_scale"):                       # shape
        nat.moe_tile_gemm(out, x, w8, *tabs, T, K, 0, s8[:, :-1].contiguous())
    with pytest.raises(RuntimeError, match="w_scale"):
        nat.moe_tile_gemm(out, x, w8, *tabs, T, K, 0, s8.reshape(-1))
    with pytest.raises(RuntimeError, match="w_scale"):                       # dtype
        nat.moe_tile_gemm(out, x, w8, *tabs, T, K, 0, s8.to(BF))
    with pytest.raises(RuntimeError, match="fp8 e4m3fn"):
        nat.moe_tile_gemm(out, x, w8.view(U8), *tabs, T, K, 0, s8)
    with pytest.raises(RuntimeError, match="w_block_scale"):                 # shape
        nat.moe_tile_gemm(out, x, w4, *tabs, T, K, 0, s4[:, :, :-1].contiguous())
    with pytest.raises(RuntimeError, match="w_block_scale"):                 # dtype
        nat.moe_tile_gemm(out, x, w4, *tabs, T, K, 0, s4.to(torch.int8))
    with pytest.raises(RuntimeError, match="K % 64"):
        nat.moe_tile_gemm(out, x[:, :96].contiguous(), w8[:, :, :96].contiguous(), *tabs, T, K, 0,
                          s8)
    with pytest.raises(RuntimeError, match="K % 128"):                       # 192: two blocks short
        nat.moe_tile_gemm(out, x[:, :192].contiguous(), w4[:, :, :96].contiguous(), *tabs, T, K, 0,
                          s4[:, :, :6].contiguous())
    with pytest.raises(RuntimeError, match="N % 128"):
        nat.moe_tile_gemm(out, x, w8[:, :192].contiguous(), *tabs, T, K, 0,
                          s8[:, :192].contiguous())
    with pytest.raises(RuntimeError, match="out"):                           # too few rows
        nat.moe_tile_gemm(out[:799], x, w8, *tabs, T, K, 0, s8)
    with pytest.raises(RuntimeError, match="out"):
        nat.moe_tile_gemm(out[:799], x, w4, *tabs, T, K, 0, s4)
    with pytest.raises(RuntimeError):                                        # another device
        nat.moe_tile_gemm(out, x, w8.cpu(), *tabs, T, K, 0, s8)
    with pytest.raises(RuntimeError):
        nat.moe_tile_gemm(out, x, w4.cpu(), *tabs, T, K, 0, s4)
    with pytest.raises(RuntimeError):
        nat.moe_tile_gemm(out, x, w8, *tabs, T, K, 0, s8.cpu())
    with pytest.raises(RuntimeError):
        nat.moe_tile_gemm(out, x, w4, *tabs, T, K, 0, s4.cpu())
    # the policy at 0: as before
    assert ops.policy().moe_tile_rows_q == 0
    with pytest.raises(ValueError, match="tiles=True needs bf16 expert weights"):
        ops.moe_grouped_gemm(x, w8, r, w_scale=s8, tiles=True)
    with pytest.raises(RuntimeError, match="bf16 expert weights only"):
        nat.moe_tile_gemm(out, x, w8, *tabs, T, K, 0)
    torch.cuda.synchronize()


def test_tile_entry_rejects_a_scale_of_another_format_before_any_launch(gpu):
    """The one native entry infers the format from the weights' dtype: a scale that does not go
    with it is refused with the output untouched, and valid calls after that give the front
    end's bits."""
    T, k, E_, N, K_ = 4, 2, 2, 128, 128
    g = torch.Generator().manual_seed(11)
    h = torch.randn(T * k, K_, generator=g).to(BF).to(gpu)
    wb = (torch.randn(E_, N, K_, generator=g) / K_ ** 0.5).to(BF)
    ew = {fmt: ops.ExpertWeights(*(t if t is None else t.to(gpu)
                                   for t in ops.ExpertWeights.quantize(wb, fmt)))
          for fmt in ["bf16"] + FMTS}
    ids = torch.tensor([[0, 1], [1, 0], [0, 1], [1, 0]], dtype=torch.int32)
    r = ops.moe_group(ids.to(gpu), torch.full((T, k), 0.5).to(gpu), E_)
    nat = ops.native().moe_tile_gemm
    tabs = (r.sorted_pairs, r.expert_count, r.expert_offset, T, k, 1)
    (w8, s8), (w4, s4) = ew["fp8"], ew["mxfp4"]
    out = torch.full((T * k, N), SENT, dtype=BF, device=gpu)
    for w, s in ((ew["bf16"].w, s8),                          # bf16 weights with a scale
                 (w8, None),                                  # fp8 weights without one
                 (w8, s8.to(U8)),                             # ... with a uint8 scale
                 (w4, s4.float()),                            # nibbles with an fp32 scale
                 (w4, s4[:, :, :-1].contiguous()),            # [E, N, K / 32 - 1]
                 (w8, s8.cpu()), (w4, s4.cpu())):             # a scale on the CPU
        with pytest.raises(RuntimeError):
            nat(out, h, w, *tabs, s)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
    with ops.kernel_policy(moe_tile_rows_q=64):
        for fmt, (w, s) in ew.items():
            nat(out, h, w, *tabs, s)
            want = ops.moe_grouped_gemm(h, ew[fmt], r, down=True, tiles=True)
            assert torch.equal(_bits(out), _bits(want)), fmt
            assert float(want.float().abs().max()) > 0.01


# ------------------------------------------------------------------------------------- the block
def _moe_spec(E_, k):
    return ModelSpec(name="moe-t", model_type="qwen3_moe", qk_norm=True, vocab_size=512,
                     hidden_size=256, intermediate_size=512, num_layers=2, num_heads=2,
                     num_kv_heads=1, head_dim=128, rms_norm_eps=1e-6, rope_theta=10000.0,
                     max_position_embeddings=4096, bos_token_id=1, eos_token_id=2, num_experts=E_,
                     num_experts_per_tok=k, moe_intermediate_size=128, norm_topk_prob=True)


SHARED = 384


def _shared_spec(E_, k):
    return ModelSpec(name="q2moe-t", model_type="qwen2_moe", vocab_size=512, hidden_size=256,
                     intermediate_size=512, num_layers=2, num_heads=2, num_kv_heads=1,
                     head_dim=128, rms_norm_eps=1e-6, rope_theta=10000.0,
                     max_position_embeddings=4096, bos_token_id=1, eos_token_id=2,
                     attention_bias=True, o_proj_bias=False, num_experts=E_,
                     num_experts_per_tok=k, moe_intermediate_size=128,
                     shared_expert_intermediate_size=SHARED, norm_topk_prob=False,
                     decoder_sparse_step=1)


_BLOCKS = {}


def _block_case(fmt, E_, k, rows, shared=False):
    """tests/test_moe_tile_gpu.py's block fixture with quantised experts: a CPU MoEMLP with weights
    of unit-scale products (``shared``: Qwen2-MoE's, with a shared expert and its gate row),
    quantised by the block's own method, its CPU output on the first ``rows`` rows, and rows
    whose CPU fp32 router logits have their k-th and (k+1)-th largest >= 1/16 apart with every
    |logit| < 4, so bf16 logit rounding cannot change the routing of any of them."""
    key = (fmt, E_, k, shared)
    if key not in _BLOCKS:
        g = torch.Generator().manual_seed(17 * E_ + k)
        mlp = MoEMLP(_shared_spec(E_, k) if shared else _moe_spec(E_, k))
        H, I = 256, 128
        with torch.no_grad():
            mlp.gate.weight.copy_((torch.randn(E_ + int(shared), H, generator=g) / H ** 0.5).to(BF))
            mlp.w_gate_up.copy_((torch.randn(E_, 2 * I, H, generator=g) / H ** 0.5).to(BF))
            mlp.w_down.copy_((torch.randn(E_, H, I, generator=g) / I ** 0.5).to(BF))
            if shared:
                sh = mlp.shared_expert
                sh.gate_up_proj.weight.copy_(
                    (torch.randn(2 * SHARED, H, generator=g) / H ** 0.5).to(BF))
                sh.down_proj.weight.copy_(
                    (torch.randn(H, SHARED, generator=g) / SHARED ** 0.5).to(BF))
        if fmt == "fp8":
            mlp.quantize_experts_fp8()
        else:
            mlp.quantize_experts_mxfp4()
        cand = torch.randn(6000, H, generator=g).to(BF)
        lf = cand.float() @ mlp.gate.weight.float().t()
        top = lf[:, :E_].sort(-1, descending=True).values
        ok = ((top[:, k - 1] - top[:, k]) >= 1 / 16) & (lf.abs().max(-1).values < 4)
        _BLOCKS[key] = [mlp, cand[ok].contiguous(), {}]
    mlp, x, wants = _BLOCKS[key]
    assert x.shape[0] >= rows, x.shape
    x = x[:rows].contiguous()
    if rows not in wants:
        with torch.no_grad():
            wants[rows] = mlp(x)
    return mlp, x, wants[rows]


def _on_gpu(mlp, fmt, gpu):
    gm = copy.deepcopy(mlp).to(gpu)
    assert gm.is_fp8 if fmt == "fp8" else gm.is_mxfp4
    assert gm.w_gate_up.is_cuda and gm.w_gate_up.dtype == (FP8 if fmt == "fp8" else U8)
    assert gm.gate.weight.dtype == BF
    return gm


def _spy(monkeypatch):
    """Counts the native tile launches per weight format (their epilogues), and lets them
    through."""
    nat = ops.native()
    calls = {"bf16": [], "fp8": [], "mxfp4": []}
    fmt_of = {BF: "bf16", FP8: "fp8", U8: "mxfp4"}

    def spy(*a, real=nat.moe_tile_gemm):
        calls[fmt_of[a[2].dtype]].append(int(a[8]))
        return real(*a)

    monkeypatch.setattr(nat, "moe_tile_gemm", spy)
    return calls


def _check_block(gpu, monkeypatch, fmt, E_, k, T, shared):
    mlp, x, want = _block_case(fmt, E_, k, T, shared)
    gm = _on_gpu(mlp, fmt, gpu)
    xg = x.to(gpu)
    calls = _spy(monkeypatch)
    other = "mxfp4" if fmt == "fp8" else "fp8"
    with ops.kernel_policy(moe_tile_rows_q=64), torch.no_grad():
        assert ops.moe_uses_tiles(T, k, E_, fmt, xg.device)
        got = gm(xg)
        torch.cuda.synchronize()
        assert calls[fmt] == [0, 1]                  # gate|up, then down, on the format's entry
        assert calls[other] == [] and calls["bf16"] == []
        _close(got, want, ATOL, RTOL, f"{fmt} MoE block E={E_} k={k} T={T} shared={shared}")
        assert got.dtype == BF and got.shape == (T, 256) and want.float().abs().max() > 0.1
        # a few rows: below the threshold, the weight-streaming kernel as before
        del calls[fmt][:]
        small = gm(xg[:4].contiguous())
    with torch.no_grad():
        base = gm(xg[:4].contiguous())
        off = gm(xg)
    torch.cuda.synchronize()
    assert calls == {"bf16": [], "fp8": [], "mxfp4": []}
    assert torch.equal(_bits(small), _bits(base))
    _close(off, want, ATOL, RTOL, "policy 0")


@pytest.mark.parametrize("E_,k,T", [(8, 2, 300), (128, 8, 1100)])
@pytest.mark.parametrize("fmt", FMTS)
def test_quantised_moe_block_under_the_policy_matches_cpu_path(gpu, monkeypatch, fmt, E_, k, T):
    _check_block(gpu, monkeypatch, fmt, E_, k, T, shared=False)


def test_qwen2_moe_block_with_fp8_experts_under_the_policy(gpu, monkeypatch):
    """The shared expert stays bf16 on the dense kernels; the routed fp8 experts take the tiles."""
    _check_block(gpu, monkeypatch, "fp8", 8, 2, 300, shared=True)


@pytest.mark.parametrize("fmt", FMTS)
def test_quantised_moe_block_graph_replay_follows_the_routing(gpu, fmt):
    """Captured once under the policy with static buffers; replayed on three inputs that route
    differently: every replay is bit-equal to the eager call (the tiles come from counts in
    device memory)."""
    T = 300
    mlp, x, _ = _block_case(fmt, 8, 2, 3 * T)
    gm = _on_gpu(mlp, fmt, gpu)
    inputs = [x[i * T:(i + 1) * T].to(gpu) for i in range(3)]
    with ops.kernel_policy(moe_tile_rows_q=64), torch.no_grad():
        assert ops.moe_uses_tiles(T, 2, 8, fmt, inputs[0].device)
        eager = [gm(v).clone() for v in inputs]
        routes = [ops.moe_route(gm.gate(v), 2, True).expert_count.cpu() for v in inputs]
        assert not torch.equal(routes[0], routes[1]) and not torch.equal(routes[1], routes[2])
        assert not torch.equal(routes[0], routes[2])
        static_x = inputs[2].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                gm(static_x)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_y = gm(static_x)
    for v, want in zip(inputs, eager):          # the captured choice holds outside the policy
        static_x.copy_(v)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(static_y), _bits(want))


# ------------------------------------------------------------------------------------- engine
def _engine(graphs):
    cfg = EngineConfig(model="moe-t", pp=1, seed=5, quantize="fp8_experts",
                       kernels=KernelPolicy(moe_tile_rows_q=64),
                       cache=CacheConfig(num_blocks=128, block_size=64, max_chunk=512),
                       serve=ServeConfig(max_batch_size=4, max_num_batched_tokens=512,
                                         max_seq_len=512, use_graphs=graphs,
                                         graph_batch_sizes=[1, 2, 4]))
    return LLMEngine(_moe_spec(8, 2), device="cuda:0", cfg=cfg)


def test_fp8_experts_engine_under_the_policy_graph_decode_equals_eager(gpu, monkeypatch):
    """A 300-token prompt: its prefill chunk has 600 pairs over 8 experts, past the threshold of
    64 rows per expert, so the prefill runs on the fp8 tile kernel; decode rows stay below it."""
    prompts = [[3 + (7 * i) % 500 for i in range(300)], [7, 8, 9], [11]]
    p = SamplingParams(max_tokens=8, ignore_eos=True)
    calls = _spy(monkeypatch)
    eng = _engine(graphs=False)
    assert ops.policy().moe_tile_rows_q == 64 and ops.policy().moe_tile_rows == 0
    for l in eng.executors[0].stage.block.layers:
        assert isinstance(l.mlp, MoEMLP) and l.mlp.is_fp8
    before = len(calls["fp8"])
    a = [s.output for s in eng.generate(prompts, p)]
    assert calls["fp8"][before:before + 4] == [0, 1, 0, 1]     # two layers x (gate|up, down)
    assert calls["bf16"] == [] and calls["mxfp4"] == []
    b = [s.output for s in _engine(graphs=True).generate(prompts, p)]
    assert all(len(o) == 8 for o in a) and a == b
