"""The grouped block-scaled MFMA tile GEMM for MXFP4 experts on MX fp8 activations
(csrc/kernels/moe_tile_scaled.hip) and its row-major quantiser, on the GPU: the quantiser bit for bit
against ops.mx_quantize, both products bit for bit against fp64 on exactly-summable operands with
row counts on every edge of the 128-row tiling, random data against fp64 on the quantise-
dequantised operands, row independence, the MoE block under ``KernelPolicy.moe_tile_mx`` (eager
and in a captured graph) and the host checks."""
import copy

import pytest
import torch

import moe_tile_cases as mc
from moe_tile_cases import (bits as _bits, guarded as _guarded, products as _products,
                            routing as _routing, swiglu64 as _swiglu64)
from distributed_llm_inference import ops
from distributed_llm_inference.config import ModelSpec
from distributed_llm_inference.models.llama.modules import MoEMLP

pytestmark = pytest.mark.gpu
BF, FP8, U8 = torch.bfloat16, torch.float8_e4m3fn, torch.uint8
SENT = mc.SENT
E, K = mc.E, mc.K_TOP
SHAPES = [(256, 128), (1152, 384)]
ATOL, RTOL = mc.ATOL, mc.RTOL   # tests/test_moe_tile_q_gpu.py's oracle tolerance for the epilogues
BOUND = 2e-2                # test_gemm_fp4_random_against_fp32_oracle's, of the largest magnitude


# ----------------------------------------------------------------------------------- quantiser
@pytest.mark.parametrize("Kd", [128, 384])
@pytest.mark.parametrize("R", [1, 65, 130])
def test_quant_mx_rows_bit_exact_against_mx_quantize(gpu, R, Kd):
    g = torch.Generator().manual_seed(R + Kd)
    x = torch.randn(R, Kd, generator=g) * torch.exp2(torch.randint(-6, 7, (R, 1), generator=g))
    blk = x.view(-1, 128)                        # specials, as many as the blocks can hold
    n = blk.shape[0]
    if n > 1:
        blk[0] = 0.0                             # an all-zero block: scale byte 127
    if n > 2:
        blk[n // 2] = blk[n // 2].clamp(-100, 100)
        blk[n // 2, 5] = 448.0 * 8               # amax an exact power of two times 448
    blk[n - 1] = blk[n - 1].clamp(-100, 100)
    blk[n - 1, 77] = -3600.0                     # ... and one just above it (bf16-exact)
    x = x.to(BF)
    want = ops.mx_quantize(x)
    qb = torch.full((R * Kd + 64,), 0xAB, dtype=U8, device=gpu)
    sb = torch.full((R * Kd // 128 + 64,), 0xAB, dtype=U8, device=gpu)
    ops.native().quant_mx_rows(qb[:R * Kd].view(R, Kd), sb[:R * Kd // 128].view(R, -1), x.to(gpu))
    torch.cuda.synchronize()
    assert torch.equal(qb[:R * Kd].view(R, Kd).cpu(), want.q.view(U8))
    assert torch.equal(sb[:R * Kd // 128].view(R, -1).cpu().int() - 127, want.exponents())
    assert bool((qb[R * Kd:] == 0xAB).all()) and bool((sb[R * Kd // 128:] == 0xAB).all())
    got = ops.quant_mx_rows(x.to(gpu))
    assert torch.equal(got.q.view(U8).cpu(), want.q.view(U8))
    assert torch.equal(got.dequantize().cpu(), want.dequantize())


# ------------------------------------------------------------------------------ exact operands
def _exact_operands(R, N, Kd, lo, seed):
    """MXFP4 experts [E, N, Kd] with all 16 nibble codes and scale bytes lo .. lo + 2 differing
    per (expert, row, 32-block); activations integers in [-4, 4] as e4m3 with exponents 0 / 1
    differing per (row, 128-block).  Every product is a multiple of q = 2^(lo - 128) and the sum
    of magnitudes stays below 2^23 q, so any fp32 summation order is exact (asserted)."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randint(0, 256, (E, N, Kd // 2), generator=g, dtype=U8)
    w[:, 0, :8] = torch.tensor([0x10, 0x32, 0x54, 0x76, 0x98, 0xBA, 0xDC, 0xFE], dtype=U8)
    s = torch.randint(lo, lo + 3, (E, N, Kd // 32), generator=g, dtype=U8)
    xi = torch.randint(-4, 5, (R, Kd), generator=g).float()
    ex = torch.randint(0, 2, (R, Kd // 128), generator=g)
    a = ops.MxFp8Rows(xi.to(FP8), (ex + 127).to(U8))
    wd = torch.stack([ops.dequantize_mxfp4(w[e], s[e]) for e in range(E)]).double()
    ad = a.dequantize().double()
    q = 2.0 ** (lo - 128)
    assert torch.cat([w & 15, w >> 4]).unique().numel() == 16 and s.unique().numel() == 3
    assert not torch.equal(s[0], s[1]) and not torch.equal(s[:, 0], s[:, 1])
    assert not torch.equal(s[..., 0], s[..., 1]) and ex[:, 0].unique().numel() == 2
    assert Kd == 128 or not torch.equal(ex[:, 0], ex[:, 1])
    assert torch.equal(ad, xi.double() * torch.exp2(ex.double()).repeat_interleave(128, dim=1))
    assert float(wd.abs().max()) <= 12 * 2.0 ** (lo - 126) and float(ad.abs().max()) <= 8
    assert torch.equal(wd / q, (wd / q).round()) and torch.equal(ad, ad.round())
    assert max(float((ad.abs() @ wd[e].abs().t()).max()) for e in range(E)) / q < 2 ** 23
    return a, ops.ExpertWeights(w, s), ad, wd


def _to(a, w, gpu):
    return (ops.MxFp8Rows(a.q.to(gpu), a.sc.to(gpu)), ops.ExpertWeights(w.w.to(gpu), w.scale.to(gpu)))


@pytest.mark.parametrize("H,I", SHAPES)
def test_layout_bit_exact_against_fp64(gpu, H, I):
    ids, r, pairs = _routing(gpu)
    T, P = ids.shape[0], ids.numel()
    e_row = ids.reshape(-1).long()[pairs]        # the expert of sorted row j
    with ops.kernel_policy(moe_tile_rows_q=32):
        # down: h rows in sorted order, K = I; scale bytes 126 .. 128 (|w| <= 12)
        a, w, ad, wd = _exact_operands(P, H, I, 126, H + I)
        ag, wg = _to(a, w, gpu)
        y = _guarded(lambda o: ops.moe_grouped_gemm(ag, wg, r, down=True, out=o, mx=True), P, H, gpu)
        want = torch.empty(P, H, dtype=BF)
        want[pairs] = _products(ad, wd, e_row).float().to(BF)
        assert torch.equal(_bits(y), _bits(want)), (y.float() - want.float()).abs().max()
        # gate|up: x per token, K = H; scale bytes 119 .. 121 keep the gate inside silu's bend
        a, w, ad, wd = _exact_operands(T, 2 * I, H, 119, H - I)
        ag, wg = _to(a, w, gpu)
        h = _guarded(lambda o: ops.moe_grouped_gemm(ag, wg, r, out=o, mx=True), P, I, gpu)
        hb = ops.moe_grouped_gemm(ad.to(BF).to(gpu), wd.to(BF).to(gpu), r, tiles=True).cpu()
    gu = _products(ad[pairs // K], wd, e_row).float().to(BF).double()
    assert 0.25 < float(gu.abs().median()) < 8, "gate values outside silu's bend"
    assert torch.equal(_bits(h), _bits(hb)), (h.float() - hb.float()).abs().max()
    want = _swiglu64(gu)
    assert bool(((h.double() - want).abs() <= ATOL + RTOL * want.abs()).all())


# ----------------------------------------------------------------------------------- random data
def _random_case(H, I, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(mc.explicit_ids().shape[0], H, generator=g).to(BF)
    gu = ops.ExpertWeights.quantize((torch.randn(E, 2 * I, H, generator=g) / H ** 0.5).to(BF), "mxfp4")
    dn = ops.ExpertWeights.quantize((torch.randn(E, H, I, generator=g) / I ** 0.5).to(BF), "mxfp4")
    return x, gu, dn


def _run(gpu, x, gu, dn, r):
    with ops.kernel_policy(moe_tile_rows_q=32):
        h = ops.moe_grouped_gemm(x.to(gpu), ops.ExpertWeights(*(t.to(gpu) for t in gu)), r, mx=True)
        y = ops.moe_grouped_gemm(h, ops.ExpertWeights(*(t.to(gpu) for t in dn)), r, down=True, mx=True)
    return h.cpu(), y.cpu()


@pytest.mark.parametrize("H,I", SHAPES)
def test_random_against_fp64_on_quantise_dequantised_operands(gpu, H, I):
    ids, r, pairs = _routing(gpu)
    e_row = ids.reshape(-1).long()[pairs]
    x, gu, dn = _random_case(H, I, H)
    h, y = _run(gpu, x, gu, dn, r)
    wd = lambda w: torch.stack([w.dequantize(e) for e in range(E)]).double()
    xd = ops.quant_mx_rows(x).dequantize().double()[pairs // K]
    want_h = _swiglu64(_products(xd, wd(gu), e_row))
    want_y = torch.empty(ids.numel(), H, dtype=torch.float64)
    want_y[pairs] = _products(ops.quant_mx_rows(h).dequantize().double(), wd(dn), e_row)
    for got, want in ((h, want_h), (y, want_y)):
        err, top = float((got.double() - want).abs().max()), float(want.abs().max())
        print(f"H={H} I={I}: max err {err:.4g} of {top:.4g}")
        assert top > 0.5 and err < BOUND * top


def test_rows_are_independent_and_launch_is_deterministic(gpu):
    H, I = 256, 128
    ids, r, pairs = _routing(gpu)
    T = ids.shape[0]
    x, gu, dn = _random_case(H, I, 5)
    h, y = _run(gpu, x, gu, dn, r)
    h2, y2 = _run(gpu, x, gu, dn, r)
    assert torch.equal(_bits(h), _bits(h2)) and torch.equal(_bits(y), _bits(y2))
    perm = torch.randperm(T, generator=torch.Generator().manual_seed(9))
    _, rp, pairs_p = _routing(gpu, ids[perm])
    hp, yp = _run(gpu, x[perm], gu, dn, rp)
    by_pair = lambda h_, p_: torch.empty_like(h_).index_copy_(0, p_, h_).view(T, K, -1)
    assert torch.equal(_bits(by_pair(hp, pairs_p)), _bits(by_pair(h, pairs)[perm]))
    assert torch.equal(_bits(yp.view(T, K, H)), _bits(y.view(T, K, H)[perm]))


# ------------------------------------------------------------------------------------- the block
def _block(gpu):
    spec = ModelSpec(name="moe-t", model_type="qwen3_moe", qk_norm=True, vocab_size=512,
                     hidden_size=256, intermediate_size=512, num_layers=2, num_heads=2,
                     num_kv_heads=1, head_dim=128, rms_norm_eps=1e-6, rope_theta=10000.0,
                     max_position_embeddings=4096, bos_token_id=1, eos_token_id=2, num_experts=E,
                     num_experts_per_tok=K, moe_intermediate_size=128, norm_topk_prob=True)
    g = torch.Generator().manual_seed(23)
    mlp = MoEMLP(spec)
    with torch.no_grad():
        mlp.gate.weight.copy_((torch.randn(E, 256, generator=g) / 16).to(BF))
        mlp.w_gate_up.copy_((torch.randn(E, 256, 256, generator=g) / 16).to(BF))
        mlp.w_down.copy_((torch.randn(E, 256, 128, generator=g) / 128 ** 0.5).to(BF))
    mlp.quantize_experts_mxfp4()
    return mlp, copy.deepcopy(mlp).to(gpu), torch.randn(900, 256, generator=g).to(BF)


def _spy(monkeypatch):
    nat, calls = ops.native(), {"mx": [], "tile": []}
    monkeypatch.setattr(nat, "moe_tile_gemm_mx",
                        lambda *a, real=nat.moe_tile_gemm_mx: (calls["mx"].append(int(a[9])), real(*a))[1])
    monkeypatch.setattr(nat, "moe_tile_gemm",
                        lambda *a, real=nat.moe_tile_gemm: (calls["tile"].append(int(a[8])), real(*a))[1])
    return calls


def test_block_under_the_policy(gpu, monkeypatch):
    mlp, gm, x = _block(gpu)
    xg, calls = x[:300].to(gpu), _spy(monkeypatch)
    with torch.no_grad(), ops.kernel_policy(moe_tile_rows_q=32, moe_tile_mx=True):
        assert ops.moe_uses_mx(300, K, E, "mxfp4", xg.device)
        got = gm(xg).cpu()
        assert calls == {"mx": [0, 1], "tile": []}
        # the CPU path with mx=True, on the GPU's routing (bf16 logit ties cannot differ)
        rg = ops.moe_route(gm.gate(xg), K, True)
        r = ops.moe_group(rg.topk_ids.cpu(), rg.topk_w.cpu(), E)
        h = ops.moe_grouped_gemm(x[:300], mlp.experts("w_gate_up"), r, mx=True)
        y = ops.moe_grouped_gemm(h, mlp.experts("w_down"), r, down=True, mx=True)
        want = ops.moe_combine(y, r.topk_w).float()
    assert float((got.float() - want).abs().max()) < BOUND * float(want.abs().max()) > 0
    del calls["mx"][:]
    with torch.no_grad(), ops.kernel_policy(moe_tile_rows_q=32, moe_tile_mx=False):
        off = gm(xg)
    with torch.no_grad(), ops.kernel_policy(moe_tile_rows_q=32):
        base = gm(xg)
    assert calls == {"mx": [], "tile": [0, 1, 0, 1]} and torch.equal(_bits(off), _bits(base))


def test_block_graph_replay_follows_the_routing(gpu):
    _, gm, x = _block(gpu)
    inputs = [x[300 * i:300 * (i + 1)].to(gpu) for i in range(3)]
    with torch.no_grad(), ops.kernel_policy(moe_tile_rows_q=32, moe_tile_mx=True):
        eager = [gm(v).clone() for v in inputs]
        counts = [ops.moe_route(gm.gate(v), K, True).expert_count.tolist() for v in inputs]
        assert counts[0] != counts[1] != counts[2] != counts[0]
        static_x = inputs[2].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            gm(static_x)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_y = gm(static_x)
    for v, want in zip(inputs, eager):
        static_x.copy_(v)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(static_y), _bits(want))


# ----------------------------------------------------------------------------------- host checks
def test_host_checks_reject_before_any_launch(gpu):
    ids, r, _ = _routing(gpu)
    T, P = ids.shape[0], ids.numel()
    x, gu, _ = _random_case(256, 128, 1)
    a = ops.quant_mx_rows(x.to(gpu))
    w, s = gu.w.to(gpu), gu.scale.to(gpu)
    out = torch.full((P, 128), SENT, dtype=BF, device=gpu)
    nat = lambda a_sc, w_, s_: ops.native().moe_tile_gemm_mx(
        out, a.q, a_sc, w_, r.sorted_pairs, r.expert_count, r.expert_offset, T, K, 0, s_)
    wb = torch.zeros(E, 256, 256, dtype=BF, device=gpu)
    bad = [lambda: nat(a.sc, wb, None),                                     # bf16 experts
           lambda: nat(a.sc, wb.to(FP8), torch.ones(E, 256, device=gpu)),   # fp8 experts
           lambda: nat(a.sc, w[:, :192].contiguous(), s[:, :192].contiguous()),       # N % 128
           lambda: nat(a.sc, w[:, :, :96].contiguous(), s[:, :, :6].contiguous()),    # K % 128
           lambda: nat(torch.cat([a.sc, a.sc], 1), w, s),                   # scale shape
           lambda: nat(a.sc.int(), w, s),                                   # scale dtype
           lambda: nat(a.sc.cpu(), w, s)]                                   # scale device
    with ops.kernel_policy(moe_tile_rows_q=32):
        bad += [lambda: ops.moe_grouped_gemm(x.to(gpu), wb, r, out=out, mx=True),
                lambda: ops.moe_grouped_gemm(x.to(gpu), ops.ExpertWeights(w[:, :192].contiguous(),
                                             s[:, :192].contiguous()), r, out=out, mx=True)]
        for f in bad:
            with pytest.raises((RuntimeError, ValueError)):
                f()
    with pytest.raises(ValueError, match="moe_tile_rows_q"):     # the policy field at 0
        ops.moe_grouped_gemm(a, ops.ExpertWeights(w, s), r, out=out, mx=True)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
