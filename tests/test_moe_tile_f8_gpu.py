"""The grouped block-scaled MFMA tile GEMM for fp8 experts on MX fp8 activations
(csrc/kernels/moe_tile_scaled.hip) on the GPU: both products bit for bit against fp64 and against the
widening fp8 tile kernel on exactly-summable operands with row counts on every edge of the 128-row
tiling, random data against fp64 on the quantise-dequantised operands, row independence, the MoE
block under ``KernelPolicy.moe_tile_f8`` (eager and in a captured graph) and the host checks."""
import copy

import pytest
import torch

import moe_tile_cases as mc
from moe_tile_cases import (bits as _bits, close as _close, guarded as _guarded,
                            products as _products, routing as _routing, swiglu64 as _swiglu64)
from distributed_llm_inference import ops
from distributed_llm_inference.config import ModelSpec
from distributed_llm_inference.models.llama.modules import MoEMLP

pytestmark = pytest.mark.gpu
BF, FP8, U8 = torch.bfloat16, torch.float8_e4m3fn, torch.uint8
SENT = mc.SENT
E, K = mc.E, mc.K_TOP
SHAPES = [(256, 128), (1152, 384)]


def _to(w, gpu):
    return ops.ExpertWeights(w.w.to(gpu), w.scale.to(gpu))


# ------------------------------------------------------------------------------ exact operands
def _exact_operands(R, N, Kd, lo, top, seed):
    """fp8 experts [E, N, Kd] from every e4m3 code with exponent field lo .. lo + 2 (both signs,
    all 8 mantissas); row scales in [top / 2, top), no power of two, differing per (expert, row);
    activations integers in [-4, 4] as e4m3 with exponents 0 / 1 differing per (row, 128-block).
    Every product is a multiple of q = 2^(lo - 10) and the sum of magnitudes stays below 2^23 q,
    so any fp32 summation order is exact (asserted)."""
    g = torch.Generator().manual_seed(seed)
    code = torch.randint(0, 48, (E, N, Kd), generator=g)
    code[0, 0, :48] = torch.arange(48)
    w = (((code // 24) << 7) | ((lo + code % 24 // 8) << 3) | (code % 8)).to(U8).view(FP8)
    s = (top * (0.5 + 0.5 * torch.rand(E, N, generator=g))).float()
    xi = torch.randint(-4, 5, (R, Kd), generator=g).float()
    ex = torch.randint(0, 2, (R, Kd // 128), generator=g)
    a = ops.MxFp8Rows(xi.to(FP8), (ex + 127).to(U8))
    wd, ad, q = w.float().double(), a.dequantize().double(), 2.0 ** (lo - 10)
    assert w.view(U8).unique().numel() == 48
    assert not torch.equal(s[0], s[1]) and not torch.equal(s[:, 0], s[:, 1])
    assert bool((torch.frexp(s).mantissa != 0.5).all()) and ex[:, 0].unique().numel() == 2
    assert Kd == 128 or not torch.equal(ex[:, 0], ex[:, 1])
    assert torch.equal(ad, xi.double() * torch.exp2(ex.double()).repeat_interleave(128, dim=1))
    assert float(wd.abs().min()) == 8 * q and float(wd.abs().max()) == 60 * q
    assert torch.equal(wd / q, (wd / q).round()) and float(ad.abs().max()) <= 8
    assert max(float((ad.abs() @ wd[e].abs().t()).max()) for e in range(E)) / q < 2 ** 23
    return a, ops.ExpertWeights(w, s), ad, wd


@pytest.mark.parametrize("H,I", SHAPES)
def test_layout_bit_exact_against_fp64_and_the_widening_kernel(gpu, H, I):
    ids, r, pairs = _routing(gpu)
    T, P = ids.shape[0], ids.numel()
    e_row = ids.reshape(-1).long()[pairs]        # the expert of sorted row j
    scaled = lambda s64, w: s64.float() * w.scale[e_row]      # fp32(exact sum) * scale, one rounding
    with ops.kernel_policy(moe_tile_rows_q=32):
        # down: h rows in sorted order, K = I
        a, w, ad, wd = _exact_operands(P, H, I, 6, 1.0, H + I)
        ag, wg = ops.MxFp8Rows(a.q.to(gpu), a.sc.to(gpu)), _to(w, gpu)
        y = _guarded(lambda o: ops.moe_grouped_gemm(ag, wg, r, down=True, out=o, mx=True), P, H, gpu)
        yw = ops.moe_grouped_gemm(ad.to(BF).to(gpu), wg, r, down=True, tiles=True).cpu()
        want = torch.empty(P, H, dtype=BF)
        want[pairs] = scaled(_products(ad, wd, e_row), w).to(BF)
        assert torch.equal(_bits(y), _bits(want)), (y.float() - want.float()).abs().max()
        assert torch.equal(_bits(y), _bits(yw))
        # gate|up: x per token, K = H.  |w| <= 7.5 and |x| <= 8 with second moments of about 15
        # and 17 give sums of deviation 16 sqrt(K); scales of 1 / (8 sqrt(K)) .. twice that bring
        # the gate to a deviation of about 3: inside silu's bend
        a, w, ad, wd = _exact_operands(T, 2 * I, H, 7, 0.25 / H ** 0.5, H - I)
        ag, wg = ops.MxFp8Rows(a.q.to(gpu), a.sc.to(gpu)), _to(w, gpu)
        h = _guarded(lambda o: ops.moe_grouped_gemm(ag, wg, r, out=o, mx=True), P, I, gpu)
        hw = ops.moe_grouped_gemm(ad.to(BF).to(gpu), wg, r, tiles=True).cpu()
    gu = scaled(_products(ad[pairs // K], wd, e_row), w).to(BF).double()
    assert 0.25 < float(gu.abs().median()) < 8, "gate values outside silu's bend"
    assert torch.equal(_bits(h), _bits(hw)), (h.float() - hw.float()).abs().max()
    assert _close(h, _swiglu64(gu))


# ----------------------------------------------------------------------------------- random data
def _random_case(H, I, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(mc.explicit_ids().shape[0], H, generator=g).to(BF)
    gu = ops.ExpertWeights.quantize((torch.randn(E, 2 * I, H, generator=g) / H ** 0.5).to(BF), "fp8")
    dn = ops.ExpertWeights.quantize((torch.randn(E, H, I, generator=g) / I ** 0.5).to(BF), "fp8")
    return x, gu, dn


def _run(gpu, x, gu, dn, r):
    with ops.kernel_policy(moe_tile_rows_q=32):
        h = ops.moe_grouped_gemm(x.to(gpu), _to(gu, gpu), r, mx=True)
        y = ops.moe_grouped_gemm(h, _to(dn, gpu), r, down=True, mx=True)
    return h.cpu(), y.cpu()


@pytest.mark.parametrize("H,I", SHAPES)
def test_random_against_fp64_on_quantise_dequantised_operands(gpu, H, I):
    ids, r, pairs = _routing(gpu)
    e_row = ids.reshape(-1).long()[pairs]
    x, gu, dn = _random_case(H, I, H)
    h, y = _run(gpu, x, gu, dn, r)
    wd = lambda w: w.w.float().double() * w.scale.double()[:, :, None]
    xd = ops.quant_mx_rows(x).dequantize().double()[pairs // K]
    want_h = _swiglu64(_products(xd, wd(gu), e_row))
    want_y = torch.empty(ids.numel(), H, dtype=torch.float64)
    want_y[pairs] = _products(ops.quant_mx_rows(h).dequantize().double(), wd(dn), e_row)
    for got, want in ((h, want_h), (y, want_y)):
        assert float(want.abs().max()) > 0.5 and _close(got, want)


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
    mlp.quantize_experts_fp8()
    return mlp, copy.deepcopy(mlp).to(gpu), torch.randn(900, 256, generator=g).to(BF)


def test_block_under_the_policy(gpu, monkeypatch):
    mlp, gm, x = _block(gpu)
    xg, nat, calls = x[:300].to(gpu), ops.native(), {"f8": [], "tile": []}
    monkeypatch.setattr(nat, "moe_tile_gemm_f8",
                        lambda *a, real=nat.moe_tile_gemm_f8: (calls["f8"].append(int(a[9])), real(*a))[1])
    monkeypatch.setattr(nat, "moe_tile_gemm",
                        lambda *a, real=nat.moe_tile_gemm: (calls["tile"].append(int(a[8])), real(*a))[1])
    with torch.no_grad(), ops.kernel_policy(moe_tile_rows_q=32, moe_tile_f8=True):
        assert ops.moe_uses_f8(300, K, E, "fp8", xg.device)
        got = gm(xg).cpu()
        assert calls == {"f8": [0, 1], "tile": []}
        # the CPU path with mx=True, on the GPU's routing (bf16 logit ties cannot differ)
        rg = ops.moe_route(gm.gate(xg), K, True)
        r = ops.moe_group(rg.topk_ids.cpu(), rg.topk_w.cpu(), E)
        h = ops.moe_grouped_gemm(x[:300], mlp.experts("w_gate_up"), r, mx=True)
        y = ops.moe_grouped_gemm(h, mlp.experts("w_down"), r, down=True, mx=True)
        want = ops.moe_combine(y, r.topk_w)
    assert float(want.abs().max()) > 0.5 and _close(got, want)
    del calls["f8"][:]
    with torch.no_grad(), ops.kernel_policy(moe_tile_rows_q=32, moe_tile_f8=False):
        off = gm(xg)
    with torch.no_grad(), ops.kernel_policy(moe_tile_rows_q=32):
        base = gm(xg)
    assert calls == {"f8": [], "tile": [0, 1, 0, 1]} and torch.equal(_bits(off), _bits(base))


def test_block_graph_replay_follows_the_routing(gpu):
    _, gm, x = _block(gpu)
    inputs = [x[300 * i:300 * (i + 1)].to(gpu) for i in range(3)]
    with torch.no_grad(), ops.kernel_policy(moe_tile_rows_q=32, moe_tile_f8=True):
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
    nat = lambda a_sc, w_, s_, q=a.q: ops.native().moe_tile_gemm_f8(
        out, q, a_sc, w_, r.sorted_pairs, r.expert_count, r.expert_offset, T, K, 0, s_)
    big = ops.native().moe_tile_f8_max_k() + 128
    bad = [lambda: nat(a.sc, w.to(BF), None),                               # bf16 experts
           lambda: nat(a.sc, torch.zeros(E, 256, 128, dtype=U8, device=gpu),
                       torch.full((E, 256, 8), 127, dtype=U8, device=gpu)),  # MXFP4 experts
           lambda: nat(a.sc, w[:, :192].contiguous(), s[:, :192].contiguous()),       # N % 128
           lambda: nat(a.sc[:, :1].contiguous(), w[:, :, :192].contiguous(), s,
                       a.q[:, :192].contiguous()),                                    # K % 128
           lambda: nat(torch.full((T, big // 128), 127, dtype=U8, device=gpu),
                       torch.zeros(E, 256, big, dtype=BF, device=gpu).to(FP8), s,
                       torch.zeros(T, big, dtype=BF, device=gpu).to(FP8)),           # K > bound
           lambda: nat(torch.cat([a.sc, a.sc], 1), w, s),                   # a_sc shape
           lambda: nat(a.sc.int(), w, s),                                   # a_sc dtype
           lambda: nat(a.sc.cpu(), w, s),                                   # a_sc device
           lambda: nat(a.sc, w, None)]                                      # no scale
    with ops.kernel_policy(moe_tile_rows_q=32):
        bad += [lambda: ops.moe_grouped_gemm(x.to(gpu), w.to(BF), r, out=out, mx=True),
                lambda: ops.moe_grouped_gemm(x.to(gpu), ops.ExpertWeights(w, None), r, out=out, mx=True),
                lambda: ops.moe_grouped_gemm(x.to(gpu), ops.ExpertWeights(w[:, :192].contiguous(),
                                             s[:, :192].contiguous()), r, out=out, mx=True)]
        for i, f in enumerate(bad):
            with pytest.raises((RuntimeError, ValueError)):
                f()
                pytest.fail(f"case {i} was accepted")
    with pytest.raises(ValueError, match="moe_tile_rows_q"):     # the policy field at 0
        ops.moe_grouped_gemm(a, ops.ExpertWeights(w, s), r, out=out, mx=True)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
