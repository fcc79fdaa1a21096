"""The fp8 x fp8 MFMA tile GEMM for block-scaled fp8 experts (csrc/kernels/moe_tile_scaled.hip)
on the GPU: exactly-summable operands bit for bit, random data against fp64, row independence, the
MoE block under ``KernelPolicy.moe_tile_f8_block`` (eager and in a captured graph) and the host
checks."""
import copy

import pytest
import torch

import moe_tile_cases as mc
from moe_tile_cases import (bits as _bits, guarded as _guarded, products as _products,
                            swiglu64 as _swiglu64)
from distributed_llm_inference import ops
from distributed_llm_inference.config import ModelSpec
from distributed_llm_inference.models.llama.modules import MoEMLP
from distributed_llm_inference.ops.reference import expand_fp8_block_scale

pytestmark = pytest.mark.gpu
BF, FP8, U8 = torch.bfloat16, torch.float8_e4m3fn, torch.uint8
SENT = mc.SENT
E, K = mc.E, mc.K_TOP
SHAPES = [(256, 128), (1152, 384)]


def _close(got, want):
    return float(want.abs().max()) > 0.5 and mc.close(got, want)


def _routing(gpu):
    ids, r, pairs = mc.routing(gpu)
    return ids, r, pairs, ids.reshape(-1).long()[pairs]       # .., the expert of sorted row j


_dq = lambda w: w.w.float().double() * expand_fp8_block_scale(w.scale).double()
_to = lambda w, gpu: ops.ExpertWeights(w.w.to(gpu), w.scale.to(gpu))


def _exact_operands(R, N, Kd, lo, p, seed):
    """fp8 experts [E, N, Kd] from every e4m3 code with exponent field lo .. lo + 2 (both signs,
    all 8 mantissas); block scales m 2^p, m in {1, 1.25, 1.5, 1.75}, differing across experts,
    16-row groups and k-blocks; activations integers in [-4, 4] as e4m3 with exponents 0 / 1
    differing per (row, 128-block).  Every term s w a is a multiple of q = 2^(lo - 10 + p - 2)
    and a row's sum of magnitudes stays below 2^23 q, so any fp32 summation order, fused or
    not, is exact (asserted)."""
    g = torch.Generator().manual_seed(seed)
    code = torch.randint(0, 48, (E, N, Kd), generator=g)
    code[0, 0, :48] = torch.arange(48)
    w = (((code // 24) << 7) | ((lo + code % 24 // 8) << 3) | (code % 8)).to(U8).view(FP8)
    s = ((4 + torch.randint(0, 4, (E, N // 16, Kd // 128), generator=g)) * 2.0 ** (p - 2)).float()
    xi = torch.randint(-4, 5, (R, Kd), generator=g).float()
    ex = torch.randint(0, 2, (R, Kd // 128), generator=g)
    a, ws = ops.MxFp8Rows(xi.to(FP8), (ex + 127).to(U8)), ops.ExpertWeights(w, s)
    wd, ad, q = _dq(ws), a.dequantize().double(), 2.0 ** (lo - 10 + p - 2)
    assert w.view(U8).unique().numel() == 48 and s.unique().numel() == 4
    assert not torch.equal(s[0], s[1]) and not torch.equal(s[:, 0], s[:, 1])
    assert Kd == 128 or not (torch.equal(s[:, :, 0], s[:, :, 1]) or torch.equal(ex[:, 0], ex[:, 1]))
    assert torch.equal(ad, xi.double() * torch.exp2(ex.double()).repeat_interleave(128, dim=1))
    assert torch.equal(wd / q, (wd / q).round()) and torch.equal(ad, ad.round())
    assert max(float((ad.abs() @ wd[e].abs().t()).max()) for e in range(E)) / q < 2 ** 23
    return a, ws, ad, wd


@pytest.mark.parametrize("H,I", SHAPES)
def test_layout_bit_exact_against_fp64_and_the_widening_kernel(gpu, H, I):
    ids, r, pairs, e_row = _routing(gpu)
    T, P = ids.shape[0], ids.numel()
    with ops.kernel_policy(moe_tile_rows_q=32):
        # down: h rows in sorted order, K = I
        a, w, ad, wd = _exact_operands(P, H, I, 6, 0, H + I)
        ag, wg = ops.MxFp8Rows(a.q.to(gpu), a.sc.to(gpu)), _to(w, gpu)
        y = _guarded(lambda o: ops.moe_grouped_gemm(ag, wg, r, down=True, out=o, f8_block=True),
                     P, H, gpu)
        yw = ops.moe_grouped_gemm(ad.to(BF).to(gpu), wg, r, down=True, tiles=True).cpu()
        want = torch.empty(P, H, dtype=BF)
        want[pairs] = _products(ad, wd, e_row).float().to(BF)
        assert torch.equal(_bits(y), _bits(want)), (y.float() - want.float()).abs().max()
        assert torch.equal(_bits(y), _bits(yw))
        # gate|up: x per token, K = H.  Sums of deviation 16 sqrt(K) (tests/test_moe_tile_f8_gpu.py)
        # times scales of 1 / (8 sqrt(K)) .. 1.75 times that, rounded down to a power of two,
        # bring the gate to a deviation of 1 .. 3: inside silu's bend
        a, w, ad, wd = _exact_operands(T, 2 * I, H, 7, -7 if H == 256 else -9, H - I)
        ag, wg = ops.MxFp8Rows(a.q.to(gpu), a.sc.to(gpu)), _to(w, gpu)
        h = _guarded(lambda o: ops.moe_grouped_gemm(ag, wg, r, out=o, f8_block=True), P, I, gpu)
        hw = ops.moe_grouped_gemm(ad.to(BF).to(gpu), wg, r, tiles=True).cpu()
    gu = _products(ad[pairs // K], wd, e_row).float().to(BF).double()
    assert 0.25 < float(gu.abs().median()) < 8, "gate values outside silu's bend"
    assert torch.equal(_bits(h), _bits(hw)), (h.float() - hw.float()).abs().max()
    assert _close(h, _swiglu64(gu))


def _random_case(H, I, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(mc.explicit_ids().shape[0], H, generator=g).to(BF)
    gu = ops.ExpertWeights.quantize((torch.randn(E, 2 * I, H, generator=g) / H ** 0.5).to(BF), "fp8_block")
    dn = ops.ExpertWeights.quantize((torch.randn(E, H, I, generator=g) / I ** 0.5).to(BF), "fp8_block")
    return x, gu, dn


def _run(gpu, x, gu, dn, r):
    with ops.kernel_policy(moe_tile_rows_q=32):
        h = ops.moe_grouped_gemm(x.to(gpu), _to(gu, gpu), r, f8_block=True)
        y = ops.moe_grouped_gemm(h, _to(dn, gpu), r, down=True, f8_block=True)
    return h.cpu(), y.cpu()


@pytest.mark.parametrize("H,I", SHAPES)
def test_random_against_fp64_on_quantise_dequantised_operands(gpu, H, I):
    ids, r, pairs, e_row = _routing(gpu)
    x, gu, dn = _random_case(H, I, H)
    h, y = _run(gpu, x, gu, dn, r)
    xd = ops.quant_mx_rows(x).dequantize().double()[pairs // K]
    want_y = torch.empty(ids.numel(), H, dtype=torch.float64)
    want_y[pairs] = _products(ops.quant_mx_rows(h).dequantize().double(), _dq(dn), e_row)
    assert _close(h, _swiglu64(_products(xd, _dq(gu), e_row))) and _close(y, want_y)


def test_rows_are_independent_and_launch_is_deterministic(gpu):
    H, I = 256, 128
    ids, r, pairs = mc.routing(gpu)
    T = ids.shape[0]
    x, gu, dn = _random_case(H, I, 5)
    h, y = _run(gpu, x, gu, dn, r)
    h2, y2 = _run(gpu, x, gu, dn, r)
    assert torch.equal(_bits(h), _bits(h2)) and torch.equal(_bits(y), _bits(y2))
    perm = torch.randperm(T, generator=torch.Generator().manual_seed(9))
    _, rp, pairs_p = mc.routing(gpu, ids[perm])
    hp, yp = _run(gpu, x[perm], gu, dn, rp)
    by_pair = lambda h_, p_: torch.empty_like(h_).index_copy_(0, p_, h_).view(T, K, -1)
    assert torch.equal(_bits(by_pair(hp, pairs_p)), _bits(by_pair(h, pairs)[perm]))
    assert torch.equal(_bits(yp.view(T, K, H)), _bits(y.view(T, K, H)[perm]))


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
    mlp.quantize_experts_fp8_block()
    return mlp, copy.deepcopy(mlp).to(gpu), torch.randn(900, 256, generator=g).to(BF)


def test_block_under_the_policy(gpu, monkeypatch):
    mlp, gm, x = _block(gpu)
    xg, nat, calls, outs = x[:300].to(gpu), ops.native(), {"f8b": [], "tile": []}, []
    monkeypatch.setattr(nat, "moe_tile_gemm_f8_block", lambda *a, real=nat.moe_tile_gemm_f8_block:
                        (calls["f8b"].append(int(a[9])), outs.append(a[0]), real(*a))[2])
    monkeypatch.setattr(nat, "moe_tile_gemm", lambda *a, real=nat.moe_tile_gemm:
                        (calls["tile"].append(int(a[8])), real(*a))[1])
    with torch.no_grad(), ops.kernel_policy(moe_tile_rows_q=32, moe_tile_f8_block=True):
        assert ops.moe_uses_f8_block(300, K, E, "fp8_block", xg.device)
        got = gm(xg).cpu()
        assert calls == {"f8b": [0, 1], "tile": []}
        # the CPU path with f8_block=True on the GPU's routing, one product at a time: the fp8
        # quantiser of h turns a bf16 ulp between two correct h into an fp8 ulp of a down operand,
        # which no tolerance on a product bounds (docs/kernels.md has the figures)
        rg = ops.moe_route(gm.gate(xg), K, True)
        r = ops.moe_group(rg.topk_ids.cpu(), rg.topk_w.cpu(), E)
        h = outs[0].cpu()
        assert _close(h, ops.moe_grouped_gemm(x[:300], mlp.experts("w_gate_up"), r, f8_block=True))
        y = ops.moe_grouped_gemm(h, mlp.experts("w_down"), r, down=True, f8_block=True)
    assert _close(got, ops.moe_combine(y, r.topk_w))
    del calls["f8b"][:]
    outs = []
    for kw in ({"moe_tile_f8_block": False}, {"moe_tile_f8": True}, {}):     # {}: today's call
        with torch.no_grad(), ops.kernel_policy(moe_tile_rows_q=32, **kw):
            outs.append(gm(xg))
    assert calls == {"f8b": [], "tile": [0, 1] * 3}
    assert torch.equal(_bits(outs[0]), _bits(outs[2])) and torch.equal(_bits(outs[1]), _bits(outs[2]))


def test_block_graph_replay_follows_the_routing(gpu):
    _, gm, x = _block(gpu)
    inputs = [x[300 * i:300 * (i + 1)].to(gpu) for i in range(3)]
    with torch.no_grad(), ops.kernel_policy(moe_tile_rows_q=32, moe_tile_f8_block=True):
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


def test_host_checks_reject_before_any_launch(gpu):
    ids, r, _, _ = _routing(gpu)
    T, P = ids.shape[0], ids.numel()
    g = torch.Generator().manual_seed(1)
    wb = (torch.randn(E, 256, 256, generator=g) / 16).to(BF)
    a = ops.quant_mx_rows(torch.randn(T, 256, generator=g).to(BF).to(gpu))
    w, s = _to(ops.ExpertWeights.quantize(wb, "fp8_block"), gpu)
    out = torch.full((P, 128), SENT, dtype=BF, device=gpu)
    nat = lambda w_, s_, q=a.q, a_sc=a.sc: ops.native().moe_tile_gemm_f8_block(
        out, q, a_sc, w_, r.sorted_pairs, r.expert_count, r.expert_offset, T, K, 0, s_)
    big = ops.native().moe_tile_f8_block_max_k() + 128
    z8 = lambda *shape: torch.zeros(*shape, dtype=BF, device=gpu).to(FP8)
    bad = [lambda: nat(w.to(BF), None),                                          # bf16 experts
           lambda: nat(w, s[:, :, 0].repeat_interleave(16, 1).contiguous()),     # per-row fp8
           lambda: nat(torch.zeros(E, 256, 128, dtype=U8, device=gpu),
                       torch.full((E, 256, 8), 127, dtype=U8, device=gpu)),      # MXFP4 experts
           lambda: nat(w[:, :192].contiguous(), s[:, :12].contiguous()),         # N % 128
           lambda: nat(w[:, :, :192].contiguous(), s, a.q[:, :192].contiguous(),
                       a.sc[:, :1].contiguous()),                                # K % 128
           lambda: nat(z8(E, 256, big), torch.ones(E, 16, big // 128, device=gpu), z8(T, big),
                       torch.full((T, big // 128), 127, dtype=U8, device=gpu)),  # K > bound
           lambda: nat(w, s[:, :8].contiguous()),                                # scale shape
           lambda: nat(w, s.double()),                                           # scale dtype
           lambda: nat(w, s.cpu())]                                              # scale device
    with ops.kernel_policy(moe_tile_rows_q=32):
        for i, f in enumerate(bad):
            with pytest.raises((RuntimeError, ValueError)):
                f()
                pytest.fail(f"case {i} was accepted")
    with pytest.raises(ValueError, match="moe_tile_rows_q"):     # the policy field at 0
        ops.moe_grouped_gemm(a, ops.ExpertWeights(w, s), r, out=out, f8_block=True)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
