"""MXFP4 expert weights on the grouped MoE GEMM (csrc/kernels/moe.hip, weight format kMoeFp4): bit
equality with the bf16 kernel on the dequantised weights (the e2m1 -> bf16 widening is exact), the
real quantiser against an fp32 oracle on the dequantised weights, host checks, the quantised block
against its CPU path, hipGraph replay and the engine under quantize="mxfp4_experts"."""
import copy

import pytest
import torch

from distributed_llm_inference import ops
from distributed_llm_inference.config import CacheConfig, ModelSpec, ServeConfig
from distributed_llm_inference.models.llama.modules import MoEMLP
from distributed_llm_inference.ops import reference as ref
from distributed_llm_inference.runtime.engine import EngineConfig, LLMEngine
from distributed_llm_inference.runtime.sequence import SamplingParams

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
U8 = torch.uint8
SENT = -12345.0
GROWS = 8          # sentinel rows before and after a guarded [rows, width] output
ATOL, RTOL = 2e-2, 2e-2     # test_moe_fp8_gpu.py's: the same numerics class (see the oracle test)
COUNTS = (0, 1, 16, 17, 32, 33, 70, 31)     # rows per expert; 200 pairs = 100 tokens x top-2
E, K_TOP = 8, 2
KUNROLL = 2                       # moe.hip's kUnrollOf<kMoeFp4>
K_GROUP = 128 * (8 * KUNROLL + 9)  # wave 0: one whole group of KUNROLL steps and a two-step tail


def _close(a, b, atol, rtol=0.0, msg=""):
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    assert not bad.any(), f"{msg} max err {err.max().item():.4g} at {bad.nonzero()[:5].tolist()}"


def _explicit_ids():
    """[100, 2] expert ids giving COUNTS rows per expert, two different experts per token, tokens
    and slots in random order (test_moe_fp8_gpu.py's routing)."""
    labels = torch.cat([torch.full((c,), e) for e, c in enumerate(COUNTS)])
    T = labels.numel() // 2
    ids = torch.stack([labels[:T], labels[T:]], 1)
    assert bool((ids[:, 0] != ids[:, 1]).all())
    g = torch.Generator().manual_seed(3)
    ids = ids[torch.randperm(T, generator=g)]
    flip = torch.rand(T, generator=g) < 0.5
    ids[flip] = ids[flip].flip(1)
    assert torch.bincount(ids.reshape(-1), minlength=E).tolist() == list(COUNTS)
    return ids.to(torch.int32)


def _guarded_rows(rows, width, gpu):
    buf = torch.full((GROWS + rows + GROWS, width), SENT, dtype=BF, device=gpu)
    return buf, buf[GROWS:]          # the op sees [rows + GROWS, width]; it may write `rows` rows


def _assert_guards(buf, rows, what):
    assert bool((buf[:GROWS] == SENT).all()), f"{what}: write before the output"
    assert bool((buf[GROWS + rows:] == SENT).all()), f"{what}: write past row P"


def _bits(t):
    return t.view(torch.int16)


# ------------------------------------------------------------------------- drawn codes and scales
def _scale_bytes(N, K):
    """bscale[e, n, kb] = 127 + d, d in [-8, 8] changing between neighbouring 32-k blocks of a row,
    with the row inside a lane's four (n % 4), between the two A tiles of a workgroup
    ((n // 16) % 2: gate against up), between workgroups and between experts."""
    n = torch.arange(N)[None, :, None]
    e = torch.arange(E)[:, None, None]
    kb = torch.arange(K // 32)[None, None, :]
    d = ((n % 4) + 3 * ((n // 16) % 2) + 5 * (n // 32) + e + 7 * kb) % 17 - 8
    assert d.min() >= -8 and d.max() <= 8
    assert bool((d[:, :, 1:] != d[:, :, :-1]).all())          # neighbouring blocks
    for a, b in ((0, 1), (0, 16), (0, 32)):                    # lane rows, A tiles, workgroups
        assert d[0, a, 0] != d[0, b, 0]
    assert d[0, 0, 0] != d[1, 0, 0]                            # experts
    return (127 + d).to(U8)


def _codes(shape, g):
    """e2m1 codes packed two per byte (element 2 j in the low nibble), uniform over the 15 codes
    the quantiser can emit: no 0x8 (negative zero)."""
    c = torch.randint(0, 15, shape, generator=g)
    c = c + (c >= 8).long()
    assert not bool((c == 8).any()) and c.max() == 15
    return (c[..., 0::2] | (c[..., 1::2] << 4)).to(U8)


@pytest.mark.parametrize("H,I", [(256, 128), (1152, 384), (K_GROUP, 128), (256, K_GROUP)])
def test_fp4_grouped_gemm_bit_equal_to_bf16_on_dequantised_weights(gpu, H, I):
    """e2m1 * 2^(byte - 127) is exact in bf16, so the bf16 kernel on the dequantised weights does
    the fp4 kernel's MFMAs on the same operands in the same order: the outputs are equal bit for
    bit -- as long as the fp4 kernel reads the nibbles in the bf16 kernel's k order and takes the
    scale byte of the right expert, row and 32-k block.  kt = 2: waves 2-7 have no step; kt = 9:
    wave 0 has two; K = K_GROUP (gate|up of the third shape, down of the fourth): wave 0 runs one
    whole group of kUnroll steps and a two-step tail, the other waves one step fewer."""
    g = torch.Generator().manual_seed(13 * H + I)
    ids = _explicit_ids()
    T = ids.shape[0]
    P = T * K_TOP
    x = torch.randn(T, H, generator=g).to(BF)
    tw = torch.rand(T, K_TOP, generator=g).to(BF).float()
    r = ops.moe_group(ids.to(gpu), tw.to(gpu), E)
    for down, (N, K) in ((False, (2 * I, H)), (True, (H, I))):
        packed = _codes((E, N, K), g)
        scales = _scale_bytes(N, K)
        assert packed.shape == (E, N, K // 2) and scales.shape == (E, N, K // 32)
        wb = torch.stack([ops.dequantize_mxfp4(packed[e], scales[e]) for e in range(E)])
        assert wb.dtype == BF and packed.numel() + scales.numel() < 25e6   # MXFP4 bytes
        tiny = torch.finfo(BF).tiny                      # every weight a normal bf16, or zero
        assert bool(((wb.float().abs() >= tiny) | (wb == 0)).all())
        xin = (torch.randn(P, K, generator=g).to(BF) if down else x).to(gpu)
        rows, width = P, (N if down else N // 2)
        b1, v1 = _guarded_rows(rows, width, gpu)
        b2, v2 = _guarded_rows(rows, width, gpu)
        want = ops.moe_grouped_gemm(xin, wb.to(gpu), r, down=down, out=v1)
        got = ops.moe_grouped_gemm(xin, packed.to(gpu), r, down=down, out=v2,
                                   w_block_scale=scales.to(gpu))
        torch.cuda.synchronize()
        what = f"{'down' if down else 'gate|up'} H={H} I={I}"
        _assert_guards(b1, rows, what + " (bf16)")
        _assert_guards(b2, rows, what + " (fp4)")
        assert bool(want[:P].float().isfinite().all()) and want[:P].float().abs().max() > 1
        assert torch.equal(_bits(got[:P]), _bits(want[:P])), what
        assert torch.equal(_bits(b2), _bits(b1)), what


# ------------------------------------------------------------------------- the real quantiser
_CASES = {}


def _gemm_case(H, I):
    """Inputs and the fp32 oracle of one (H, I), computed once: weights quantised by
    ops.quantize_expert_weights_mxfp4 (gate|up after swiglu_interleave); per pair, fp32 products
    of the bf16 rows with the dequantised weights (ops/reference.py), no intermediate rounding."""
    if (H, I) not in _CASES:
        g = torch.Generator().manual_seed(H + I)
        ids = _explicit_ids()
        T = ids.shape[0]
        x = torch.randn(T, H, generator=g).to(BF)
        wg = (torch.randn(E, I, H, generator=g) / H ** 0.5).to(BF)
        wu = (torch.randn(E, I, H, generator=g) / H ** 0.5).to(BF)
        wd = (torch.randn(E, H, I, generator=g) / I ** 0.5).to(BF)
        w = torch.rand(T, K_TOP, generator=g).to(BF).float()
        wgu = torch.stack([ops.swiglu_interleave(torch.cat([wg[j], wu[j]], 0)) for j in range(E)])
        wgu4, sgu = ops.quantize_expert_weights_mxfp4(wgu)
        wd4, sd = ops.quantize_expert_weights_mxfp4(wd)
        dgu = torch.stack([ops.swiglu_deinterleave(ref.dequantize_mxfp4(wgu4[j], sgu[j])).float()
                           for j in range(E)])
        dg, du = dgu[:, :I], dgu[:, I:]
        dd = torch.stack([ref.dequantize_mxfp4(wd4[j], sd[j]).float() for j in range(E)])
        e = ids.long()
        xf = x.float()
        gate = torch.einsum("th,tsih->tsi", xf, dg[e])
        up = torch.einsum("th,tsih->tsi", xf, du[e])
        h = torch.nn.functional.silu(gate) * up                     # [T, k, I], by pair
        y = torch.einsum("tsi,tshi->tsh", h, dd[e])                  # [T, k, H]
        out = (w[:, :, None] * y).sum(1)
        _CASES[(H, I)] = dict(ids=ids, x=x, w=w, wgu4=wgu4, sgu=sgu, wd4=wd4, sd=sd, dd=dd,
                              h=h.reshape(T * K_TOP, I), y=y.reshape(T * K_TOP, H), out=out)
    return _CASES[(H, I)]


@pytest.mark.parametrize("H,I", [(256, 128), (1152, 384)])
def test_fp4_grouped_gemm_and_combine_against_fp32_oracle(gpu, H, I):
    """The oracle multiplies with the quantised weights, so the tolerance holds no quantisation
    error: the GPU result differs by summation order and the bf16 roundings of gate, up, h and y
    only -- the numerics class test_moe_fp8_gpu.py bounds with the same ATOL / RTOL."""
    c = _gemm_case(H, I)
    T = c["ids"].shape[0]
    P = T * K_TOP
    r = ops.moe_group(c["ids"].to(gpu), c["w"].to(gpu), E)
    want_r = ops.moe_group(c["ids"], c["w"], E)
    assert r.expert_count.cpu().tolist() == list(COUNTS)
    pairs = want_r.sorted_pairs.long()
    x = c["x"].to(gpu)
    wgu4, sgu, wd4, sd = (c[n].to(gpu) for n in ("wgu4", "sgu", "wd4", "sd"))
    assert wgu4.dtype == U8 and wgu4.shape == (E, 2 * I, H // 2)
    assert sgu.shape == (E, 2 * I, H // 32)
    assert wd4.dtype == U8 and wd4.shape == (E, H, I // 2) and sd.shape == (E, H, I // 32)

    hbuf, hview = _guarded_rows(P, I, gpu)
    h = ops.moe_grouped_gemm(x, wgu4, r, out=hview, w_block_scale=sgu)
    torch.cuda.synchronize()
    _assert_guards(hbuf, P, "gate|up")
    _close(h[:P], c["h"][pairs], ATOL, RTOL, f"gate|up H={H} I={I}")

    ybuf, yview = _guarded_rows(P, H, gpu)
    y = ops.moe_grouped_gemm(h[:P].contiguous(), wd4, r, down=True, out=yview, w_block_scale=sd)
    torch.cuda.synchronize()
    _assert_guards(ybuf, P, "down")
    _close(y[:P], c["y"], ATOL, RTOL, f"down H={H} I={I}")        # back in pair order
    # ... and exactly the product of the rows the kernel read
    e_of_pair = c["ids"].reshape(-1).long()
    hp = torch.empty(P, I)
    hp[pairs] = h[:P].float().cpu()
    _close(y[:P], torch.einsum("pi,phi->ph", hp, c["dd"][e_of_pair]), ATOL, RTOL, "down/h")

    out = ops.moe_combine(y[:P].contiguous(), r.topk_w)
    torch.cuda.synchronize()
    _close(out, c["out"], ATOL, RTOL, f"combine H={H} I={I}")
    # the CPU front end is the same computation within the oracle tolerance
    cpu = ops.moe_combine(
        ops.moe_grouped_gemm(
            ops.moe_grouped_gemm(c["x"], c["wgu4"], want_r, w_block_scale=c["sgu"]),
            c["wd4"], want_r, down=True, w_block_scale=c["sd"]), c["w"])
    _close(out, cpu, ATOL, RTOL, "GPU vs CPU front end")
    # ... and the whole op with the keyword arguments of ops.moe_mlp's grouped GEMMs
    assert torch.equal(_bits(ops.moe_grouped_gemm(x, wgu4, r, w_block_scale=sgu)), _bits(h[:P]))


def test_fp4_grouped_gemm_deterministic_and_host_checks(gpu):
    c = _gemm_case(256, 128)
    r = ops.moe_group(c["ids"].to(gpu), c["w"].to(gpu), E)
    x, w4, s = c["x"].to(gpu), c["wgu4"].to(gpu), c["sgu"].to(gpu)
    a = ops.moe_grouped_gemm(x, w4, r, w_block_scale=s)
    b = ops.moe_grouped_gemm(x, w4, r, w_block_scale=s)
    assert torch.equal(_bits(a), _bits(b))
    wb = torch.stack([ops.dequantize_mxfp4(w4[e], s[e]) for e in range(E)])
    assert torch.equal(_bits(ops.moe_grouped_gemm(x, wb, r)), _bits(a))
    err = (RuntimeError, ValueError)
    with pytest.raises(err, match="not both"):
        ops.moe_grouped_gemm(x, w4, r, w_scale=torch.ones(E, 256, device=gpu), w_block_scale=s)
    with pytest.raises(err, match="w_block_scale"):
        ops.moe_grouped_gemm(x, w4, r)                               # nibbles without scales
    with pytest.raises(err, match="w_block_scale"):
        ops.moe_grouped_gemm(x, wb, r, w_block_scale=s)              # bf16 weights with them
    with pytest.raises(err, match="w_block_scale"):
        ops.moe_grouped_gemm(x, w4, r, w_block_scale=s[:, :, :-1].contiguous())
    with pytest.raises(err, match="w_block_scale"):
        ops.moe_grouped_gemm(x, w4, r, w_block_scale=s[:, :-1].contiguous())
    with pytest.raises(err, match="w_block_scale"):
        ops.moe_grouped_gemm(x, w4, r, w_block_scale=s.cpu())
    with pytest.raises(err, match="w_block_scale"):
        ops.moe_grouped_gemm(x, w4, r, w_block_scale=s.float())
    with pytest.raises(err, match="K % 128"):
        ops.moe_grouped_gemm(x[:, :192].contiguous(), w4[:, :, :96].contiguous(), r,
                             w_block_scale=s[:, :, :6].contiguous())
    # the binding's own checks, without the Python front end before them
    nat = ops.native().moe_grouped_gemm
    out = torch.empty(200, 128, dtype=BF, device=gpu)
    tabs = (r.sorted_pairs, r.tile_expert, r.tile_start, r.tile_rows, r.n_tiles, 100, 2, 0)
    nat(out, x, w4, *tabs, s)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(a))
    with pytest.raises(RuntimeError, match="w_block_scale"):         # an fp8 row scale instead
        nat(out, x, w4, *tabs, torch.ones(E, 256, device=gpu))
    with pytest.raises(RuntimeError, match="w_block_scale"):
        nat(out, x, w4, *tabs)
    with pytest.raises(RuntimeError, match="w_block_scale"):
        nat(out, x, wb, *tabs, s)
    with pytest.raises(RuntimeError, match="w_block_scale"):
        nat(out, x, w4, *tabs, s[:, :, :-1].contiguous())
    with pytest.raises(RuntimeError):
        nat(out, x, w4, *tabs, s.cpu())
    with pytest.raises(RuntimeError, match="K % 128"):
        nat(out, x[:, :192].contiguous(), w4[:, :, :96].contiguous(), *tabs,
            s[:, :, :6].contiguous())


# ------------------------------------------------------------------------------------- the block
def _moe_spec(n_experts, k):
    return ModelSpec(name="moe-t", model_type="qwen3_moe", qk_norm=True, vocab_size=512,
                     hidden_size=256, intermediate_size=512, num_layers=2, num_heads=2,
                     num_kv_heads=1, head_dim=128, rms_norm_eps=1e-6, rope_theta=10000.0,
                     max_position_embeddings=4096, bos_token_id=1, eos_token_id=2,
                     num_experts=n_experts, num_experts_per_tok=k, moe_intermediate_size=128,
                     norm_topk_prob=True)


_BLOCKS = {}


def _block_case(n_experts, k):
    """A CPU MoEMLP with weights of unit-scale products, its experts quantised to MXFP4, and 40
    rows whose CPU fp32 router logits have their k-th and (k+1)-th largest >= 1/16 apart with
    every |logit| < 4 -- picked from random candidates, so bf16 logit rounding cannot change the
    routing of any of them (the router stays bf16)."""
    if (n_experts, k) not in _BLOCKS:
        g = torch.Generator().manual_seed(17 * n_experts + k)
        mlp = MoEMLP(_moe_spec(n_experts, k))
        H, I = 256, 128
        with torch.no_grad():
            mlp.gate.weight.copy_((torch.randn(n_experts, H, generator=g) / H ** 0.5).to(BF))
            mlp.w_gate_up.copy_((torch.randn(n_experts, 2 * I, H, generator=g) / H ** 0.5).to(BF))
            mlp.w_down.copy_((torch.randn(n_experts, H, I, generator=g) / I ** 0.5).to(BF))
        mlp.quantize_experts_mxfp4()
        cand = torch.randn(600, H, generator=g).to(BF)
        lf = cand.float() @ mlp.gate.weight.float().t()
        top = lf.sort(-1, descending=True).values
        ok = ((top[:, k - 1] - top[:, k]) >= 1 / 16) & (lf.abs().max(-1).values < 4)
        x = cand[ok][:40].contiguous()
        _BLOCKS[(n_experts, k)] = (mlp, x)
    return _BLOCKS[(n_experts, k)]


def _on_gpu(mlp, gpu):
    gm = copy.deepcopy(mlp).to(gpu)
    assert gm.is_mxfp4 and not gm.is_fp8
    assert gm.w_gate_up.dtype == U8 and gm.w_down.dtype == U8 and gm.w_gate_up.is_cuda
    assert gm.w_gate_up_block_scale.is_cuda and gm.w_down_block_scale.dtype == U8
    assert gm.gate.weight.dtype == BF
    return gm


@pytest.mark.parametrize("T", [1, 4, 40])
@pytest.mark.parametrize("n_experts,k", [(8, 2), (128, 8)])
def test_fp4_moe_block_gpu_matches_cpu_path(gpu, n_experts, k, T):
    mlp, x40 = _block_case(n_experts, k)
    assert x40.shape[0] == 40
    x = x40[:T].contiguous()
    lf = x.float() @ mlp.gate.weight.float().t()                 # the fixture's promise, per row
    top = lf.sort(-1, descending=True).values
    assert bool(((top[:, k - 1] - top[:, k]) >= 1 / 16).all()) and bool((lf.abs() < 4).all())
    gm = _on_gpu(mlp, gpu)
    xg = x.to(gpu)
    want_ids, _ = ops.moe_topk(mlp.gate(x), k, True)
    got_ids, _ = ops.moe_topk(gm.gate(xg), k, True)
    assert torch.equal(got_ids.cpu().sort(-1).values, want_ids.sort(-1).values)   # equal routing
    want = mlp(x)
    got = gm(xg)
    torch.cuda.synchronize()
    assert got.dtype == BF and got.shape == (T, 256)
    _close(got, want, ATOL, RTOL, f"MXFP4 MoE block E={n_experts} k={k} T={T}")
    assert want.float().abs().max() > 0.1


def test_fp4_moe_block_graph_replay_follows_the_routing(gpu):
    """Captured once with static buffers; replayed on three inputs that route differently: every
    replay is bit-equal to the eager call."""
    mlp, x40 = _block_case(128, 8)
    gm = _on_gpu(mlp, gpu)
    T = 12
    inputs = [x40[i * T:(i + 1) * T].to(gpu) for i in range(3)]
    with torch.no_grad():
        eager = [gm(x).clone() for x in inputs]
        routes = [ops.moe_topk(gm.gate(x), 8, True)[0].cpu() for x in inputs]
    assert not torch.equal(routes[0], routes[1]) and not torch.equal(routes[1], routes[2])
    static_x = inputs[2].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(2):
            gm(static_x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        static_y = gm(static_x)
    for x, want in zip(inputs, eager):
        static_x.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(static_y), _bits(want))


# ------------------------------------------------------------------------------------- engine
def _engine(graphs):
    # num_blocks is fixed (a test must not size a KV pool from the whole device's free memory),
    # so the block count says nothing about the memory the MXFP4 experts free
    cfg = EngineConfig(model="moe-t", pp=1, seed=5, quantize="mxfp4_experts",
                       cache=CacheConfig(num_blocks=128, block_size=64, max_chunk=256),
                       serve=ServeConfig(max_batch_size=4, max_num_batched_tokens=256,
                                         max_seq_len=512, use_graphs=graphs,
                                         graph_batch_sizes=[1, 2, 4]))
    return LLMEngine(_moe_spec(8, 2), device="cuda:0", cfg=cfg)


def test_fp4_experts_engine_graph_decode_equals_eager(gpu):
    prompts = [list(range(3, 40)), [7, 8, 9], [11]]
    p = SamplingParams(max_tokens=8, ignore_eos=True)
    eng = _engine(graphs=False)
    layers = eng.executors[0].stage.block.layers
    assert len(layers) == 2
    for l in layers:
        assert isinstance(l.mlp, MoEMLP) and l.mlp.is_mxfp4 and not l.mlp.is_fp8
        assert l.mlp.w_gate_up.dtype == U8 and l.mlp.w_gate_up.shape == (8, 256, 128)
        assert l.mlp.w_down.dtype == U8 and l.mlp.w_down.shape == (8, 256, 64)
        assert l.mlp.w_gate_up_block_scale.shape == (8, 256, 8)
        assert l.mlp.w_down_block_scale.shape == (8, 256, 4)
        assert l.mlp.gate.weight.dtype == BF
        assert l.self_attn.qkv_proj.weight.dtype == BF
        assert l.self_attn.o_proj.weight.dtype == BF
    a = [s.output for s in eng.generate(prompts, p)]
    b = [s.output for s in _engine(graphs=True).generate(prompts, p)]
    assert all(len(o) == 8 for o in a) and a == b
