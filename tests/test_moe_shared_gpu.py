"""The shared-expert pieces of the sparse-MoE kernels (csrc/kernels/moe.hip) on the GPU: routing
with the shared gate's logit as one more column of strided router logits, the combine with the
shared term, the Qwen2-MoE block against its CPU path, hipGraph replay with changing routing, and
the engine on a stack that mixes dense and sparse layers."""
import pytest
import torch

from distributed_llm_inference import ops
from distributed_llm_inference.config import CacheConfig, ModelSpec, ServeConfig
from distributed_llm_inference.models.llama.modules import LlamaMLP, MoEMLP
from distributed_llm_inference.ops import reference as ref
from distributed_llm_inference.runtime.engine import EngineConfig, LLMEngine
from distributed_llm_inference.runtime.sequence import SamplingParams

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SENT = -12345.0
GROWS = 8          # sentinel rows before and after a guarded [rows, width] output
ATOL, RTOL = 2e-2, 2e-2     # test_moe_gpu.py's numerics class


def _close(a, b, atol, rtol=0.0, msg=""):
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    assert not bad.any(), f"{msg} max err {err.max().item():.4g} at {bad.nonzero()[:5].tolist()}"


# ------------------------------------------------------------------------------------- routing
def _perm_logits(T, E, seed):
    """test_moe_gpu.py's: every row a permutation of E distinct bf16 values (multiples of 1/16 in
    [-4, 4)): no tie anywhere."""
    g = torch.Generator().manual_seed(seed)
    vals = (torch.arange(E, dtype=torch.float32) - E / 2) / 16
    assert torch.equal(vals.to(BF).float(), vals)
    return torch.stack([vals[torch.randperm(E, generator=g)] for _ in range(T)]).to(BF)


def _bf16_ulp(w):
    return torch.exp2(torch.floor(torch.log2(w)) - 7)


def _gate_column(T):
    """T gate logits spanning [-8, 8], with +0 and -0 among them where there is room."""
    col = torch.linspace(-8, 8, T)
    col[0] = 0.0
    if T > 1:
        col[T // 2] = -0.0
        col[1], col[-1] = -8.0, 8.0
    return col.to(BF)


def _assert_grouping_equal(got, want):
    n = int(want.n_tiles)
    assert int(got.n_tiles) == n
    for name in ("expert_count", "expert_offset", "sorted_pairs"):
        assert torch.equal(getattr(got, name).cpu(), getattr(want, name).cpu()), name
    for name in ("tile_expert", "tile_start", "tile_rows"):
        assert torch.equal(getattr(got, name)[:n].cpu(), getattr(want, name)[:n].cpu()), name


@pytest.mark.parametrize("renorm", [False, True])
@pytest.mark.parametrize("T,E,k,ld", [(1, 8, 2, 9), (5, 60, 4, 64), (67, 128, 8, 136),
                                      (33, 256, 8, 264)])
def test_route_with_the_gate_column(gpu, T, E, k, ld, renorm):
    """E = 60 leaves lanes without an expert, ld > E + 1 exercises the stride and the padding
    (+30: it would win every ranking if it were read), E = 256 puts the gate in column 256."""
    logits = torch.full((T, ld), 30.0, dtype=BF)
    logits[:, :E] = _perm_logits(T, E, 100 * T + E)
    col = _gate_column(T)
    logits[:, E] = col
    if T > 1:
        bits = col.view(torch.int16)
        assert bits[0] == 0 and bits[T // 2] == -32768            # +0 and -0
    want = ops.moe_route(logits, k, renorm, num_experts=E)
    got = ops.moe_route(logits.to(gpu), k, renorm, num_experts=E)
    torch.cuda.synchronize()
    assert got.topk_ids.dtype == torch.int32 and got.topk_w.dtype == torch.float32
    assert torch.equal(got.topk_ids.cpu(), want.topk_ids)
    err = (got.topk_w.cpu() - want.topk_w).abs()
    assert bool((err <= _bf16_ulp(want.topk_w)).all()), err.max().item()
    w = got.topk_w.cpu()
    assert torch.equal(w.to(BF).float(), w)                 # the stored weight is a bf16 value
    sw, want_sw = got.shared_w.cpu(), torch.sigmoid(col).float()
    assert sw.dtype == torch.float32 and sw.shape == (T,)
    assert torch.equal(want.shared_w, want_sw)
    assert bool(((sw - want_sw).abs() <= _bf16_ulp(want_sw)).all()), (sw - want_sw).abs().max()
    assert torch.equal(sw.to(BF).float(), sw)               # ... and so is the gate's sigmoid
    assert sw[0] == 0.5 and (T == 1 or sw[T // 2] == 0.5)
    _assert_grouping_equal(got, want)
    # ids and w are those of the contiguous [:, :E] slice, bit for bit, on the same kernel
    plain = ops.moe_route(logits[:, :E].contiguous().to(gpu), k, renorm)
    assert plain.shared_w is None
    assert torch.equal(plain.topk_ids, got.topk_ids)
    assert torch.equal(plain.topk_w.view(torch.int32), got.topk_w.view(torch.int32))
    _assert_grouping_equal(got, plain)
    again = ops.moe_route(logits.to(gpu), k, renorm, num_experts=E)   # deterministic
    assert torch.equal(again.topk_w, got.topk_w) and torch.equal(again.topk_ids, got.topk_ids)
    assert torch.equal(again.shared_w.view(torch.int32), got.shared_w.view(torch.int32))
    _assert_grouping_equal(again, want)


def test_route_host_checks(gpu):
    lg = torch.zeros(4, 9, dtype=BF, device=gpu)
    ids = torch.empty(4, 2, dtype=torch.int32, device=gpu)
    w = torch.empty(4, 2, device=gpu)
    with pytest.raises(ValueError, match="num_experts"):
        ops.moe_topk(lg, 2, False, num_experts=9)
    with pytest.raises(RuntimeError, match="num_experts"):
        ops.native().moe_topk(ids, w, lg, False, 9, torch.empty(4, device=gpu))
    with pytest.raises(RuntimeError, match="shared_w"):
        ops.native().moe_topk(ids, w, lg, False, 8, torch.empty(5, device=gpu))
    with pytest.raises(RuntimeError, match="float32"):
        ops.native().moe_topk(ids, w, lg, False, 8, torch.empty(4, dtype=BF, device=gpu))
    with pytest.raises(RuntimeError, match="shared_w"):
        ops.native().moe_topk(ids, w, lg, False, 8, torch.empty(4))
    with pytest.raises(RuntimeError, match="go together"):
        ops.native().moe_topk(ids, w, lg, False, 8)


# ------------------------------------------------------------------------------------- combine
def _guarded_rows(rows, width, gpu):
    buf = torch.full((GROWS + rows + GROWS, width), SENT, dtype=BF, device=gpu)
    return buf, buf[GROWS:]


def _assert_guards(buf, rows, what):
    assert bool((buf[:GROWS] == SENT).all()), f"{what}: write before the output"
    assert bool((buf[GROWS + rows:] == SENT).all()), f"{what}: write past the last row"


@pytest.mark.parametrize("T,k,H", [(1, 2, 256), (33, 8, 1152), (40, 4, 256)])
def test_combine_with_the_shared_term(gpu, T, k, H):
    """1 row; 33 x 1152 / 8 = 4752 vectors (19 workgroups, the last one partly idle) at k = 8;
    40 x 256 / 8 = 1280 vectors, exactly 5 workgroups."""
    g = torch.Generator().manual_seed(T + k + H)
    y = torch.randn(T * k, H, generator=g).to(BF)
    w = torch.rand(T, k, generator=g).to(BF).float()
    s = torch.randn(T, H, generator=g).to(BF)
    sw = torch.rand(T, generator=g).to(BF).float()
    yg, wg, sg, swg = (t.to(gpu) for t in (y, w, s, sw))
    buf, view = _guarded_rows(T, H, gpu)
    out = ops.moe_combine(yg, wg, out=view[:T], shared=sg, shared_w=swg)
    torch.cuda.synchronize()
    _assert_guards(buf, T, "combine + shared")
    want = ref.moe_combine(y, w, s, sw).float()
    assert bool(((out.float().cpu() - want).abs() <= 2.0 ** -7 * want.abs()).all())
    assert not torch.equal(out.cpu(), ref.moe_combine(y, w))        # the term is in the sum
    # shared_w = 0: the kernel without the shared term, bit for bit
    buf0, view0 = _guarded_rows(T, H, gpu)
    zero = ops.moe_combine(yg, wg, out=view0[:T], shared=sg, shared_w=torch.zeros_like(swg))
    plain = ops.moe_combine(yg, wg)
    torch.cuda.synchronize()
    _assert_guards(buf0, T, "combine + shared, zero weight")
    assert torch.equal(zero.view(torch.int16), plain.view(torch.int16))
    # no routed weight at all: bf16(shared_w * s)
    only = ops.moe_combine(yg, torch.zeros_like(wg), shared=sg, shared_w=swg)
    assert torch.equal(only.cpu(), (sw[:, None] * s.float()).to(BF))


def test_combine_host_checks(gpu):
    T, k, H = 6, 2, 256
    y = torch.zeros(T * k, H, dtype=BF, device=gpu)
    w = torch.zeros(T, k, device=gpu)
    s = torch.zeros(T, H, dtype=BF, device=gpu)
    sw = torch.zeros(T, device=gpu)
    ops.moe_combine(y, w, shared=s, shared_w=sw)
    with pytest.raises(RuntimeError, match="shared"):
        ops.moe_combine(y, w, shared=s[:, :128].contiguous(), shared_w=sw)
    with pytest.raises(RuntimeError, match="shared"):
        ops.moe_combine(y, w, shared=s[:5].contiguous(), shared_w=sw)
    with pytest.raises(RuntimeError, match="shared"):
        ops.moe_combine(y, w, shared=s.float(), shared_w=sw)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.moe_combine(y, w, shared=torch.zeros(T, 2 * H, dtype=BF, device=gpu)[:, ::2],
                        shared_w=sw)
    with pytest.raises(RuntimeError, match="shared_w"):
        ops.moe_combine(y, w, shared=s, shared_w=sw[:5].contiguous())
    with pytest.raises(RuntimeError, match="shared_w"):
        ops.moe_combine(y, w, shared=s, shared_w=sw.to(BF))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.moe_combine(y, w, shared=s, shared_w=sw.cpu())
    with pytest.raises(ValueError, match="go together"):
        ops.moe_combine(y, w, shared=s)
    with pytest.raises(RuntimeError, match="go together"):
        ops.native().moe_combine(torch.empty(T, H, dtype=BF, device=gpu), y, w, s)


# ------------------------------------------------------------------------------------- the block
SHARED = 384        # != the expert width 128, and 2 x 384 is no multiple of 256 x 2


def _spec(E, k, layers=3, shared=SHARED, step=1):
    return ModelSpec(name="q2moe-t", model_type="qwen2_moe", vocab_size=512, hidden_size=256,
                     intermediate_size=512, num_layers=layers, num_heads=2, num_kv_heads=1,
                     head_dim=128, rms_norm_eps=1e-6, rope_theta=10000.0,
                     max_position_embeddings=4096, bos_token_id=1, eos_token_id=2,
                     attention_bias=True, o_proj_bias=False, num_experts=E,
                     num_experts_per_tok=k, moe_intermediate_size=128,
                     shared_expert_intermediate_size=shared, norm_topk_prob=False,
                     decoder_sparse_step=step)


_BLOCKS = {}


def _block_case(E, k):
    """A CPU MoEMLP with a shared expert, weights of unit-scale products, and 40 rows picked like
    test_moe_gpu.py's: the k-th and (k+1)-th largest fp32 router logits >= 1/16 apart and every
    |logit| < 4, so bf16 logit rounding cannot change any row's routing.  The CPU results are
    computed once."""
    if (E, k) not in _BLOCKS:
        g = torch.Generator().manual_seed(17 * E + k)
        mlp = MoEMLP(_spec(E, k))
        H, I, S = 256, 128, SHARED
        with torch.no_grad():
            mlp.gate.weight.copy_((torch.randn(E + 1, H, generator=g) / H ** 0.5).to(BF))
            mlp.w_gate_up.copy_((torch.randn(E, 2 * I, H, generator=g) / H ** 0.5).to(BF))
            mlp.w_down.copy_((torch.randn(E, H, I, generator=g) / I ** 0.5).to(BF))
            sh = mlp.shared_expert
            sh.gate_up_proj.weight.copy_((torch.randn(2 * S, H, generator=g) / H ** 0.5).to(BF))
            sh.down_proj.weight.copy_((torch.randn(H, S, generator=g) / S ** 0.5).to(BF))
        cand = torch.randn(900, H, generator=g).to(BF)
        lf = cand.float() @ mlp.gate.weight.float().t()
        top = lf[:, :E].sort(-1, descending=True).values
        ok = ((top[:, k - 1] - top[:, k]) >= 1 / 16) & (lf.abs().max(-1).values < 4)
        x = cand[ok][:40].contiguous()
        assert x.shape[0] == 40
        with torch.no_grad():
            want = mlp(x)
            routed = ops.moe_mlp(x, mlp.gate(x)[:, :E].contiguous(), mlp.w_gate_up, mlp.w_down, k,
                                 False)
        _BLOCKS[(E, k)] = (mlp, x, want, routed)
    return _BLOCKS[(E, k)]


def _gpu_block(mlp, E, k, gpu):
    gm = MoEMLP(_spec(E, k), device=gpu)
    gm.load_state_dict(mlp.state_dict())
    return gm


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("T", [1, 4, 40])
@pytest.mark.parametrize("E,k", [(8, 2), (60, 4)])
def test_shared_block_gpu_matches_cpu_path(gpu, E, k, T, fused):
    """1 row (GEMV), 4 and 40 rows; ``fused``: the shared expert's gate|up rows in the fused-SwiGLU
    order the engine uses on the GPU (the same function of x)."""
    mlp, x40, want40, routed40 = _block_case(E, k)
    x, want = x40[:T].contiguous(), want40[:T]
    gm = _gpu_block(mlp, E, k, gpu)
    if fused:
        gm.set_fused_swiglu(True)
        assert gm.shared_expert.fused_swiglu
    xg = x.to(gpu)
    assert gm.gate.weight.shape == (E + 1, 256)
    want_r = ops.moe_route(mlp.gate(x), k, False, num_experts=E)
    got_r = ops.moe_route(gm.gate(xg), k, False, num_experts=E)
    assert torch.equal(got_r.topk_ids.cpu().sort(-1).values, want_r.topk_ids.sort(-1).values)
    with torch.no_grad():
        got = gm(xg)
    torch.cuda.synchronize()
    assert got.dtype == BF and got.shape == (T, 256)
    _close(got, want, ATOL, RTOL, f"shared block E={E} k={k} T={T}")
    # the shared term is a real part of the output: dropping it could not pass
    moved = (want.float() - routed40[:T].float()).abs()
    assert moved.max().item() > 0.1
    assert ((got.float().cpu() - routed40[:T].float()).abs() > ATOL + RTOL * want.float().abs()).any()


def test_shared_block_graph_replay_follows_the_routing(gpu):
    """Captured once with static buffers at T = 12; replayed on three inputs that route
    differently: every replay is bit-equal to the eager call."""
    E, k = 60, 4
    mlp, x40, _, _ = _block_case(E, k)
    gm = _gpu_block(mlp, E, k, gpu)
    T = 12
    inputs = [x40[i * T:(i + 1) * T].to(gpu) for i in range(3)]
    with torch.no_grad():
        eager = [gm(x).clone() for x in inputs]
        routes = [ops.moe_topk(gm.gate(x), k, False, num_experts=E)[0].cpu() for x in inputs]
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
        assert torch.equal(static_y.view(torch.int16), want.view(torch.int16))


# ------------------------------------------------------------------------------------- engine
def _engine(graphs, quantize=False):
    cfg = EngineConfig(model="q2moe-t", pp=1, seed=5, quantize=quantize,
                       cache=CacheConfig(num_blocks=128, block_size=64, max_chunk=256),
                       serve=ServeConfig(max_batch_size=4, max_num_batched_tokens=256,
                                         max_seq_len=512, use_graphs=graphs,
                                         graph_batch_sizes=[1, 2, 4]))
    return LLMEngine(_spec(8, 2, layers=3, shared=256, step=2), device="cuda:0", cfg=cfg)


PROMPTS = [list(range(3, 40)), [7, 8, 9], [11]]


def test_mixed_stack_engine_graph_decode_equals_eager(gpu):
    p = SamplingParams(max_tokens=8, ignore_eos=True)
    eng = _engine(graphs=False)
    layers = eng.executors[0].stage.block.layers
    assert [type(l.mlp) for l in layers] == [LlamaMLP, MoEMLP, LlamaMLP]   # dense, sparse, dense
    assert layers[1].mlp.shared_expert.intermediate_size == 256
    a = [s.output for s in eng.generate(PROMPTS, p)]
    b = [s.output for s in _engine(graphs=True).generate(PROMPTS, p)]
    assert all(len(o) == 8 for o in a) and a == b


@pytest.mark.parametrize("mode", ["fp8_experts", "mxfp4_experts"])
def test_mixed_stack_engine_with_quantised_experts(gpu, mode):
    eng = _engine(graphs=True, quantize=mode)
    layers = eng.executors[0].stage.block.layers
    m = layers[1].mlp
    assert m.is_fp8 if mode == "fp8_experts" else m.is_mxfp4
    assert m.shared_expert.down_proj.weight.dtype == BF and m.gate.weight.dtype == BF
    assert not layers[0].mlp.down_proj.is_fp8 and not layers[0].mlp.down_proj.is_fp4
    out = [s.output for s in eng.generate(PROMPTS, SamplingParams(max_tokens=8, ignore_eos=True))]
    assert all(len(o) == 8 for o in out)
