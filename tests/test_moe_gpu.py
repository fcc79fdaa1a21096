"""The sparse-MoE kernels (csrc/kernels/moe.hip) on the GPU: routing against the reference op,
the grouped GEMM and the combine against an fp32 oracle with explicit ids and sentinel rows, the
MoE block against its CPU path, hipGraph replay with changing routing, and the engine."""
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
SENT = -12345.0
GROWS = 8          # sentinel rows before and after a guarded [rows, width] output


def _close(a, b, atol, rtol=0.0, msg=""):
    """tests/test_fp8_small_gpu.py's comparison."""
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol)
    assert not bad.any(), f"{msg} max err {err.max().item():.4g} at {bad.nonzero()[:5].tolist()}"


ATOL, RTOL = 2e-2, 2e-2     # test_small_gemm_fp8_against_fp32_oracle's: the same numerics class


# ------------------------------------------------------------------------------------- routing
def _perm_logits(T, E, seed):
    """Every row a permutation of E distinct bf16 values (multiples of 1/16 in [-4, 4)): no tie
    at the top-k boundary, or anywhere."""
    g = torch.Generator().manual_seed(seed)
    vals = (torch.arange(E, dtype=torch.float32) - E / 2) / 16
    assert torch.equal(vals.to(BF).float(), vals)
    return torch.stack([vals[torch.randperm(E, generator=g)] for _ in range(T)]).to(BF)


def _bf16_ulp(w):
    return torch.exp2(torch.floor(torch.log2(w)) - 7)


def _assert_grouping_equal(got, want):
    n = int(want.n_tiles)
    assert int(got.n_tiles) == n
    for name in ("expert_count", "expert_offset", "sorted_pairs"):
        assert torch.equal(getattr(got, name).cpu(), getattr(want, name)), name
    for name in ("tile_expert", "tile_start", "tile_rows"):
        assert torch.equal(getattr(got, name)[:n].cpu(), getattr(want, name)[:n]), name


@pytest.mark.parametrize("renorm", [True, False])
@pytest.mark.parametrize("T,E,k", [(1, 8, 2), (5, 128, 8), (33, 128, 8), (67, 8, 2),
                                   (512, 128, 8)])
def test_moe_route_against_reference(gpu, T, E, k, renorm):
    logits = _perm_logits(T, E, 100 * T + E)
    want = ops.moe_route(logits, k, renorm)
    got = ops.moe_route(logits.to(gpu), k, renorm)
    torch.cuda.synchronize()
    assert got.topk_ids.dtype == torch.int32 and got.topk_w.dtype == torch.float32
    assert torch.equal(got.topk_ids.cpu(), want.topk_ids)
    err = (got.topk_w.cpu() - want.topk_w).abs()
    assert bool((err <= _bf16_ulp(want.topk_w)).all()), err.max().item()
    w = got.topk_w.cpu()
    assert torch.equal(w.to(BF).float(), w)                 # the stored weight is a bf16 value
    _assert_grouping_equal(got, want)
    again = ops.moe_route(logits.to(gpu), k, renorm)        # deterministic, bit for bit
    assert torch.equal(again.topk_w, got.topk_w) and torch.equal(again.topk_ids, got.topk_ids)
    _assert_grouping_equal(again, want)


def test_moe_route_tie_rule(gpu):
    """Equal logits: the k lowest expert indices, in order; a tie across the boundary goes to the
    lower index; -0 ties with +0."""
    got = ops.moe_route(torch.zeros(70, 128, dtype=BF, device=gpu), 8, True)
    assert got.topk_ids.cpu().tolist() == [list(range(8))] * 70
    assert got.topk_w.cpu().tolist() == [[0.125] * 8] * 70
    _assert_grouping_equal(got, ops.moe_route(torch.zeros(70, 128, dtype=BF), 8, True))
    assert int(got.n_tiles) == 8 * 3 and got.tile_rows[:3].cpu().tolist() == [32, 32, 6]
    lg = torch.tensor([[1.0, 3.0, 2.0, 2.0, 2.0, 0.0], [-0.0, 0.0, -1.0, 0.0, -0.0, -2.0]]).to(BF)
    want = ops.moe_route(lg, 3, False)
    got = ops.moe_route(lg.to(gpu), 3, False)
    assert got.topk_ids.cpu().tolist() == want.topk_ids.tolist() == [[1, 2, 3], [0, 1, 3]]
    assert bool(((got.topk_w.cpu() - want.topk_w).abs() <= _bf16_ulp(want.topk_w)).all())


# ------------------------------------------------------------------------------------- grouped GEMM
COUNTS = (0, 1, 16, 17, 32, 33, 70, 31)     # rows per expert; 200 pairs = 100 tokens x top-2
_CASES = {}


def _explicit_ids():
    """[100, 2] expert ids giving COUNTS rows per expert, two different experts per token, tokens
    and slots in random order."""
    labels = torch.cat([torch.full((c,), e) for e, c in enumerate(COUNTS)])
    T = labels.numel() // 2
    ids = torch.stack([labels[:T], labels[T:]], 1)
    assert bool((ids[:, 0] != ids[:, 1]).all())
    g = torch.Generator().manual_seed(3)
    ids = ids[torch.randperm(T, generator=g)]
    flip = torch.rand(T, generator=g) < 0.5
    ids[flip] = ids[flip].flip(1)
    assert torch.bincount(ids.reshape(-1), minlength=8).tolist() == list(COUNTS)
    return ids.to(torch.int32)


def _gemm_case(H, I, gpu):
    """Inputs and the fp32 oracle of one (H, I), computed once: per pair, fp32 products of the bf16
    operands with no intermediate rounding."""
    if (H, I) not in _CASES:
        E, k = 8, 2
        g = torch.Generator().manual_seed(H + I)
        ids = _explicit_ids()
        T = ids.shape[0]
        x = torch.randn(T, H, generator=g).to(BF)
        wg = (torch.randn(E, I, H, generator=g) / H ** 0.5).to(BF)
        wu = (torch.randn(E, I, H, generator=g) / H ** 0.5).to(BF)
        wd = (torch.randn(E, H, I, generator=g) / I ** 0.5).to(BF)
        w = torch.rand(T, k, generator=g).to(BF).float()
        e = ids.long()
        xf = x.float()
        gate = torch.einsum("th,tsih->tsi", xf, wg.float()[e])
        up = torch.einsum("th,tsih->tsi", xf, wu.float()[e])
        h = torch.nn.functional.silu(gate) * up                     # [T, k, I], by pair
        y = torch.einsum("tsi,tshi->tsh", h, wd.float()[e])          # [T, k, H]
        out = (w[:, :, None] * y).sum(1)
        w_gate_up = torch.stack([ops.swiglu_interleave(torch.cat([wg[j], wu[j]], 0))
                                 for j in range(E)])
        _CASES[(H, I)] = dict(ids=ids, x=x, w=w, wd=wd, w_gate_up=w_gate_up,
                              h=h.reshape(T * k, I), y=y.reshape(T * k, H), out=out)
    return _CASES[(H, I)]


def _guarded_rows(rows, width, gpu):
    buf = torch.full((GROWS + rows + GROWS, width), SENT, dtype=BF, device=gpu)
    return buf, buf[GROWS:]          # the op sees [rows + GROWS, width]; it may write `rows` rows


def _assert_guards(buf, rows, what):
    assert bool((buf[:GROWS] == SENT).all()), f"{what}: write before the output"
    assert bool((buf[GROWS + rows:] == SENT).all()), f"{what}: write past row P"


@pytest.mark.parametrize("H,I", [(256, 128), (1152, 384)])
def test_grouped_gemm_and_combine_against_fp32_oracle(gpu, H, I):
    """Experts with 0, 1, 16, 17, 32, 33 and 70 rows (one-row tiles, both MFMA row-tile counts,
    exactly full tiles, three tiles); H = 256 / I = 128 give fewer k-steps than the 8 K-split
    waves, 1152 / 384 an uneven split.  h and y carry sentinel rows on both sides."""
    c = _gemm_case(H, I, gpu)
    E, k = 8, 2
    T = c["ids"].shape[0]
    P = T * k
    r = ops.moe_group(c["ids"].to(gpu), c["w"].to(gpu), E)
    want_r = ops.moe_group(c["ids"], c["w"], E)
    _assert_grouping_equal(r, want_r)
    assert r.expert_count.cpu().tolist() == list(COUNTS)
    assert sorted(r.tile_rows[:int(r.n_tiles)].cpu().tolist()) == sorted(
        [1, 16, 17, 32, 32, 1, 32, 32, 6, 31])
    x, wgu, wd = c["x"].to(gpu), c["w_gate_up"].to(gpu), c["wd"].to(gpu)
    pairs = want_r.sorted_pairs.long()

    hbuf, hview = _guarded_rows(P, I, gpu)
    h = ops.moe_grouped_gemm(x, wgu, r, out=hview)
    torch.cuda.synchronize()
    _assert_guards(hbuf, P, "gate|up")
    # row j of h belongs to pair sorted_pairs[j]
    _close(h[:P], c["h"][pairs], ATOL, RTOL, f"gate|up H={H} I={I}")

    ybuf, yview = _guarded_rows(P, H, gpu)
    y = ops.moe_grouped_gemm(h[:P].contiguous(), wd, r, down=True, out=yview)
    torch.cuda.synchronize()
    _assert_guards(ybuf, P, "down")
    _close(y[:P], c["y"], ATOL, RTOL, f"down H={H} I={I}")        # back in pair order
    # ... and exactly the product of the rows the kernel read
    e_of_pair = c["ids"].reshape(-1).long()
    hp = torch.empty(P, I)
    hp[pairs] = h[:P].float().cpu()
    _close(y[:P], torch.einsum("pi,phi->ph", hp, c["wd"].float()[e_of_pair]), ATOL, RTOL, "down/h")

    obuf, oview = _guarded_rows(T, H, gpu)
    out = ops.moe_combine(y, r.topk_w, out=oview[:T])
    torch.cuda.synchronize()
    _assert_guards(obuf, T, "combine")
    _close(out, c["out"], ATOL, RTOL, f"combine H={H} I={I}")
    # fp32 in slot order, one rounding: the reference op on the kernel's y, to a bf16 ulp
    want = ref.moe_combine(y[:P].cpu(), c["w"]).float()
    assert bool(((out.float().cpu() - want).abs() <= 2.0 ** -7 * want.abs()).all())
    # the CPU front end is the same computation within the oracle tolerance
    cpu = ops.moe_combine(ops.moe_grouped_gemm(ops.moe_grouped_gemm(c["x"], c["w_gate_up"], want_r),
                                               c["wd"], want_r, down=True), c["w"])
    _close(out, cpu, ATOL, RTOL, "GPU vs CPU front end")


def test_grouped_gemm_deterministic_and_host_checks(gpu):
    c = _gemm_case(256, 128, gpu)
    r = ops.moe_group(c["ids"].to(gpu), c["w"].to(gpu), 8)
    x, wgu = c["x"].to(gpu), c["w_gate_up"].to(gpu)
    a = ops.moe_grouped_gemm(x, wgu, r)
    b = ops.moe_grouped_gemm(x, wgu, r)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    with pytest.raises(RuntimeError, match="K % 128"):
        ops.moe_grouped_gemm(x[:, :192].contiguous(), wgu[:, :, :192].contiguous(), r)
    with pytest.raises(RuntimeError, match="out"):
        ops.moe_grouped_gemm(x, wgu, r, out=torch.empty(199, 128, dtype=BF, device=gpu))
    with pytest.raises(RuntimeError, match="E <= 256"):
        ops.native().moe_topk(torch.empty(2, 2, dtype=torch.int32, device=gpu),
                              torch.empty(2, 2, device=gpu),
                              torch.zeros(2, 257, dtype=BF, device=gpu), True)
    with pytest.raises(ValueError, match="moe_topk"):
        ops.moe_topk(torch.zeros(2, 8, dtype=BF, device=gpu), 9, True)


# ------------------------------------------------------------------------------------- the block
def _moe_spec(E, k):
    return ModelSpec(name="moe-t", model_type="qwen3_moe", qk_norm=True, vocab_size=512,
                     hidden_size=256, intermediate_size=512, num_layers=2, num_heads=2,
                     num_kv_heads=1, head_dim=128, rms_norm_eps=1e-6, rope_theta=10000.0,
                     max_position_embeddings=4096, bos_token_id=1, eos_token_id=2, num_experts=E,
                     num_experts_per_tok=k, moe_intermediate_size=128, norm_topk_prob=True)


_BLOCKS = {}


def _block_case(E, k):
    """A CPU MoEMLP with weights of unit-scale products, and 40 rows whose CPU fp32 router logits
    have their k-th and (k+1)-th largest >= 1/16 apart with every |logit| < 4 -- picked from
    random candidates, so bf16 logit rounding cannot change the routing of any of them."""
    if (E, k) not in _BLOCKS:
        g = torch.Generator().manual_seed(17 * E + k)
        mlp = MoEMLP(_moe_spec(E, k))
        H, I = 256, 128
        with torch.no_grad():
            mlp.gate.weight.copy_((torch.randn(E, H, generator=g) / H ** 0.5).to(BF))
            mlp.w_gate_up.copy_((torch.randn(E, 2 * I, H, generator=g) / H ** 0.5).to(BF))
            mlp.w_down.copy_((torch.randn(E, H, I, generator=g) / I ** 0.5).to(BF))
        cand = torch.randn(600, H, generator=g).to(BF)
        lf = cand.float() @ mlp.gate.weight.float().t()
        top = lf.sort(-1, descending=True).values
        ok = ((top[:, k - 1] - top[:, k]) >= 1 / 16) & (lf.abs().max(-1).values < 4)
        x = cand[ok][:40].contiguous()
        _BLOCKS[(E, k)] = (mlp, x)
    return _BLOCKS[(E, k)]


@pytest.mark.parametrize("T", [1, 4, 40])
@pytest.mark.parametrize("E,k", [(8, 2), (128, 8)])
def test_moe_block_gpu_matches_cpu_path(gpu, E, k, T):
    mlp, x40 = _block_case(E, k)
    assert x40.shape[0] == 40
    x = x40[:T].contiguous()
    lf = x.float() @ mlp.gate.weight.float().t()                 # the fixture's promise, per row
    top = lf.sort(-1, descending=True).values
    assert bool(((top[:, k - 1] - top[:, k]) >= 1 / 16).all()) and bool((lf.abs() < 4).all())
    gm = MoEMLP(_moe_spec(E, k), device=gpu)
    gm.load_state_dict(mlp.state_dict())
    xg = x.to(gpu)
    want_ids, want_w = ops.moe_topk(mlp.gate(x), k, True)
    got_ids, got_w = ops.moe_topk(gm.gate(xg), k, True)
    assert torch.equal(got_ids.cpu().sort(-1).values, want_ids.sort(-1).values)   # equal routing
    want = mlp(x)
    got = gm(xg)
    torch.cuda.synchronize()
    assert got.dtype == BF and got.shape == (T, 256)
    _close(got, want, ATOL, RTOL, f"MoE block E={E} k={k} T={T}")
    assert want.float().abs().max() > 0.1


def test_moe_block_graph_replay_follows_the_routing(gpu):
    """Captured once with static buffers; replayed on three inputs that route differently: every
    replay is bit-equal to the eager call (all counts are read from device memory)."""
    mlp, x40 = _block_case(128, 8)
    gm = MoEMLP(_moe_spec(128, 8), device=gpu)
    gm.load_state_dict(mlp.state_dict())
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
        assert torch.equal(static_y.view(torch.int16), want.view(torch.int16))


# ------------------------------------------------------------------------------------- engine
def _engine(graphs):
    cfg = EngineConfig(model="moe-t", pp=1, seed=5,
                       cache=CacheConfig(num_blocks=128, block_size=64, max_chunk=256),
                       serve=ServeConfig(max_batch_size=4, max_num_batched_tokens=256,
                                         max_seq_len=512, use_graphs=graphs,
                                         graph_batch_sizes=[1, 2, 4]))
    return LLMEngine(_moe_spec(8, 2), device="cuda:0", cfg=cfg)


def test_moe_engine_graph_decode_equals_eager(gpu):
    prompts = [list(range(3, 40)), [7, 8, 9], [11]]
    p = SamplingParams(max_tokens=8, ignore_eos=True)
    eng = _engine(graphs=False)
    layers = eng.executors[0].stage.block.layers
    assert len(layers) == 2 and all(isinstance(l.mlp, MoEMLP) for l in layers)
    a = [s.output for s in eng.generate(prompts, p)]
    b = [s.output for s in _engine(graphs=True).generate(prompts, p)]
    assert all(len(o) == 8 for o in a) and a == b
    with pytest.raises(ValueError, match="sparse MoE"):
        LLMEngine(_moe_spec(8, 2), device="cuda:0",
                  cfg=EngineConfig(model="moe-t", pp=1, quantize="fp8",
                                   cache=CacheConfig(num_blocks=16),
                                   serve=ServeConfig(max_batch_size=2, max_num_batched_tokens=64,
                                                     max_seq_len=128, use_graphs=False)))
