"""The grouped MFMA tile GEMM for experts with many rows (csrc/kernels/moe_tile.hip) on the GPU:
both epilogues against an fp32 oracle on explicit ids whose row counts sit on every edge of the
128-row tiling (sentinel rows around the outputs), against the weight-streaming kernel, row
independence under a token permutation, determinism and the host checks, the MoE block and the
engine under ``KernelPolicy.moe_tile_rows``, hipGraph replay with changing routing, and quantised
experts staying on the 32-row kernel."""
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
SENT = -12345.0
GROWS = 8          # sentinel rows before and after a guarded [rows, width] output
ATOL, RTOL = 2e-2, 2e-2     # tests/test_moe_gpu.py's: the same numerics class
E, K = mc.E, mc.K_TOP


def _close(a, b, atol, rtol=0.0, msg=""):
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    assert not bad.any(), f"{msg} max err {err.max().item():.4g} at {bad.nonzero()[:5].tolist()}"


def _bits(t):
    return t.contiguous().view(torch.int16)


_CASES = {}


def _gemm_case(H, I):
    """Inputs and the fp32 oracle of one (H, I), computed once: per pair, fp32 products of the bf16
    operands with no intermediate rounding (tests/test_moe_gpu.py's oracle, one expert at a
    time)."""
    if (H, I) not in _CASES:
        g = torch.Generator().manual_seed(H + I)
        ids = mc.explicit_ids()
        T = ids.shape[0]
        x = torch.randn(T, H, generator=g).to(BF)
        wg = (torch.randn(E, I, H, generator=g) / H ** 0.5).to(BF)
        wu = (torch.randn(E, I, H, generator=g) / H ** 0.5).to(BF)
        wd = (torch.randn(E, H, I, generator=g) / I ** 0.5).to(BF)
        w = torch.rand(T, K, generator=g).to(BF).float()
        h = torch.zeros(T, K, I)
        y = torch.zeros(T, K, H)
        for e in range(E):
            t, s = (ids == e).nonzero(as_tuple=True)
            if t.numel() == 0:
                continue
            xe = x[t].float()
            he = torch.nn.functional.silu(xe @ wg[e].float().t()) * (xe @ wu[e].float().t())
            h[t, s] = he
            y[t, s] = he @ wd[e].float().t()
        w_gate_up = torch.stack([ops.swiglu_interleave(torch.cat([wg[j], wu[j]], 0))
                                 for j in range(E)])
        _CASES[(H, I)] = dict(ids=ids, x=x, w=w, wd=wd, w_gate_up=w_gate_up,
                              h=h.reshape(T * K, I), y=y.reshape(T * K, H))
    return _CASES[(H, I)]


def _guarded_rows(rows, width, gpu):
    buf = torch.full((GROWS + rows + GROWS, width), SENT, dtype=BF, device=gpu)
    return buf, buf[GROWS:]          # the op sees [rows + GROWS, width]; it may write `rows` rows


def _assert_guards(buf, rows, what):
    assert bool((buf[:GROWS] == SENT).all()), f"{what}: write before the output"
    assert bool((buf[GROWS + rows:] == SENT).all()), f"{what}: write past row P"


def _run_both(c, gpu, tiles):
    """gate|up and down of case ``c`` into guarded outputs; returns (routing, h [P, I], y [P, H])."""
    T = c["ids"].shape[0]
    P = T * K
    I, H = c["h"].shape[1], c["y"].shape[1]
    r = ops.moe_group(c["ids"].to(gpu), c["w"].to(gpu), E)
    hbuf, hview = _guarded_rows(P, I, gpu)
    h = ops.moe_grouped_gemm(c["x"].to(gpu), c["w_gate_up"].to(gpu), r, out=hview, tiles=tiles)
    torch.cuda.synchronize()
    _assert_guards(hbuf, P, "gate|up")
    ybuf, yview = _guarded_rows(P, H, gpu)
    y = ops.moe_grouped_gemm(h[:P].contiguous(), c["wd"].to(gpu), r, down=True, out=yview,
                             tiles=tiles)
    torch.cuda.synchronize()
    _assert_guards(ybuf, P, "down")
    return r, h[:P], y[:P]


@pytest.mark.parametrize("H,I", [(256, 128), (1152, 384)])
def test_tile_gemm_against_fp32_oracle(gpu, H, I):
    """Experts with 0, 1, 127, 128, 129, 300, 33 and 82 rows: an empty expert, a one-row tile, one
    row short of a full tile, an exactly full tile, a full tile plus one row, three tiles.
    (256, 128): the down product has two k-steps; (1152, 384): 9 blocks of weight rows, three
    256-row interleave groups, 18 / 6 k-steps."""
    c = _gemm_case(H, I)
    P = c["ids"].numel()
    r, h, y = _run_both(c, gpu, tiles=True)
    assert r.expert_count.cpu().tolist() == list(mc.COUNTS)
    assert len(mc.brute_force_tiles(c["ids"], E, mc.TM)) == 10
    pairs = r.sorted_pairs.cpu().long()
    _close(h, c["h"][pairs], ATOL, RTOL, f"gate|up H={H} I={I}")   # row j is pair sorted_pairs[j]
    _close(y, c["y"], ATOL, RTOL, f"down H={H} I={I}")             # back in pair order
    # ... and exactly the product of the rows the kernel read
    e_of_pair = c["ids"].reshape(-1).long()
    hp = torch.empty(P, I)
    hp[pairs] = h.float().cpu()
    want = torch.empty(P, H)
    for e in range(E):
        want[e_of_pair == e] = hp[e_of_pair == e] @ c["wd"][e].float().t()
    _close(y, want, ATOL, RTOL, "down/h")
    assert float(y.float().abs().max()) > 0.5


@pytest.mark.parametrize("H,I", [(256, 128), (1152, 384)])
def test_tile_gemm_against_the_streaming_kernel(gpu, H, I):
    """Both kernels match the oracle and each other within the oracle tolerance (not bit for bit:
    the K summation order differs)."""
    c = _gemm_case(H, I)
    r, ht, yt = _run_both(c, gpu, tiles=True)
    _, hs, ys = _run_both(c, gpu, tiles=False)
    pairs = r.sorted_pairs.cpu().long()
    for name, h, y in (("tiles", ht, yt), ("streaming", hs, ys)):
        _close(h, c["h"][pairs], ATOL, RTOL, f"{name} gate|up")
        _close(y, c["y"], ATOL, RTOL, f"{name} down")
    _close(ht, hs, ATOL, RTOL, "gate|up tiles vs streaming")
    _close(yt, ys, ATOL, RTOL, "down tiles vs streaming")
    # on the same h rows the two down kernels differ by summation order only
    yt2 = ops.moe_grouped_gemm(hs.contiguous(), c["wd"].to(gpu), r, down=True, tiles=True)
    _close(yt2, ys, ATOL, RTOL, "down on equal h")


def test_tile_gemm_rows_are_independent(gpu):
    """A permutation of the tokens moves every pair to another row of another tile (and other
    pairs into the masked tails): each pair's gate|up and down results stay bit for bit."""
    c = _gemm_case(256, 128)
    T = c["ids"].shape[0]
    perm = torch.randperm(T, generator=torch.Generator().manual_seed(9))
    assert not torch.equal(perm, torch.arange(T))
    c2 = dict(c, ids=c["ids"][perm].contiguous(), x=c["x"][perm].contiguous(), w=c["w"][perm])
    r1, h1, y1 = _run_both(c, gpu, tiles=True)
    r2, h2, y2 = _run_both(c2, gpu, tiles=True)
    assert not torch.equal(r1.sorted_pairs, r2.sorted_pairs)

    def by_pair(r, h):
        out = torch.empty_like(h)
        out[r.sorted_pairs.long()] = h
        return out.view(T, K, -1).cpu()

    hp1, hp2 = by_pair(r1, h1), by_pair(r2, h2)
    assert torch.equal(_bits(hp2), _bits(hp1[perm]))                 # token perm[t] is now t
    assert torch.equal(_bits(y2.view(T, K, -1).cpu()), _bits(y1.view(T, K, -1).cpu()[perm]))


def test_tile_gemm_deterministic_and_host_checks(gpu):
    c = _gemm_case(256, 128)
    r = ops.moe_group(c["ids"].to(gpu), c["w"].to(gpu), E)
    x, wgu = c["x"].to(gpu), c["w_gate_up"].to(gpu)
    a = ops.moe_grouped_gemm(x, wgu, r, tiles=True)
    b = ops.moe_grouped_gemm(x, wgu, r, tiles=True)
    assert torch.equal(_bits(a), _bits(b))
    ya = ops.moe_grouped_gemm(a, c["wd"].to(gpu), r, down=True, tiles=True)
    yb = ops.moe_grouped_gemm(a, c["wd"].to(gpu), r, down=True, tiles=True)
    assert torch.equal(_bits(ya), _bits(yb))
    with pytest.raises(RuntimeError, match="K % 64"):
        ops.moe_grouped_gemm(x[:, :96].contiguous(), wgu[:, :, :96].contiguous(), r, tiles=True)
    with pytest.raises(RuntimeError, match="N % 128"):
        ops.moe_grouped_gemm(x, wgu[:, :192].contiguous(), r, tiles=True)
    with pytest.raises(RuntimeError, match="out"):
        ops.moe_grouped_gemm(x, wgu, r, out=torch.empty(799, 128, dtype=BF, device=gpu),
                             tiles=True)
    w8, scale = ops.quantize_expert_weights_fp8(wgu)
    with pytest.raises(ValueError, match="tiles=True needs bf16 expert weights"):
        ops.moe_grouped_gemm(x, w8, r, w_scale=scale, tiles=True)
    with pytest.raises(RuntimeError, match="bf16 expert weights only"):
        ops.native().moe_tile_gemm(a, x, w8, r.sorted_pairs, r.expert_count, r.expert_offset,
                                   x.shape[0], K, 0)


# ------------------------------------------------------------------------------------- the block
def _moe_spec(E_, k):
    return ModelSpec(name="moe-t", model_type="qwen3_moe", qk_norm=True, vocab_size=512,
                     hidden_size=256, intermediate_size=512, num_layers=2, num_heads=2,
                     num_kv_heads=1, head_dim=128, rms_norm_eps=1e-6, rope_theta=10000.0,
                     max_position_embeddings=4096, bos_token_id=1, eos_token_id=2, num_experts=E_,
                     num_experts_per_tok=k, moe_intermediate_size=128, norm_topk_prob=True)


_BLOCKS = {}


def _block_case(E_, k, rows):
    """tests/test_moe_gpu.py's block fixture with ``rows`` rows: a CPU MoEMLP with weights of
    unit-scale products, and rows whose CPU fp32 router logits have their k-th and (k+1)-th
    largest >= 1/16 apart with every |logit| < 4, so bf16 logit rounding cannot change the
    routing of any of them."""
    if (E_, k) not in _BLOCKS:
        g = torch.Generator().manual_seed(17 * E_ + k)
        mlp = MoEMLP(_moe_spec(E_, k))
        H, I = 256, 128
        with torch.no_grad():
            mlp.gate.weight.copy_((torch.randn(E_, H, generator=g) / H ** 0.5).to(BF))
            mlp.w_gate_up.copy_((torch.randn(E_, 2 * I, H, generator=g) / H ** 0.5).to(BF))
            mlp.w_down.copy_((torch.randn(E_, H, I, generator=g) / I ** 0.5).to(BF))
        cand = torch.randn(6000, H, generator=g).to(BF)
        lf = cand.float() @ mlp.gate.weight.float().t()
        top = lf.sort(-1, descending=True).values
        ok = ((top[:, k - 1] - top[:, k]) >= 1 / 16) & (lf.abs().max(-1).values < 4)
        _BLOCKS[(E_, k)] = (mlp, cand[ok].contiguous())
    mlp, x = _BLOCKS[(E_, k)]
    assert x.shape[0] >= rows, x.shape
    return mlp, x[:rows].contiguous()


def _gpu_block(mlp, E_, k, gpu):
    gm = MoEMLP(_moe_spec(E_, k), device=gpu)
    gm.load_state_dict(mlp.state_dict())
    return gm


def _spy(monkeypatch):
    """Counts the native tile launches (their epilogues), and lets them through."""
    nat = ops.native()
    real, calls = nat.moe_tile_gemm, []

    def spy(*a):
        calls.append(int(a[8]))
        return real(*a)

    monkeypatch.setattr(nat, "moe_tile_gemm", spy)
    return calls


@pytest.mark.parametrize("E_,k,T", [(8, 2, 300), (128, 8, 1100)])
def test_moe_block_under_the_policy_matches_cpu_path(gpu, monkeypatch, E_, k, T):
    mlp, x = _block_case(E_, k, T)
    gm = _gpu_block(mlp, E_, k, gpu)
    xg = x.to(gpu)
    calls = _spy(monkeypatch)
    want = mlp(x)
    with ops.kernel_policy(moe_tile_rows=64), torch.no_grad():
        assert ops.moe_uses_tiles(T, k, E_, "bf16", xg.device)
        got = gm(xg)
        torch.cuda.synchronize()
        assert calls == [0, 1]                       # gate|up, then down, on the tile launcher
        _close(got, want, ATOL, RTOL, f"MoE block E={E_} k={k} T={T}")
        assert got.dtype == BF and got.shape == (T, 256) and want.float().abs().max() > 0.1
        # a few rows: below the threshold, the weight-streaming kernel as before
        del calls[:]
        small = gm(xg[:4].contiguous())
    with torch.no_grad():
        base = gm(xg[:4].contiguous())
        off = gm(xg)
    torch.cuda.synchronize()
    assert calls == []
    assert torch.equal(_bits(small), _bits(base))
    _close(off, want, ATOL, RTOL, "policy 0")


def test_moe_block_graph_replay_follows_the_routing(gpu):
    """Captured once under the policy with static buffers; replayed on three inputs that route
    differently: every replay is bit-equal to the eager call (the tiles come from counts in
    device memory)."""
    T = 300
    mlp, x = _block_case(8, 2, 3 * T)
    gm = _gpu_block(mlp, 8, 2, gpu)
    inputs = [x[i * T:(i + 1) * T].to(gpu) for i in range(3)]
    with ops.kernel_policy(moe_tile_rows=64), torch.no_grad():
        eager = [gm(v).clone() for v in inputs]
        routes = [ops.moe_route(gm.gate(v), 2, True).expert_count.cpu() for v in inputs]
        assert not torch.equal(routes[0], routes[1]) and not torch.equal(routes[1], routes[2])
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


def test_quantised_experts_ignore_the_policy(gpu, monkeypatch):
    T = 300
    mlp, x = _block_case(8, 2, T)
    gm = _gpu_block(mlp, 8, 2, gpu)
    gm.quantize_experts_fp8()
    xg = x.to(gpu)
    calls = _spy(monkeypatch)
    with torch.no_grad():
        base = gm(xg)
        with ops.kernel_policy(moe_tile_rows=64):
            assert not ops.moe_uses_tiles(T, 2, 8, "fp8", xg.device)
            got = gm(xg)
    torch.cuda.synchronize()
    assert calls == [] and torch.equal(_bits(got), _bits(base))


# ------------------------------------------------------------------------------------- engine
def _engine(graphs):
    cfg = EngineConfig(model="moe-t", pp=1, seed=5, kernels=KernelPolicy(moe_tile_rows=64),
                       cache=CacheConfig(num_blocks=128, block_size=64, max_chunk=512),
                       serve=ServeConfig(max_batch_size=4, max_num_batched_tokens=512,
                                         max_seq_len=512, use_graphs=graphs,
                                         graph_batch_sizes=[1, 2, 4]))
    return LLMEngine(_moe_spec(8, 2), device="cuda:0", cfg=cfg)


def test_moe_engine_under_the_policy_graph_decode_equals_eager(gpu, monkeypatch):
    """A 300-token prompt: its prefill chunk has 600 pairs over 8 experts, past the threshold of
    64 rows per expert, so the prefill runs on the tile kernel; decode rows stay below it."""
    prompts = [[3 + (7 * i) % 500 for i in range(300)], [7, 8, 9], [11]]
    p = SamplingParams(max_tokens=8, ignore_eos=True)
    calls = _spy(monkeypatch)
    eng = _engine(graphs=False)
    assert ops.policy().moe_tile_rows == 64
    before = len(calls)
    a = [s.output for s in eng.generate(prompts, p)]
    assert calls[before:before + 4] == [0, 1, 0, 1]     # two layers x (gate|up, down)
    b = [s.output for s in _engine(graphs=True).generate(prompts, p)]
    assert all(len(o) == 8 for o in a) and a == b
