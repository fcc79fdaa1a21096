"""Block-scaled fp8 experts ("fp8_block": e4m3 bytes, one fp32 scale per 16 stored rows and 128 k)
on the grouped weight-streaming GEMM (moe_fp8_block.hip) and on the tile GEMM
(moe_tile_fp8_block.hip) against an fp64 oracle, and the MoE block against its CPU path."""
import copy

import pytest
import torch

import moe_tile_cases as tc
from distributed_llm_inference import ops
from distributed_llm_inference.models.llama.modules import MoEMLP
from test_moe_fp8_gpu import (ATOL, COUNTS, E, K_TOP, RTOL, _assert_guards, _close, _e4m3,
                              _explicit_ids, _guarded_rows, _moe_spec)

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
assert (E, K_TOP) == (tc.E, tc.K_TOP)
_CASES = {}


def _scale(N, K):
    """scale[e, group, block] = 2^-p (1 + u / 4), u in [0, 1): p in 0..6 moves by at least 2 (mod
    7) between neighbouring 16-row groups, 128-k blocks and experts, so neighbouring scales are
    more than 2x apart and a scale taken from the wrong place is far outside the tolerance."""
    gi = torch.arange(N // 16)[None, :, None]
    kb = torch.arange(K // 128)[None, None, :]
    p = (2 * gi + 4 * kb + 3 * torch.arange(E)[:, None, None]) % 7
    u = torch.rand(p.shape, generator=torch.Generator().manual_seed(N + K))
    return torch.exp2(-p.float()) * (1 + u / 4)


def _case(kind, H, I):
    """Inputs and fp64 oracle of both products of one shape, computed once: e4m3 weights drawn
    directly, rows of expert e times (w8 * scale) of that expert in fp64; gate|up through an
    unrounded SwiGLU on the interleaved columns, down scattered to the pair index."""
    if (kind, H, I) not in _CASES:
        g = torch.Generator().manual_seed(7 * H + I)
        ids = _explicit_ids() if kind == "stream" else tc.explicit_ids()
        T = ids.shape[0]
        P = T * K_TOP
        flat = ids.reshape(-1).long()
        pairs = torch.sort(flat, stable=True).indices
        owner = flat[pairs]                                   # expert of sorted row j
        prods = []
        for down, (N, K) in ((False, (2 * I, H)), (True, (H, I))):
            w8, scale = _e4m3((E, N, K), g), _scale(N, K)
            wd = w8.double() * scale.double().repeat_interleave(16, 1).repeat_interleave(128, 2)
            x = torch.randn(P if down else T, K, generator=g).to(BF)
            rows = x.double() if down else x.double()[pairs // K_TOP]
            full = torch.cat([rows[owner == e] @ wd[e].t() for e in range(E)])
            if down:
                want = torch.empty_like(full)
                want[pairs] = full
            else:
                v = full.reshape(P, N // 256, 4, 2, 2, 16)
                want = (torch.nn.functional.silu(v[..., 0, :]) * v[..., 1, :]).reshape(P, I)
            prods.append((x, ops.ExpertWeights(w8, scale), want))
        _CASES[(kind, H, I)] = (ids, prods)
    return _CASES[(kind, H, I)]


# stream: the down product at I = 128 is one k-step (seven waves idle), 1152 is 9 steps on 8 waves;
# tiles: K = 128 is one scale block, K = 384 an odd number of them, experts of 0 .. 300 rows
@pytest.mark.parametrize("kind,H,I", [("stream", 256, 128), ("stream", 1152, 384),
                                      ("tiles", 128, 384), ("tiles", 384, 128)])
def test_fp8_block_grouped_gemm_against_fp64_oracle(gpu, kind, H, I):
    ids, prods = _case(kind, H, I)
    assert torch.bincount(ids.reshape(-1).long(), minlength=E).tolist() == list(
        COUNTS if kind == "stream" else tc.COUNTS)
    T = ids.shape[0]
    P = T * K_TOP
    r = ops.moe_group(ids.to(gpu), torch.ones(T, K_TOP, device=gpu), E)
    for down, (x, w, want) in enumerate(prods):
        buf, view = _guarded_rows(P, want.shape[1], gpu)
        wg = ops.ExpertWeights(w.w.to(gpu), w.scale.to(gpu))
        assert wg.format == "fp8_block"
        with ops.kernel_policy(moe_tile_rows_q=64 if kind == "tiles" else 0):
            got = ops.moe_grouped_gemm(x.to(gpu), wg, r, down=bool(down), out=view,
                                       tiles=kind == "tiles")
        torch.cuda.synchronize()
        what = f"{kind} {'down' if down else 'gate|up'} H={H} I={I}"
        _assert_guards(buf, P, what)
        assert want.abs().max() > 1
        _close(got[:P], want, ATOL, RTOL, what)


@pytest.mark.parametrize("T", [1, 4, 40])
def test_fp8_block_moe_block_matches_cpu_path(gpu, T):
    g = torch.Generator().manual_seed(5)
    mlp = MoEMLP(_moe_spec(8, 2))
    H, I = 256, 128
    with torch.no_grad():
        mlp.gate.weight.copy_((torch.randn(8, H, generator=g) / H ** 0.5).to(BF))
        mlp.w_gate_up.copy_((torch.randn(8, 2 * I, H, generator=g) / H ** 0.5).to(BF))
        mlp.w_down.copy_((torch.randn(8, H, I, generator=g) / I ** 0.5).to(BF))
    mlp.quantize_experts_fp8_block()
    assert mlp.is_fp8_block and mlp.experts("w_down").format == "fp8_block"
    # rows whose k-th and (k+1)-th router logits are >= 1/16 apart: bf16 rounding cannot reroute
    cand = torch.randn(600, H, generator=g).to(BF)
    top = (cand.float() @ mlp.gate.weight.float().t()).sort(-1, descending=True).values
    x = cand[(top[:, 1] - top[:, 2]) >= 1 / 16][:T].contiguous()
    with torch.no_grad():
        want = mlp(x)
        got = copy.deepcopy(mlp).to(gpu)(x.to(gpu))
    torch.cuda.synchronize()
    assert got.shape == (T, H) and want.float().abs().max() > 0.1
    _close(got, want, ATOL, RTOL, f"fp8_block MoE block T={T}")
