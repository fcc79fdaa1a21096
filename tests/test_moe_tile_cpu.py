"""The sparse-MoE tile-GEMM switch without a GPU: the ``moe_tile_rows`` policy field and its
refusals, the pure predicate ``ops.moe_uses_tiles``, the reference's 128-row tiling against a
brute-force one, and the CPU path ignoring the field.  The kernel (csrc/kernels/moe_tile.hip) is
pinned by tests/test_moe_tile_gpu.py."""
import pytest
import torch

import moe_tile_cases as mc
from distributed_llm_inference import ops
from distributed_llm_inference.config import KernelPolicy
from distributed_llm_inference.ops import reference as ref

BF = torch.bfloat16


def test_policy_field_default_parse_and_refusals():
    assert KernelPolicy().moe_tile_rows == 0
    assert KernelPolicy().with_overrides("moe_tile_rows=64").moe_tile_rows == 64
    assert KernelPolicy(moe_tile_rows=32).moe_tile_rows == 32
    assert KernelPolicy(moe_tile_rows=1024).moe_tile_rows == 1024
    for bad in (16, 2048, 31, 1025, -64):
        with pytest.raises(ValueError, match="moe_tile_rows"):
            KernelPolicy(moe_tile_rows=bad)
        with pytest.raises(ValueError, match="moe_tile_rows"):
            KernelPolicy().with_overrides(f"moe_tile_rows={bad}")


def test_predicate():
    cuda, cpu = torch.device("cuda:0"), torch.device("cpu")
    assert ops.policy().moe_tile_rows == 0
    assert not ops.moe_uses_tiles(4096, 2, 8, "bf16", cuda)          # policy 0: never
    with ops.kernel_policy(moe_tile_rows=64):
        assert ops.moe_uses_tiles(256, 2, 8, "bf16", cuda)           # 512 pairs = 64 x 8
        assert not ops.moe_uses_tiles(255, 2, 8, "bf16", cuda)       # 510 pairs
        assert ops.moe_uses_tiles(1024, 8, 128, "bf16", "cuda")
        assert not ops.moe_uses_tiles(1023, 8, 128, "bf16", "cuda")
        for fmt in ("fp8", "mxfp4"):
            assert not ops.moe_uses_tiles(4096, 2, 8, fmt, cuda)
        assert not ops.moe_uses_tiles(4096, 2, 8, "bf16", cpu)
        assert not ops.moe_uses_tiles(4096, 2, 8, "bf16", torch.zeros(1).device)
    assert not ops.moe_uses_tiles(256, 2, 8, "bf16", cuda)


def test_reference_tiling_at_128_rows_equals_brute_force():
    ids = mc.explicit_ids()
    T, k = ids.shape
    assert (T, k) == (400, 2)
    want = mc.brute_force_tiles(ids, mc.E, mc.TM)
    assert [t[2] for t in want] == [1, 127, 128, 128, 1, 128, 128, 44, 33, 82]
    cap = ref.moe_tile_capacity(T, mc.E, k, tile_rows=mc.TM)
    assert cap == mc.E + 800 // 128 and len(want) <= cap
    count, offset, pairs, te, ts, tr, nt = ref.moe_group(ids, mc.E, tile_rows=mc.TM)
    n = int(nt)
    assert n == len(want) == 10 and te.numel() == ts.numel() == tr.numel() == cap
    assert list(zip(te[:n].tolist(), ts[:n].tolist(), tr[:n].tolist())) == want
    assert count.tolist() == list(mc.COUNTS)
    # every tile's rows are pairs of its expert, in ascending pair order (the stable sort)
    flat = ids.reshape(-1)
    for e, start, rows in want:
        p = pairs[start:start + rows].long()
        assert bool((flat[p] == e).all()) and bool((p[1:] > p[:-1]).all())
    # ids outside [0, E) are clamped, as in the 32-row grouping
    wild = ids.clone()
    wild[0, 0], wild[1, 1] = -5, 99
    got = ref.moe_group(wild, mc.E, tile_rows=mc.TM)
    wn = int(got[6])
    assert list(zip(got[3][:wn].tolist(), got[4][:wn].tolist(), got[5][:wn].tolist())) == \
        mc.brute_force_tiles(wild, mc.E, mc.TM)
    # a tile size that divides nothing evenly
    g7 = ref.moe_group(ids, mc.E, tile_rows=70)
    n7 = int(g7[6])
    assert list(zip(g7[3][:n7].tolist(), g7[4][:n7].tolist(), g7[5][:n7].tolist())) == \
        mc.brute_force_tiles(ids, mc.E, 70)


def test_reference_defaults_unchanged():
    ids = mc.explicit_ids()
    T, k = ids.shape
    a = ref.moe_group(ids, mc.E)
    b = ref.moe_group(ids, mc.E, tile_rows=32)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    n = int(a[6])
    assert list(zip(a[3][:n].tolist(), a[4][:n].tolist(), a[5][:n].tolist())) == \
        mc.brute_force_tiles(ids, mc.E, 32)
    assert ref.moe_tile_capacity(T, mc.E, k) == ref.moe_tile_capacity(T, mc.E, k, 32) \
        == mc.E + 800 // 32
    assert ops.moe_tile_capacity(3, 128, 8) == 24 and ops.moe_tile_capacity(1, 8, 2) == 2
    r = ops.moe_group(ids, torch.ones(T, k), mc.E)
    assert all(torch.equal(u, v) for u, v in zip(r[2:9], a))


def test_cpu_path_ignores_the_policy():
    g = torch.Generator().manual_seed(5)
    T, E, k, H, I = 256, 8, 2, 128, 128
    x = torch.randn(T, H, generator=g).to(BF)
    logits = torch.randn(T, E, generator=g).to(BF)
    wgu = (torch.randn(E, 2 * I, H, generator=g) / H ** 0.5).to(BF)
    wd = (torch.randn(E, H, I, generator=g) / I ** 0.5).to(BF)
    base = ops.moe_mlp(x, logits, wgu, wd, k, True)
    with ops.kernel_policy(moe_tile_rows=64):
        assert T * k >= 64 * E and not ops.moe_uses_tiles(T, k, E, "bf16", x.device)
        got = ops.moe_mlp(x, logits, wgu, wd, k, True)
        r = ops.moe_route(logits, k, True)
        forced = ops.moe_grouped_gemm(x, wgu, r, tiles=True)     # the CPU path ignores `tiles`
    assert torch.equal(got.view(torch.int16), base.view(torch.int16))
    assert float(base.float().abs().max()) > 0.05
    assert torch.equal(forced.view(torch.int16),
                       ops.moe_grouped_gemm(x, wgu, r, tiles=False).view(torch.int16))
