"""Inputs shared by test_moe_tile_cpu.py and test_moe_tile_gpu.py: the explicit expert ids whose
row counts sit on every edge of a 128-row tiling, and that tiling written out by brute force.
Below them, what the GPU tests of the block-scaled tile kernel (csrc/kernels/moe_tile_scaled.hip:
test_moe_tile_mx_gpu.py, test_moe_tile_f8_gpu.py, test_moe_tile_f8_block_gpu.py) share: the
routing of those ids, guarded output buffers, the fp64 products and the elementwise bound."""
import torch

from distributed_llm_inference import ops

TM = 128                                        # rows per tile of csrc/kernels/moe_tile.hip
# rows per expert: an empty expert, a one-row tile, one row short of a full tile, an exactly full
# tile, a full tile plus one row, three tiles; 800 pairs = 400 tokens x top-2
COUNTS = (0, 1, 127, 128, 129, 300, 33, 82)
E, K_TOP = 8, 2


def explicit_ids():
    """[400, 2] expert ids giving COUNTS rows per expert, two different experts per token, tokens
    and slots in random order (tests/test_moe_gpu.py's construction)."""
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


def brute_force_tiles(ids, num_experts, tile_rows):
    """(expert, start, rows) of every tile, in order: walk the experts, cut each one's run of the
    stably sorted pairs into pieces of at most ``tile_rows``."""
    flat = [min(max(int(v), 0), num_experts - 1) for v in ids.reshape(-1).tolist()]
    tiles, start = [], 0
    for e in range(num_experts):
        left = flat.count(e)
        while left > 0:
            rows = min(left, tile_rows)
            tiles.append((e, start, rows))
            start += rows
            left -= rows
    return tiles


# ------------------------------------------------------- the block-scaled tile kernel's GPU tests
SENT, G = -12345.0, 8       # sentinel value and number of guard rows on either side of an output
ATOL, RTOL = 2e-2, 2e-2     # tests/test_moe_tile_q_gpu.py's oracle tolerance, elementwise


def bits(t):
    return t.contiguous().view(torch.int16)


def close(got, want):
    err = (got.double() - want.double()).abs()
    print(f"max err {float(err.max()):.4g} of {float(want.abs().max()):.4g}")
    return bool((err <= ATOL + RTOL * want.double().abs()).all())


def routing(gpu, ids=None):
    """(ids, the routing tables of ``ids`` on the GPU, sorted_pairs on the CPU)."""
    ids = explicit_ids() if ids is None else ids
    r = ops.moe_group(ids.to(gpu), torch.ones(ids.shape, device=gpu), E)
    return ids, r, r.sorted_pairs.cpu().long()


def guarded(fn, rows, width, gpu):
    """fn(out) on a [rows + G, width] view between sentinel rows; the first ``rows`` rows."""
    buf = torch.full((G + rows + G, width), SENT, dtype=torch.bfloat16, device=gpu)
    fn(buf[G:])
    torch.cuda.synchronize()
    assert bool((buf[:G] == SENT).all()) and bool((buf[G + rows:] == SENT).all()), "guard rows"
    return buf[G:G + rows].cpu()


def products(rows, wd, e_row):
    """fp64 [P, N]: row j of ``rows [P, K]`` times expert ``e_row[j]`` of ``wd [E, N, K]``."""
    out = torch.empty(rows.shape[0], wd.shape[1], dtype=torch.float64)
    for e in range(E):
        out[e_row == e] = rows[e_row == e] @ wd[e].t()
    return out


def swiglu64(gu):
    v = gu.reshape(gu.shape[0], -1, 2, 16)       # swiglu_interleave: 16 gate rows, 16 up rows
    return (torch.nn.functional.silu(v[:, :, 0]) * v[:, :, 1]).reshape(gu.shape[0], -1)
