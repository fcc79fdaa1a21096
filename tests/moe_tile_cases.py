"""Inputs shared by test_moe_tile_cpu.py and test_moe_tile_gpu.py: the explicit expert ids whose
row counts sit on every edge of a 128-row tiling, and that tiling written out by brute force."""
import torch

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
