#!/usr/bin/env python3
"""What MX fp8 activation rounding costs one MoE block with MXFP4 (default) or fp8 (``--fp8``)
experts: the largest absolute error of the block output, relative to the output's largest
magnitude, against an fp64 reference on the UNQUANTISED bf16 activations and the dequantised expert
weights, for the widening tile kernel (moe_tile.hip) and the block-scaled one
(moe_tile_scaled.hip).  Random weights, one layer.

    python3 scripts/moe_mx_accuracy.py [--fp8] [--model qwen3-30b-a3b] [--tokens 2048]

Prints one JSON line."""
import argparse
import json

import bench_mxfp4 as bm  # noqa: F401  (its path set-up makes the package importable)
import torch

from distributed_llm_inference import ops
from distributed_llm_inference.config import PRESETS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="qwen3-30b-a3b")
    ap.add_argument("--tokens", type=int, default=2048)
    ap.add_argument("--fp8", action="store_true", help="fp8 experts (moe_tile_scaled.hip)")
    a = ap.parse_args()
    spec = PRESETS[a.model]
    H, I, E, k = (spec.hidden_size, spec.moe_intermediate_size, spec.num_experts,
                  spec.num_experts_per_tok)
    dev, T = torch.device("cuda", 0), a.tokens
    gen = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s, std=1.0: torch.empty(*s, device=dev, dtype=torch.bfloat16).normal_(0, std, generator=gen)
    fmt, arm = ("fp8", "moe_tile_f8") if a.fp8 else ("mxfp4", "moe_tile_mx")
    gu = ops.ExpertWeights.quantize(rnd(E, 2 * I, H, std=H ** -0.5), fmt)
    dn = ops.ExpertWeights.quantize(rnd(E, H, I, std=I ** -0.5), fmt)
    x, logits = rnd(T, H), rnd(T, E)
    r = ops.moe_route(logits, k, spec.norm_topk_prob)
    # fp64: per expert, unquantised x, SwiGLU and combine without any rounding in between
    want = torch.zeros(T, H, device=dev, dtype=torch.float64)
    ids, w = r.topk_ids.long(), r.topk_w.double()
    # expert e in fp64: MXFP4 widens exactly; fp8 bytes times the row scale without the bf16 rounding
    deq = lambda w, e: (w.w[e].float().double() * w.scale[e].double()[:, None] if a.fp8
                        else w.dequantize(e).double())
    for e in range(E):
        tok, slot = (ids == e).nonzero(as_tuple=True)
        if tok.numel() == 0:
            continue
        g = (x[tok].double() @ deq(gu, e).t()).view(tok.numel(), -1, 2, 16)
        h = (torch.nn.functional.silu(g[:, :, 0]) * g[:, :, 1]).reshape(tok.numel(), I)
        want.index_add_(0, tok, (h @ deq(dn, e).t()) * w[tok, slot][:, None])
    out = {"model": a.model, "experts": fmt, "T": T, "max_abs_reference": float(want.abs().max())}
    with ops.kernel_policy(moe_tile_rows_q=32):
        for name, mx in (("moe_tile", False), (arm, True)):
            h = ops.moe_grouped_gemm(x, gu, r, tiles=True, mx=mx)
            y = ops.moe_combine(ops.moe_grouped_gemm(h, dn, r, down=True, tiles=True, mx=mx), r.topk_w)
            out[name + "_max_err_rel"] = float((y.double() - want).abs().max() / want.abs().max())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
