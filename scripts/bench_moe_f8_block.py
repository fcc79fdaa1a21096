#!/usr/bin/env python3
"""Block-scaled fp8 experts in prefill: the fp8 x fp8 tile GEMM (csrc/kernels/moe_tile_scaled.hip,
MX fp8 activations) against the widening tile GEMM (csrc/kernels/moe_tile_fp8_block.hip, bf16
activations) that runs today.  scripts/bench_moe.py's protocol and scripts/bench_mxfp4.py's helpers.

    python3 scripts/bench_moe_f8_block.py [--models qwen3-30b-a3b,mixtral-8x7b]
                                          [--rows 128,512,2048,8192] [--out DIR]

Per model (one layer's shapes) and row count T, random weights and router logits, every candidate
captured in one hipGraph over ``copies`` layers (own weights, own logits), replays interleaved, 7
rounds, ``KernelPolicy.moe_tile_rows_q = 32`` throughout:

``moe_tile``            route, gate|up and down on the widening kernel (``tiles=True``), combine;
``moe_tile_f8_block``   route, quantise x to MX fp8, gate|up, quantise h, down on the fp8 x fp8
                        kernel (``f8_block=True``), combine -- both quantiser passes inside;
``gate_up_tile`` / ``down_tile``, ``gate_up_tile_f8_block`` / ``down_tile_f8_block``
                        the two products alone (the new kernel's on activations quantised
                        beforehand), ``quant_x`` / ``quant_h`` the quantiser passes alone.

``vs_tile`` is the ratio of the medians, ``vs_tile_range`` the extremes of the per-round ratios,
``separated`` whether the min-max ranges of the two candidates' rounds are apart.  ``accuracy``:
for the first model at T = 2048, the largest absolute error of either path's block output against
fp64 on the UNQUANTISED bf16 activations and the dequantised experts, relative to the reference's
largest magnitude (scripts/moe_mx_accuracy.py's measure).  Result:
``<out>/moe_tile_f8_block.json`` (default ``profiles/moe``)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_mxfp4 as bm  # noqa: E402  (its path set-up makes the package importable too)


def _experts(torch, ops, spec, gen, dev):
    H, I, E = spec.hidden_size, spec.moe_intermediate_size, spec.num_experts
    out = []
    for shape, fan in (((E, 2 * I, H), H), ((E, H, I), I)):
        w = torch.empty(*shape, device=dev, dtype=torch.bfloat16).normal_(0, fan ** -0.5,
                                                                          generator=gen)
        out.append(ops.ExpertWeights.quantize(w, "fp8_block"))
        del w
    return out


def bench(torch, ops, name, rows, res, a):
    from distributed_llm_inference.config import PRESETS
    spec, dev = PRESETS[name], torch.device("cuda", 0)
    H, I, E, k = (spec.hidden_size, spec.moe_intermediate_size, spec.num_experts,
                  spec.num_experts_per_tok)
    copies = 16 if E * 3 * H * I < (1 << 30) else 3      # bench_moe.py's rule at a byte per weight
    gen = torch.Generator(device=dev).manual_seed(1)
    gu, dn = zip(*[_experts(torch, ops, spec, gen, dev) for _ in range(copies)])
    for T in rows:
        x = torch.randn(T, H, device=dev, dtype=torch.bfloat16, generator=gen)
        logits = [torch.randn(T, E, device=dev, generator=gen).to(torch.bfloat16)
                  for _ in range(copies)]
        routes = [ops.moe_route(lg, k, spec.norm_topk_prob) for lg in logits]

        def block(**kw):
            def run(c):
                r = ops.moe_route(logits[c], k, spec.norm_topk_prob)
                h = ops.moe_grouped_gemm(x, gu[c], r, **kw)
                return ops.moe_combine(ops.moe_grouped_gemm(h, dn[c], r, down=True, **kw), r.topk_w)
            return run

        hs = [ops.moe_grouped_gemm(x, gu[c], routes[c], tiles=True) for c in range(copies)]
        ys = [ops.moe_grouped_gemm(hs[c], dn[c], routes[c], down=True, tiles=True)
              for c in range(copies)]
        xq, hq = ops.quant_mx_rows(x), [ops.quant_mx_rows(h) for h in hs]
        hm = [h.clone() for h in hs]
        cands = {
            "moe_tile": block(tiles=True), "moe_tile_f8_block": block(f8_block=True),
            "gate_up_tile": lambda c: ops.moe_grouped_gemm(x, gu[c], routes[c], out=hs[c], tiles=True),
            "down_tile": lambda c: ops.moe_grouped_gemm(hs[c], dn[c], routes[c], down=True,
                                                        out=ys[c], tiles=True),
            "gate_up_tile_f8_block": lambda c: ops.moe_grouped_gemm(xq, gu[c], routes[c], out=hm[c],
                                                                    f8_block=True),
            "down_tile_f8_block": lambda c: ops.moe_grouped_gemm(hq[c], dn[c], routes[c], down=True,
                                                                 out=ys[c], f8_block=True),
            "quant_x": lambda c: ops.quant_mx_rows(x).q,
            "quant_h": lambda c: ops.quant_mx_rows(hm[c]).q}
        graphs = {n: bm._graph(torch, [(lambda c=c, f=f: f(c)) for c in range(copies)])
                  for n, f in cands.items()}
        samples = {n: [] for n in cands}
        reps = 10 if T <= 2048 else 3
        for _ in range(7):                            # interleaved: same box, same minute
            for n in cands:
                samples[n].append(bm._timed(torch, graphs[n], reps) / copies)
        P = T * k
        flop = {"moe": 6 * P * H * I, "gate_up": 4 * P * H * I, "down": 2 * P * H * I}
        row = {"T": T, "mean_rows_per_expert": round(P / E, 2), "copies": copies}
        for n in cands:
            us = statistics.median(samples[n])
            row[n] = {"us": round(us, 2), "min_us": round(min(samples[n]), 2),
                      "max_us": round(max(samples[n]), 2)}
            if n.split("_")[0] != "quant":
                row[n]["TFLOPs"] = round(flop[n.split("_tile")[0]] / us / 1e6, 1)
        for n in ("moe", "gate_up", "down"):
            m, t = row[n + "_tile_f8_block"], row[n + "_tile"]
            per_round = [p / q for p, q in zip(samples[n + "_tile_f8_block"], samples[n + "_tile"])]
            m["vs_tile"] = round(m["us"] / t["us"], 3)
            m["vs_tile_range"] = [round(min(per_round), 3), round(max(per_round), 3)]
            m["separated"] = bool(m["max_us"] < t["min_us"] or t["max_us"] < m["min_us"])
        res["models"].setdefault(name, {"H": H, "I": I, "E": E, "k": k, "rows": {}})
        res["models"][name]["rows"][str(T)] = row
        b = row["moe_tile_f8_block"]
        print(f"{name:14s} T={T:5d} moe_tile {row['moe_tile']['us']:10.1f} us  f8_block "
              f"{b['us']:10.1f} us  x{b['vs_tile']:.3f} ({b['vs_tile_range'][0]:.3f}-"
              f"{b['vs_tile_range'][1]:.3f}, sep {b['separated']})  gate_up "
              f"x{row['gate_up_tile_f8_block']['vs_tile']:.3f}  down "
              f"x{row['down_tile_f8_block']['vs_tile']:.3f}  quant x {row['quant_x']['us']:.1f} "
              f"h {row['quant_h']['us']:.1f}", flush=True)
        bm._save(a, "moe_tile_f8_block.json", res)
        del graphs
        torch.cuda.empty_cache()


def accuracy(torch, ops, name, T):
    from distributed_llm_inference.config import PRESETS
    from distributed_llm_inference.ops.reference import expand_fp8_block_scale
    spec, dev = PRESETS[name], torch.device("cuda", 0)
    H, I, E, k = (spec.hidden_size, spec.moe_intermediate_size, spec.num_experts,
                  spec.num_experts_per_tok)
    gen = torch.Generator(device=dev).manual_seed(1)
    gu, dn = _experts(torch, ops, spec, gen, dev)
    x = torch.randn(T, H, device=dev, dtype=torch.bfloat16, generator=gen)
    r = ops.moe_route(torch.randn(T, E, device=dev, generator=gen).to(torch.bfloat16), k,
                      spec.norm_topk_prob)
    # fp64: per expert, unquantised x, SwiGLU and combine without any rounding in between
    want = torch.zeros(T, H, device=dev, dtype=torch.float64)
    ids, w = r.topk_ids.long(), r.topk_w.double()
    deq = lambda q, e: q.w[e].float().double() * expand_fp8_block_scale(q.scale[e]).double()
    for e in range(E):
        tok, slot = (ids == e).nonzero(as_tuple=True)
        if tok.numel() == 0:
            continue
        g = (x[tok].double() @ deq(gu, e).t()).view(tok.numel(), -1, 2, 16)
        h = (torch.nn.functional.silu(g[:, :, 0]) * g[:, :, 1]).reshape(tok.numel(), I)
        want.index_add_(0, tok, (h @ deq(dn, e).t()) * w[tok, slot][:, None])
    out = {"model": name, "T": T, "max_abs_reference": float(want.abs().max())}
    for n, kw in (("moe_tile", {"tiles": True}), ("moe_tile_f8_block", {"f8_block": True})):
        h = ops.moe_grouped_gemm(x, gu, r, **kw)
        y = ops.moe_combine(ops.moe_grouped_gemm(h, dn, r, down=True, **kw), r.topk_w)
        out[n + "_max_err_rel"] = float((y.double() - want).abs().max() / want.abs().max())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--models", default="qwen3-30b-a3b,mixtral-8x7b")
    ap.add_argument("--rows", default="128,512,2048,8192")
    ap.add_argument("--out", default=os.path.join(bm.REPO, "profiles", "moe"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    torch = bm._torch()
    from distributed_llm_inference import ops
    res = {"unit": "us per MoE layer (median of 7 interleaved rounds of 10 graph replays, 3 past "
                   "T = 2048, over `copies` layers); TFLOPs = 6 T k H I (gate_up: 4, down: 2) / "
                   "time; vs_tile = time / the widening kernel's, vs_tile_range its extremes over "
                   "the rounds; separated = the two candidates' min-max ranges do not overlap",
           "weight_format": "fp8_block", "models": {}}
    models = [m.strip() for m in a.models.split(",")]
    with torch.no_grad(), ops.kernel_policy(moe_tile_rows_q=32):
        res["accuracy"] = accuracy(torch, ops, models[0], 2048)
        print(res["accuracy"], flush=True)
        for name in models:
            bench(torch, ops, name, [int(r) for r in a.rows.split(",")], res, a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
