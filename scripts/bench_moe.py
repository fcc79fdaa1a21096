#!/usr/bin/env python3
"""The sparse-MoE MLP on the grouped weight-streaming GEMM (csrc/kernels/moe.hip) measured against
a loop over the hit experts (docs/kernels.md, "Sparse MoE", quotes the results).
scripts/bench_mxfp4.py's protocol and helpers.

    python3 scripts/bench_moe.py [--models qwen3-30b-a3b,mixtral-8x7b] [--rows 1,8,64,512] [--out DIR]
    python3 scripts/bench_moe.py --fp8 [...]      fp8 expert weights against bf16 -> moe_fp8.json
    python3 scripts/bench_moe.py --fp4 [...]      MXFP4 and fp8 against bf16 -> moe_fp4.json
    python3 scripts/bench_moe.py --shared [...]   Qwen2-MoE's shared expert -> moe_shared.json
    python3 scripts/bench_moe.py --tile [...]     the tile GEMM for many rows per expert -> moe_tile.json
    python3 scripts/bench_moe.py --tile --fp8 | --fp4 [...]   the same on quantised experts
                                                  -> moe_tile_fp8.json / moe_tile_fp4.json

Per model (one layer's shapes) and per decode row count T, with random router logits:

``moe``       ops.moe_mlp: routing (top-k + grouping), gate|up + SwiGLU, down, combine -- every
              count read from device memory, nothing on the host;
``loop``      the baseline: for each hit expert, index_select its tokens, F.linear, the SwiGLU
              kernel, F.linear, scale by the router weight, index_add_ in fp32 -- the routing and
              the per-expert index lists computed on the host beforehand and NOT timed.

Both are captured in one hipGraph over enough layer copies (own weights, own logits) that the
touched expert weights stream from HBM, replays interleaved, median of 7 rounds.  ``moe`` is also
split into its launches (route, gate|up, down, combine), each in a graph of its own.  Reported:
us per layer and expert bytes streamed per second (the hit experts' 3 H I bf16 weights over the
time).  Results: ``<out>/moe.json`` (default ``profiles/moe``).

``--fp8`` measures fp8 expert weights (ops.quantize_expert_weights_fp8 of the same bf16 tensors)
against bf16 instead: candidates ``moe`` / ``gate_up`` / ``down`` and ``moe_fp8`` /
``gate_up_fp8`` / ``down_fp8``, the same graphs over copies, interleaved in the same process.
Reported per fp8 candidate: TB/s on the fp8 bytes (the hit experts' 3 H I bytes and their 2 I + H
fp32 row scales) and the time ratio to its bf16 twin.  Results: ``<out>/moe_fp8.json``.

``--fp4`` adds MXFP4 expert weights (ops.quantize_expert_weights_mxfp4 of the same bf16 tensors):
candidates ``moe_fp4`` / ``gate_up_fp4`` / ``down_fp4`` next to the bf16 and fp8 ones, all nine
interleaved in the same process.  Their TB/s is on 17/32 byte per hit expert weight (nibbles and
block scales); ``vs_fp8`` is the time ratio to the fp8 twin and ``bytes_vs_fp8`` the byte ratio
it is held against.  Results: ``<out>/moe_fp4.json``.

``--shared`` measures the Qwen2-MoE block (models.llama.modules.MoEMLP with a shared expert;
default models qwen1.5-moe-a2.7b and qwen2-57b-a14b, rows 1, 4, 32, 512), two ways on the same
weights, the same graphs over copies, interleaved:

``fused``     the block as the model runs it: the shared gate's row stored behind the router's,
              its sigmoid taken in moe_topk and the shared term added in moe_combine;
``unfused``   the composition it replaces: the router product on the E router rows, a separate
              H -> 1 product with the gate row, ops.moe_mlp without the shared term, then
              ``sigmoid(g) * s`` and the add as elementwise torch ops.

Both run the same shared expert and the same routed experts; the difference is the N = 1
product and the two elementwise passes over [T, H].  Results: ``<out>/moe_shared.json``.

``--tile`` measures the grouped MFMA tile GEMM (csrc/kernels/moe_tile.hip, bf16 experts; default
rows 64, 512, 2048, 8192): ``moe`` (route, both products on the weight-streaming kernel, combine),
``moe_tile`` (the same launches with both products on the tile kernel) and ``loop``, plus the two
products alone on either kernel (``gate_up`` / ``down`` and ``gate_up_tile`` / ``down_tile``), the
same graphs over copies, interleaved.  Reported besides the times: achieved TFLOP/s from the
shapes (6 T k H I per layer), the time ratios, and whether the min-max ranges of the two kernels
are apart (``separated``).  Results: ``<out>/moe_tile.json``.

``--tile --fp8`` / ``--tile --fp4`` run the same protocol on quantised experts
(ops.quantize_expert_weights_fp8 / _mxfp4 of the random bf16 tensors; default rows 128, 512,
2048, 8192): ``moe_tile`` (both products on the quantised tile kernels, forced with ``tiles=True``
under ``KernelPolicy.moe_tile_rows_q``), ``moe`` (the 32-row weight-streaming kernel on the same
quantised experts: what runs without the knob), ``loop`` (the expert loop on the dequantised bf16
weights) and ``moe_tile_bf16`` (the bf16 tile kernel on the dequantised weights, in the same run:
does the quantised kernel follow its bytes?), plus the two products alone on each kernel.
``vs_bf16_tile`` is the time ratio of a quantised tile candidate to its bf16 twin and
``weight_bytes_vs_bf16`` the ratio of the expert bytes behind it.  Results:
``<out>/moe_tile_fp8.json`` / ``<out>/moe_tile_fp4.json``.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_mxfp4 as bm  # noqa: E402  (its path set-up makes the package importable too)


def bench_model(torch, ops, F, name, rows, res, a):
    from distributed_llm_inference.config import PRESETS
    spec = PRESETS[name]
    dev = torch.device("cuda", 0)
    H, I, E, k = (spec.hidden_size, spec.moe_intermediate_size, spec.num_experts,
                  spec.num_experts_per_tok)
    layer_bytes = E * 3 * H * I * 2
    # at T = 1 only k experts per layer are read: enough copies that even those pass the 256 MB
    # Infinity Cache between replays
    copies = 8 if layer_bytes < (2 << 30) else 3
    if a.fp8 and copies == 8:
        copies = 16                                   # ... at half the bytes per expert
    if a.fp4:
        copies = 32 if copies == 8 else 4             # ... at 17/64 of them
    gen = torch.Generator(device=dev).manual_seed(1)
    wgu = [torch.empty(E, 2 * I, H, device=dev, dtype=torch.bfloat16).normal_(0, H ** -0.5, generator=gen)
           for _ in range(copies)]
    wd = [torch.empty(E, H, I, device=dev, dtype=torch.bfloat16).normal_(0, I ** -0.5, generator=gen)
          for _ in range(copies)]
    # per quantised format: (gate|up weights, down weights, their scales, the scale keyword)
    quant = {}
    for fmt, on, fn, kw in (("fp8", a.fp8 or a.fp4, ops.quantize_expert_weights_fp8, "w_scale"),
                            ("fp4", a.fp4, ops.quantize_expert_weights_mxfp4, "w_block_scale")):
        if on:
            q = [(fn(wgu[c]), fn(wd[c])) for c in range(copies)]
            quant[fmt] = ([p[0][0] for p in q], [p[1][0] for p in q], [p[0][1] for p in q],
                          [p[1][1] for p in q], kw)
            del q
    for T in rows:
        x = torch.randn(T, H, device=dev, dtype=torch.bfloat16, generator=gen)
        logits = [torch.randn(T, E, device=dev, generator=gen).to(torch.bfloat16)
                  for _ in range(copies)]
        routes = [ops.moe_route(lg, k, spec.norm_topk_prob) for lg in logits]
        hit_total, loops = 0, []
        for c in range(copies):                      # host-side routing of the baseline: not timed
            ids, w = routes[c].topk_ids.cpu(), routes[c].topk_w.cpu()
            per = []
            for e in ids.unique().tolist():
                tok, slot = (ids == e).nonzero(as_tuple=True)
                per.append((e, tok.to(dev), w[tok, slot].to(dev)[:, None]))
            hit_total += len(per)
            loops.append(per)
        hit = hit_total / copies
        touched = hit * 3 * H * I * 2                 # expert bytes one layer streams

        def moe(c):
            return ops.moe_mlp(x, logits[c], wgu[c], wd[c], k, spec.norm_topk_prob)

        def loop(c):
            acc = torch.zeros(T, H, device=dev, dtype=torch.float32)
            for e, tok, we in loops[c]:
                h = ops.swiglu_interleaved(F.linear(x.index_select(0, tok), wgu[c][e]))
                acc.index_add_(0, tok, F.linear(h, wd[c][e]).float() * we)
            return acc.to(torch.bfloat16)

        err = (moe(0).float() - loop(0).float()).abs().max().item()
        scale = loop(0).float().abs().max().item()
        hs = [ops.moe_grouped_gemm(x, wgu[c], routes[c]) for c in range(copies)]
        ys = [ops.moe_grouped_gemm(hs[c], wd[c], routes[c], down=True) for c in range(copies)]
        parts = {
            "route": lambda c: ops.moe_route(logits[c], k, spec.norm_topk_prob),
            "gate_up": lambda c: ops.moe_grouped_gemm(x, wgu[c], routes[c], out=hs[c]),
            "down": lambda c: ops.moe_grouped_gemm(hs[c], wd[c], routes[c], down=True, out=ys[c]),
            "combine": lambda c: ops.moe_combine(ys[c], routes[c].topk_w),
        }
        cands = {"moe": moe, "loop": loop, **parts}
        errq = {}
        if quant:
            cands = {"moe": moe, "gate_up": parts["gate_up"], "down": parts["down"]}
        for fmt, (qgu, qd, sgu, sd, kw) in quant.items():
            def moe_q(c, qgu=qgu, qd=qd, sgu=sgu, sd=sd):
                return ops.moe_mlp(x, logits[c], ops.ExpertWeights(qgu[c], sgu[c]),
                                   ops.ExpertWeights(qd[c], sd[c]), k, spec.norm_topk_prob)

            hq = [ops.moe_grouped_gemm(x, qgu[c], routes[c], **{kw: sgu[c]}) for c in range(copies)]
            yq = [torch.empty_like(ys[c]) for c in range(copies)]
            cands["moe_" + fmt] = moe_q

            def gate_up_q(c, qgu=qgu, sgu=sgu, kw=kw, hq=hq):
                return ops.moe_grouped_gemm(x, qgu[c], routes[c], out=hq[c], **{kw: sgu[c]})

            def down_q(c, qd=qd, sd=sd, kw=kw, hq=hq, yq=yq):
                return ops.moe_grouped_gemm(hq[c], qd[c], routes[c], down=True, out=yq[c],
                                            **{kw: sd[c]})

            cands["gate_up_" + fmt] = gate_up_q
            cands["down_" + fmt] = down_q
            errq[fmt] = (moe_q(0).float() - moe(0).float()).abs().max().item()
        graphs = {n: bm._graph(torch, [(lambda c=c, f=f: f(c)) for c in range(copies)])
                  for n, f in cands.items()}
        samples = {n: [] for n in cands}
        for _ in range(7):                            # interleaved: same box, same minute
            for n in cands:
                samples[n].append(bm._timed(torch, graphs[n], 10) / copies)
        row = {"T": T, "hit_experts_per_layer": round(hit, 2), "copies": copies,
               "expert_MB_touched": round(touched / 1e6, 1),
               "max_abs_diff_moe_vs_loop": round(err, 4), "max_abs_loop": round(scale, 3)}
        for n in cands:
            us = statistics.median(samples[n])
            row[n] = {"us": round(us, 2), "min_us": round(min(samples[n]), 2),
                      "max_us": round(max(samples[n]), 2)}
        res["models"].setdefault(name, {"H": H, "I": I, "E": E, "k": k, "rows": {}})
        res["models"][name]["rows"][str(T)] = row
        if quant:
            # bytes of one layer's hit experts: gate|up is 2 / 3 of the weights and 2 I of the rows
            byt = {"moe": touched, "gate_up": touched * 2 / 3, "down": touched / 3}
            sc = {"moe": hit * (2 * I + H) * 4, "gate_up": hit * 2 * I * 4, "down": hit * H * 4}
            for fmt in quant:
                row[f"max_abs_diff_{fmt}_vs_bf16"] = round(errq[fmt], 4)
            for n in ("moe", "gate_up", "down"):
                row[n]["expert_TBps"] = round(byt[n] / row[n]["us"] / 1e6, 3)
                f8 = row[n + "_fp8"]
                f8["expert_TBps"] = round((byt[n] / 2 + sc[n]) / f8["us"] / 1e6, 3)
                f8["vs_bf16"] = round(f8["us"] / row[n]["us"], 3)
                if a.fp4:   # 17/32 byte per weight: the nibbles and one scale byte per 32
                    f4 = row[n + "_fp4"]
                    f4["expert_TBps"] = round(byt[n] * 17 / 64 / f4["us"] / 1e6, 3)
                    f4["vs_bf16"] = round(f4["us"] / row[n]["us"], 3)
                    f4["vs_fp8"] = round(f4["us"] / f8["us"], 3)
                    f4["bytes_vs_fp8"] = round(byt[n] * 17 / 64 / (byt[n] / 2 + sc[n]), 3)
            last = "fp4" if a.fp4 else "fp8"
            print(f"{name:14s} T={T:4d} hit {hit:6.1f}  " + "  ".join(
                f"{n} " + " / ".join(f"{row[n + s]['us']:.1f}"
                                     for s in [""] + ["_" + f for f in quant])
                + f" us ({row[n + '_' + last]['expert_TBps']:.2f} TB/s, "
                f"x{row[n + '_' + last]['vs_bf16']:.3f}"
                + (f", x{row[n + '_fp4']['vs_fp8']:.3f} of fp8" if a.fp4 else "") + ")"
                for n in ("moe", "gate_up", "down")), flush=True)
            bm._save(a, "moe_fp4.json" if a.fp4 else "moe_fp8.json", res)
            del graphs
            torch.cuda.empty_cache()
            continue
        for n in ("moe", "loop"):
            row[n]["expert_TBps"] = round(touched / row[n]["us"] / 1e6, 3)
        row["moe_vs_loop"] = round(row["moe"]["us"] / row["loop"]["us"], 3)
        print(f"{name:14s} T={T:4d} hit {hit:6.1f}  moe {row['moe']['us']:9.2f} us "
              f"({row['moe']['expert_TBps']:.2f} TB/s)  loop {row['loop']['us']:9.2f} us "
              f"({row['loop']['expert_TBps']:.2f} TB/s)  moe/loop {row['moe_vs_loop']:.3f}  "
              + "  ".join(f"{n} {row[n]['us']:.1f}" for n in parts), flush=True)
        bm._save(a, "moe.json", res)
        del graphs
        torch.cuda.empty_cache()


def bench_tile(torch, ops, F, name, rows, res, a):
    """The grouped MFMA tile GEMM against the weight-streaming kernel and the expert loop (module
    docstring, ``--tile``)."""
    from distributed_llm_inference.config import PRESETS
    spec = PRESETS[name]
    dev = torch.device("cuda", 0)
    H, I, E, k = (spec.hidden_size, spec.moe_intermediate_size, spec.num_experts,
                  spec.num_experts_per_tok)
    copies = 8 if E * 3 * H * I * 2 < (2 << 30) else 3   # bench_model's rule
    gen = torch.Generator(device=dev).manual_seed(1)
    wgu = [torch.empty(E, 2 * I, H, device=dev, dtype=torch.bfloat16).normal_(0, H ** -0.5, generator=gen)
           for _ in range(copies)]
    wd = [torch.empty(E, H, I, device=dev, dtype=torch.bfloat16).normal_(0, I ** -0.5, generator=gen)
          for _ in range(copies)]
    for T in rows:
        x = torch.randn(T, H, device=dev, dtype=torch.bfloat16, generator=gen)
        logits = [torch.randn(T, E, device=dev, generator=gen).to(torch.bfloat16)
                  for _ in range(copies)]
        routes = [ops.moe_route(lg, k, spec.norm_topk_prob) for lg in logits]
        hit_total, loops = 0, []
        for c in range(copies):                      # host-side routing of the baseline: not timed
            ids, w = routes[c].topk_ids.cpu(), routes[c].topk_w.cpu()
            per = []
            for e in ids.unique().tolist():
                tok, slot = (ids == e).nonzero(as_tuple=True)
                per.append((e, tok.to(dev), w[tok, slot].to(dev)[:, None]))
            hit_total += len(per)
            loops.append(per)
        hit = hit_total / copies
        touched = hit * 3 * H * I * 2                 # expert bytes one layer streams

        def moe_with(tiles):
            def run(c):
                r = ops.moe_route(logits[c], k, spec.norm_topk_prob)
                h = ops.moe_grouped_gemm(x, wgu[c], r, tiles=tiles)
                y = ops.moe_grouped_gemm(h, wd[c], r, down=True, tiles=tiles)
                return ops.moe_combine(y, r.topk_w)
            return run

        def loop(c):
            acc = torch.zeros(T, H, device=dev, dtype=torch.float32)
            for e, tok, we in loops[c]:
                h = ops.swiglu_interleaved(F.linear(x.index_select(0, tok), wgu[c][e]))
                acc.index_add_(0, tok, F.linear(h, wd[c][e]).float() * we)
            return acc.to(torch.bfloat16)

        ref = loop(0).float()
        err = {n: (moe_with(t)(0).float() - ref).abs().max().item()
               for n, t in (("moe", False), ("moe_tile", True))}
        hs = [ops.moe_grouped_gemm(x, wgu[c], routes[c], tiles=False) for c in range(copies)]
        ys = [ops.moe_grouped_gemm(hs[c], wd[c], routes[c], down=True, tiles=False)
              for c in range(copies)]
        cands = {"moe": moe_with(False), "moe_tile": moe_with(True), "loop": loop}
        for n, t in (("", False), ("_tile", True)):
            cands["gate_up" + n] = lambda c, t=t: ops.moe_grouped_gemm(
                x, wgu[c], routes[c], out=hs[c], tiles=t)
            cands["down" + n] = lambda c, t=t: ops.moe_grouped_gemm(
                hs[c], wd[c], routes[c], down=True, out=ys[c], tiles=t)
        graphs = {n: bm._graph(torch, [(lambda c=c, f=f: f(c)) for c in range(copies)])
                  for n, f in cands.items()}
        samples = {n: [] for n in cands}
        reps = 10 if T <= 2048 else 3                 # the 32-row kernel takes tens of ms up there
        for _ in range(7):                            # interleaved: same box, same minute
            for n in cands:
                samples[n].append(bm._timed(torch, graphs[n], reps) / copies)
        P = T * k
        flop = {"moe": 6 * P * H * I, "gate_up": 4 * P * H * I, "down": 2 * P * H * I}
        row = {"T": T, "mean_rows_per_expert": round(P / E, 2),
               "hit_experts_per_layer": round(hit, 2), "copies": copies,
               "expert_MB_touched": round(touched / 1e6, 1),
               "max_abs_diff_vs_loop": {n: round(v, 4) for n, v in err.items()},
               "max_abs_loop": round(ref.abs().max().item(), 3)}
        for n in cands:
            us = statistics.median(samples[n])
            row[n] = {"us": round(us, 2), "min_us": round(min(samples[n]), 2),
                      "max_us": round(max(samples[n]), 2),
                      "TFLOPs": round(flop[n.replace("_tile", "").replace("loop", "moe")]
                                      / us / 1e6, 1)}
        for n in ("moe", "gate_up", "down"):
            t, s = row[n + "_tile"], row[n]
            t["vs_" + n] = round(t["us"] / s["us"], 3)
            # the min-max ranges of the rounds do not overlap
            t["separated"] = bool(t["max_us"] < s["min_us"] or s["max_us"] < t["min_us"])
        row["moe_tile"]["vs_loop"] = round(row["moe_tile"]["us"] / row["loop"]["us"], 3)
        row["moe"]["vs_loop"] = round(row["moe"]["us"] / row["loop"]["us"], 3)
        res["models"].setdefault(name, {"H": H, "I": I, "E": E, "k": k, "rows": {}})
        res["models"][name]["rows"][str(T)] = row
        print(f"{name:14s} T={T:5d} rows/expert {P / E:7.1f}  moe {row['moe']['us']:10.1f} us  "
              f"moe_tile {row['moe_tile']['us']:10.1f} us ({row['moe_tile']['TFLOPs']:.0f} TF, "
              f"x{row['moe_tile']['vs_moe']:.3f} of moe, x{row['moe_tile']['vs_loop']:.3f} of loop)"
              f"  loop {row['loop']['us']:10.1f} us  gate_up {row['gate_up']['us']:.1f} -> "
              f"{row['gate_up_tile']['us']:.1f}  down {row['down']['us']:.1f} -> "
              f"{row['down_tile']['us']:.1f}", flush=True)
        bm._save(a, "moe_tile.json", res)
        del graphs
        torch.cuda.empty_cache()
    del wgu, wd
    torch.cuda.empty_cache()


def bench_tile_q(torch, ops, F, name, rows, res, a):
    """bench_tile's protocol on fp8 (``--fp8``) or MXFP4 (``--fp4``) experts (module docstring,
    ``--tile --fp8`` / ``--tile --fp4``)."""
    from distributed_llm_inference.config import PRESETS
    spec = PRESETS[name]
    dev = torch.device("cuda", 0)
    H, I, E, k = (spec.hidden_size, spec.moe_intermediate_size, spec.num_experts,
                  spec.num_experts_per_tok)
    fmt = "fp4" if a.fp4 else "fp8"
    kw = "w_block_scale" if a.fp4 else "w_scale"
    quantise = ops.quantize_expert_weights_mxfp4 if a.fp4 else ops.quantize_expert_weights_fp8
    copies = 8 if E * 3 * H * I * 2 < (2 << 30) else 3   # bench_model's rule, on the bf16 bytes
    gen = torch.Generator(device=dev).manual_seed(1)

    def dequantised(q, s):
        out = torch.empty(q.shape[0], q.shape[1], s.shape[2] * 32 if a.fp4 else q.shape[2],
                          device=dev, dtype=torch.bfloat16)
        for e in range(q.shape[0]):                   # one expert at a time: a small temporary
            if a.fp4:
                ops.dequantize_mxfp4(q[e], s[e], out=out[e])
            else:
                out[e] = (q[e].float() * s[e][:, None]).to(torch.bfloat16)
        return out

    # per copy: the quantised experts and their dequantised bf16 twin (the original is dropped)
    qgu, sgu, qd, sd, wgu, wd = [], [], [], [], [], []
    for _ in range(copies):
        for shape, fan, qs, ss, ws in (((E, 2 * I, H), H, qgu, sgu, wgu), ((E, H, I), I, qd, sd, wd)):
            w = torch.empty(*shape, device=dev, dtype=torch.bfloat16).normal_(0, fan ** -0.5,
                                                                              generator=gen)
            q, s = quantise(w)
            del w
            qs.append(q)
            ss.append(s)
            ws.append(dequantised(q, s))
    # expert bytes per bf16 byte: fp8 adds one fp32 scale per row, MXFP4 is 17/32 byte per weight
    byte_ratio = 17 / 64 if a.fp4 else 0.5 + (2 * I + H) * 4 / (3 * H * I * 2)
    for T in rows:
        x = torch.randn(T, H, device=dev, dtype=torch.bfloat16, generator=gen)
        logits = [torch.randn(T, E, device=dev, generator=gen).to(torch.bfloat16)
                  for _ in range(copies)]
        routes = [ops.moe_route(lg, k, spec.norm_topk_prob) for lg in logits]
        hit_total, loops = 0, []
        for c in range(copies):                      # host-side routing of the baseline: not timed
            ids, w = routes[c].topk_ids.cpu(), routes[c].topk_w.cpu()
            per = []
            for e in ids.unique().tolist():
                tok, slot = (ids == e).nonzero(as_tuple=True)
                per.append((e, tok.to(dev), w[tok, slot].to(dev)[:, None]))
            hit_total += len(per)
            loops.append(per)
        hit = hit_total / copies
        touched = hit * 3 * H * I * 2 * byte_ratio    # expert bytes one layer streams

        def moe_with(tiles, bf16=False):
            def run(c):
                r = ops.moe_route(logits[c], k, spec.norm_topk_prob)
                if bf16:
                    h = ops.moe_grouped_gemm(x, wgu[c], r, tiles=tiles)
                    y = ops.moe_grouped_gemm(h, wd[c], r, down=True, tiles=tiles)
                else:
                    h = ops.moe_grouped_gemm(x, qgu[c], r, tiles=tiles, **{kw: sgu[c]})
                    y = ops.moe_grouped_gemm(h, qd[c], r, down=True, tiles=tiles, **{kw: sd[c]})
                return ops.moe_combine(y, r.topk_w)
            return run

        def loop(c):
            acc = torch.zeros(T, H, device=dev, dtype=torch.float32)
            for e, tok, we in loops[c]:
                h = ops.swiglu_interleaved(F.linear(x.index_select(0, tok), wgu[c][e]))
                acc.index_add_(0, tok, F.linear(h, wd[c][e]).float() * we)
            return acc.to(torch.bfloat16)

        ref = loop(0).float()
        err = {n: (f(0).float() - ref).abs().max().item()
               for n, f in (("moe", moe_with(False)), ("moe_tile", moe_with(True)),
                            ("moe_tile_bf16", moe_with(True, bf16=True)))}
        hs = [ops.moe_grouped_gemm(x, qgu[c], routes[c], tiles=False, **{kw: sgu[c]})
              for c in range(copies)]
        ys = [ops.moe_grouped_gemm(hs[c], qd[c], routes[c], down=True, tiles=False, **{kw: sd[c]})
              for c in range(copies)]
        cands = {"moe": moe_with(False), "moe_tile": moe_with(True), "loop": loop,
                 "moe_tile_bf16": moe_with(True, bf16=True)}
        for n, t in (("", False), ("_tile", True)):
            cands["gate_up" + n] = lambda c, t=t: ops.moe_grouped_gemm(
                x, qgu[c], routes[c], out=hs[c], tiles=t, **{kw: sgu[c]})
            cands["down" + n] = lambda c, t=t: ops.moe_grouped_gemm(
                hs[c], qd[c], routes[c], down=True, out=ys[c], tiles=t, **{kw: sd[c]})
        cands["gate_up_tile_bf16"] = lambda c: ops.moe_grouped_gemm(
            x, wgu[c], routes[c], out=hs[c], tiles=True)
        cands["down_tile_bf16"] = lambda c: ops.moe_grouped_gemm(
            hs[c], wd[c], routes[c], down=True, out=ys[c], tiles=True)
        graphs = {n: bm._graph(torch, [(lambda c=c, f=f: f(c)) for c in range(copies)])
                  for n, f in cands.items()}
        samples = {n: [] for n in cands}
        reps = 10 if T <= 2048 else 3                 # the 32-row kernel takes tens of ms up there
        for _ in range(7):                            # interleaved: same box, same minute
            for n in cands:
                samples[n].append(bm._timed(torch, graphs[n], reps) / copies)
        P = T * k
        flop = {"moe": 6 * P * H * I, "gate_up": 4 * P * H * I, "down": 2 * P * H * I}
        row = {"T": T, "mean_rows_per_expert": round(P / E, 2),
               "hit_experts_per_layer": round(hit, 2), "copies": copies,
               "expert_MB_touched": round(touched / 1e6, 1),
               "weight_bytes_vs_bf16": round(byte_ratio, 4),
               "max_abs_diff_vs_loop": {n: round(v, 4) for n, v in err.items()},
               "max_abs_loop": round(ref.abs().max().item(), 3)}
        for n in cands:
            us = statistics.median(samples[n])
            base = n.replace("_tile_bf16", "").replace("_tile", "").replace("loop", "moe")
            row[n] = {"us": round(us, 2), "min_us": round(min(samples[n]), 2),
                      "max_us": round(max(samples[n]), 2),
                      "TFLOPs": round(flop[base] / us / 1e6, 1)}
        for n in ("moe", "gate_up", "down"):
            t, s, b = row[n + "_tile"], row[n], row[n + "_tile_bf16"]
            t["vs_" + n] = round(t["us"] / s["us"], 3)
            # the min-max ranges of the rounds do not overlap
            t["separated"] = bool(t["max_us"] < s["min_us"] or s["max_us"] < t["min_us"])
            t["vs_bf16_tile"] = round(t["us"] / b["us"], 3)
            t["separated_from_bf16_tile"] = bool(t["max_us"] < b["min_us"]
                                                 or b["max_us"] < t["min_us"])
        row["moe_tile"]["vs_loop"] = round(row["moe_tile"]["us"] / row["loop"]["us"], 3)
        row["moe"]["vs_loop"] = round(row["moe"]["us"] / row["loop"]["us"], 3)
        res["models"].setdefault(name, {"H": H, "I": I, "E": E, "k": k, "rows": {}})
        res["models"][name]["rows"][str(T)] = row
        print(f"{name:14s} {fmt} T={T:5d} rows/expert {P / E:7.1f}  moe {row['moe']['us']:10.1f} us"
              f"  moe_tile {row['moe_tile']['us']:10.1f} us ({row['moe_tile']['TFLOPs']:.0f} TF, "
              f"x{row['moe_tile']['vs_moe']:.3f} of moe, sep {row['moe_tile']['separated']}, "
              f"x{row['moe_tile']['vs_bf16_tile']:.3f} of the bf16 tiles "
              f"{row['moe_tile_bf16']['us']:.1f})  loop {row['loop']['us']:10.1f} us  gate_up "
              f"{row['gate_up']['us']:.1f} -> {row['gate_up_tile']['us']:.1f} "
              f"(bf16 {row['gate_up_tile_bf16']['us']:.1f})  down {row['down']['us']:.1f} -> "
              f"{row['down_tile']['us']:.1f} (bf16 {row['down_tile_bf16']['us']:.1f})", flush=True)
        bm._save(a, f"moe_tile_{fmt}.json", res)
        del graphs
        torch.cuda.empty_cache()
    del qgu, sgu, qd, sd, wgu, wd
    torch.cuda.empty_cache()


def bench_shared(torch, ops, F, name, rows, res, a):
    """The Qwen2-MoE block with its shared expert, fused against unfused (module docstring)."""
    from distributed_llm_inference.config import PRESETS
    from distributed_llm_inference.models.common import Linear
    from distributed_llm_inference.models.llama.modules import MoEMLP
    spec = PRESETS[name]
    dev = torch.device("cuda", 0)
    H, I, E, k, S = (spec.hidden_size, spec.moe_intermediate_size, spec.num_experts,
                     spec.num_experts_per_tok, spec.shared_expert_intermediate_size)
    layer_bytes = (E * 3 * H * I + 3 * H * S) * 2
    copies = 8 if layer_bytes < (2 << 30) else 3      # bench_model's rule: past the Infinity Cache
    gen = torch.Generator(device=dev).manual_seed(1)
    blocks, routers, gates = [], [], []
    for _ in range(copies):
        m = MoEMLP(spec, device=dev)
        for p_, fan in ((m.gate.weight, H), (m.w_gate_up, H), (m.w_down, I),
                        (m.shared_expert.gate_up_proj.weight, H),
                        (m.shared_expert.down_proj.weight, S)):
            p_.data.normal_(0, fan ** -0.5, generator=gen)
        m.set_fused_swiglu(True)                      # the engine's setting on the GPU
        # the unfused composition's two products, on views of the same weight
        r, g1 = Linear(H, E, device="meta"), Linear(H, 1, device="meta")
        r.weight = torch.nn.Parameter(m.gate.weight[:E], requires_grad=False)
        g1.weight = torch.nn.Parameter(m.gate.weight[E:], requires_grad=False)
        blocks.append(m)
        routers.append(r)
        gates.append(g1)
    for T in rows:
        x = torch.randn(T, H, device=dev, dtype=torch.bfloat16, generator=gen)

        def fused(c):
            return blocks[c](x)

        def unfused(c):
            m = blocks[c]
            s = m.shared_expert(x)
            y = ops.moe_mlp(x, routers[c](x), m.w_gate_up, m.w_down, k, spec.norm_topk_prob)
            return y + torch.sigmoid(gates[c](x)) * s

        hit = sum(ops.moe_topk(routers[c](x), k, spec.norm_topk_prob)[0].unique().numel()
                  for c in range(copies)) / copies
        f0, u0 = fused(0).float(), unfused(0).float()
        cands = {"fused": fused, "unfused": unfused,
                 "shared_expert": lambda c: blocks[c].shared_expert(x)}
        graphs = {n: bm._graph(torch, [(lambda c=c, f=f: f(c)) for c in range(copies)])
                  for n, f in cands.items()}
        samples = {n: [] for n in cands}
        for _ in range(7):                            # interleaved: same box, same minute
            for n in cands:
                samples[n].append(bm._timed(torch, graphs[n], 10) / copies)
        touched = (hit * 3 * H * I + 3 * H * S) * 2   # hit experts + the shared expert, bf16
        row = {"T": T, "hit_experts_per_layer": round(hit, 2), "copies": copies,
               "weight_MB_touched": round(touched / 1e6, 1),
               "max_abs_diff_fused_vs_unfused": round((f0 - u0).abs().max().item(), 4),
               "max_abs_unfused": round(u0.abs().max().item(), 3)}
        for n in cands:
            us = statistics.median(samples[n])
            row[n] = {"us": round(us, 2), "min_us": round(min(samples[n]), 2),
                      "max_us": round(max(samples[n]), 2)}
        for n in ("fused", "unfused"):
            row[n]["weight_TBps"] = round(touched / row[n]["us"] / 1e6, 3)
        row["fused_vs_unfused"] = round(row["fused"]["us"] / row["unfused"]["us"], 3)
        res["models"].setdefault(name, {"H": H, "I": I, "E": E, "k": k, "shared": S, "rows": {}})
        res["models"][name]["rows"][str(T)] = row
        print(f"{name:18s} T={T:4d} hit {hit:5.1f}  fused {row['fused']['us']:9.2f} us "
              f"({row['fused']['weight_TBps']:.2f} TB/s)  unfused {row['unfused']['us']:9.2f} us  "
              f"fused/unfused {row['fused_vs_unfused']:.3f}  shared expert alone "
              f"{row['shared_expert']['us']:.1f} us", flush=True)
        bm._save(a, "moe_shared.json", res)
        del graphs
        torch.cuda.empty_cache()
    del blocks, routers, gates
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--models", default=None,
                    help="default qwen3-30b-a3b,mixtral-8x7b (--shared: qwen1.5-moe-a2.7b,"
                         "qwen2-57b-a14b)")
    ap.add_argument("--rows", default=None, help="default 1,8,64,512 (--shared: 1,4,32,512)")
    ap.add_argument("--shared", action="store_true",
                    help="Qwen2-MoE's shared expert: the fused block against the unfused "
                         "composition (moe_shared.json)")
    ap.add_argument("--out", default=os.path.join(bm.REPO, "profiles", "moe"))
    ap.add_argument("--fp8", action="store_true",
                    help="fp8 expert weights against bf16 (moe_fp8.json) instead of moe against loop")
    ap.add_argument("--fp4", action="store_true",
                    help="MXFP4 and fp8 expert weights against bf16 (moe_fp4.json)")
    ap.add_argument("--tile", action="store_true",
                    help="the tile GEMM for many rows per expert against the weight-streaming "
                         "kernel and the loop (moe_tile.json)")
    ap.add_argument("--note", default="", help="free text kept in the result file (--fp8 / --fp4)")
    a = ap.parse_args()
    if a.shared and (a.fp8 or a.fp4):
        ap.error("--shared measures bf16 weights: not with --fp8 / --fp4")
    if a.tile and a.fp8 and a.fp4:
        ap.error("--tile measures one quantised format per run: --fp8 or --fp4")
    if a.shared and a.tile:
        ap.error("--shared or --tile, not both")
    a.models = a.models or ("qwen1.5-moe-a2.7b,qwen2-57b-a14b" if a.shared
                            else "qwen3-30b-a3b,mixtral-8x7b")
    tile_q = a.tile and (a.fp8 or a.fp4)
    a.rows = a.rows or ("1,4,32,512" if a.shared else "128,512,2048,8192" if tile_q
                        else "64,512,2048,8192" if a.tile else "1,8,64,512")
    os.makedirs(a.out, exist_ok=True)
    torch = bm._torch()
    import torch.nn.functional as F
    from distributed_llm_inference import ops
    res = {"unit": "us per MoE layer (median of 7 interleaved rounds of 10 graph replays over "
                   "`copies` layers); expert_TBps = the hit experts' bf16 weight bytes / time",
           "candidates": {"moe": "ops.moe_mlp: moe_route + grouped GEMM x 2 + moe_combine",
                          "loop": "per hit expert: index_select, F.linear, swiglu, F.linear, "
                                  "index_add_ (fp32); routing on the host, not timed",
                          "route / gate_up / down / combine": "moe's launches, each alone"},
           "models": {}}
    if (a.fp8 or a.fp4) and not a.tile:
        res["unit"] = ("us per MoE layer (median of 7 interleaved rounds of 10 graph replays over "
                       "`copies` layers); expert_TBps = the hit experts' weight bytes in the "
                       "candidate's format (fp8: plus their fp32 row scales) / time; vs_bf16 = "
                       "time / the bf16 twin's time")
        res["candidates"] = {"moe / gate_up / down": "bf16 expert weights (ops.moe_mlp and its "
                                                     "two grouped GEMMs alone)",
                             "moe_fp8 / gate_up_fp8 / down_fp8": "the same on "
                             "ops.quantize_expert_weights_fp8 of the same tensors"}
    if a.fp4 and not a.tile:
        res["unit"] = ("us per MoE layer (median of 7 interleaved rounds of 10 graph replays over "
                       "`copies` layers); expert_TBps = the hit experts' weight bytes in the "
                       "candidate's format (fp8: plus their fp32 row scales; fp4: 17/32 byte per "
                       "weight, nibbles and e8m0 block scales) / time; vs_bf16 / vs_fp8 = time / "
                       "the bf16 / fp8 twin's time; bytes_vs_fp8 = the byte ratio to the fp8 twin")
        res["candidates"]["moe_fp4 / gate_up_fp4 / down_fp4"] = (
            "the same on ops.quantize_expert_weights_mxfp4 of the same tensors")
    if a.shared:
        res["unit"] = ("us per MoE block (median of 7 interleaved rounds of 10 graph replays over "
                       "`copies` blocks); weight_TBps = the hit experts' and the shared expert's "
                       "bf16 weight bytes / time; fused_vs_unfused = time ratio")
        res["candidates"] = {
            "fused": "MoEMLP.forward: shared expert, one router product with the gate row, "
                     "moe_topk with the gate column, grouped GEMM x 2, moe_combine with the "
                     "shared term",
            "unfused": "the same shared expert and routed experts with a separate H -> 1 "
                       "product, sigmoid * mul and add as torch ops",
            "shared_expert": "the shared expert's dense MLP alone (part of both)"}
    if a.tile:
        res["unit"] = ("us per MoE layer (median of 7 interleaved rounds of 10 graph replays, 3 "
                       "past T = 2048, over `copies` layers); TFLOPs = 6 T k H I (gate_up: 4, "
                       "down: 2) / time; vs_* = time ratio; separated = the min-max ranges of "
                       "the rounds of the two kernels do not overlap")
        res["candidates"] = {
            "moe": "moe_route, both grouped products on the weight-streaming kernel (32-row "
                   "tiles), moe_combine",
            "moe_tile": "the same launches with both products on the MFMA tile GEMM (128-row "
                        "tiles, moe_tile.hip)",
            "loop": "per hit expert: index_select, F.linear, swiglu, F.linear, index_add_ "
                    "(fp32); routing on the host, not timed",
            "gate_up / down, gate_up_tile / down_tile": "the two products alone, on either kernel"}
    if tile_q:
        fmt = "MXFP4" if a.fp4 else "fp8"
        res["unit"] += ("; vs_bf16_tile = time / the bf16 tile kernel's on the dequantised "
                        "weights; weight_bytes_vs_bf16 = the expert bytes behind it / the bf16 ones")
        res["weight_format"] = fmt
        res["candidates"] = {
            "moe": f"moe_route, both grouped products on the weight-streaming kernel (32-row "
                   f"tiles) on {fmt} experts, moe_combine: what runs with moe_tile_rows_q = 0",
            "moe_tile": f"the same launches with both products on the {fmt} MFMA tile GEMM "
                        "(128-row tiles, moe_tile.hip; the weights widened at fragment-read time)",
            "moe_tile_bf16": "the bf16 tile GEMM on the dequantised weights",
            "loop": "per hit expert on the dequantised bf16 weights: index_select, F.linear, "
                    "swiglu, F.linear, index_add_ (fp32); routing on the host, not timed",
            "gate_up / down, gate_up_tile / down_tile, gate_up_tile_bf16 / down_tile_bf16":
                "the two products alone, on each kernel"}
    if (a.fp8 or a.fp4 or a.shared or a.tile) and a.note:
        res["note"] = a.note
    with torch.no_grad():
        for name in a.models.split(","):
            if a.shared:
                bench_shared(torch, ops, F, name.strip(), [int(r) for r in a.rows.split(",")],
                             res, a)
                continue
            if tile_q:      # tiles=True on quantised experts needs the knob set
                with ops.kernel_policy(moe_tile_rows_q=32):
                    bench_tile_q(torch, ops, F, name.strip(),
                                 [int(r) for r in a.rows.split(",")], res, a)
                continue
            if a.tile:
                bench_tile(torch, ops, F, name.strip(), [int(r) for r in a.rows.split(",")],
                           res, a)
                continue
            bench_model(torch, ops, F, name.strip(), [int(r) for r in a.rows.split(",")], res, a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
