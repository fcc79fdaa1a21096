#!/usr/bin/env python3
"""MXFP4 weights measured against fp8 and bf16 on one GPU (docs/kernels.md quotes the results).

    python3 scripts/bench_mxfp4.py [all|gemv|gemm|small|decode|batch512|decode_small]
                                   [--num-layers N] [--out DIR]

``gemv``      per-shape weight-streaming GEMV time for the four Llama-3-70B projections at
              M = 1 and 2, fp4 / fp8 / bf16: every format's launches captured in one hipGraph
              over enough weight copies (> 1 GiB) that they stream from HBM, replays of the three
              formats interleaved on the same box; us per launch and effective weight TB/s.
``decode``    batch-1 decode through LLMEngine (random-init llama-3-70b, ``--num-layers`` of its
              80 layers): ms per token and KV blocks for bf16, fp8 and mxfp4.
``gemm``      the four projections at M = 64 and 512 through ``Linear``: MXFP4 on the fp4 x fp8
              MFMA tile GEMM (``KernelPolicy.fp4_mfma``; with and without its activation
              quantiser) against the dequantise path, fp8 and bf16; graph-timed over weight
              copies, candidates interleaved, median of 7 rounds.
``small``     the four projections (gate|up with its SwiGLU) at M = 3, 4, 8, 16, 17 and 32: the
              weight-streaming MFMA kernel for MXFP4 (``KernelPolicy.fp4_small_m``) against the
              dequantise path, the ``fp4_mfma`` tile GEMM, fp8 and bf16, with the fp4 GEMV at
              M = 2 as the floor; same protocol as ``gemm``.  Also derives the recommended
              ``fp4_small_m``: the largest M up to which the kernel beats both existing MXFP4
              routes on all four shapes.
``batch512``  one 512-sequence decode step, mxfp4 against bf16: the price of the dequantise pass;
              then mxfp4 with ``fp4_mfma`` on and off (and fp8) in the same process.
``decode_small``  a decode step of 4, 8, 16 and 32 sequences (one engine per mode, one graph
              bucket per batch): mxfp4 with ``fp4_small_m`` off, ``fp4_small_m=32`` and
              ``fp4_mfma=1``, fp8 and bf16 in the same process.
``all``       (default) runs the steps one after the other, each as a child process under
              its own time limit; it stops at the first step that fails and never opens the GPU
              itself.  Results: ``<out>/gemv.json``, ``gemm.json``, ``decode_b1.json``,
              ``decode_b512.json``, ``decode_b512_mfma.json``, ``small.json``, ``decode_small.json``.
"""
import argparse
import gc
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

STEP_LIMIT_S = {"gemv": 300, "gemm": 420, "small": 600, "decode": 900, "batch512": 900,
                "decode_small": 900}
H, I = 8192, 28672
SHAPES = {"qkv": (10240, H), "o": (H, H), "gate_up": (2 * I, H), "down": (H, I)}
BYTES_PER_WEIGHT = {"fp4": 17 / 32, "fp8": 1.0, "bf16": 2.0}


def _torch():
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    if not torch.cuda.is_available():
        raise SystemExit("bench_mxfp4: needs a GPU (nothing is measured without one)")
    return torch


def _graph(torch, fns):
    """The calls ``fns`` captured in one hipGraph (after an eager warm-up run of them)."""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for f in fns:
            f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for f in fns:
            f()
    g.replay()
    torch.cuda.synchronize()
    return g


def _timed(torch, g, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps     # us per replay


# ----------------------------------------------------------------------------- GEMV rates
def step_gemv(a):
    torch = _torch()
    from distributed_llm_inference import ops
    dev = torch.device("cuda", 0)

    def weights(fmt, N, K, n):
        if fmt == "bf16":
            return [(torch.empty(N, K, device=dev, dtype=torch.bfloat16).normal_(0, 0.02),)
                    for _ in range(n)]
        if fmt == "fp8":
            sc = torch.rand(N, device=dev) * 1e-2 + 1e-3
            return [(torch.randint(-100, 100, (N, K), device=dev, dtype=torch.int8)
                     .view(torch.uint8).bitwise_and_(0x77).view(torch.float8_e4m3fn), sc)
                    for _ in range(n)]
        return [(torch.randint(0, 256, (N, K // 2), device=dev, dtype=torch.uint8),
                 torch.randint(117, 128, (N, K // 32), device=dev, dtype=torch.uint8))
                for _ in range(n)]

    def call(fmt, x, w):
        if fmt == "bf16":
            return ops.skinny_gemm(x, w[0])
        if fmt == "fp8":
            return ops.skinny_gemm_fp8(x, w[0], w[1])
        return ops.skinny_gemm_fp4(x, w[0], w[1])

    res = {"unit": "us per launch (median of interleaved rounds), effective weight TB/s",
           "bytes_per_weight": BYTES_PER_WEIGHT, "shapes": {}}
    for name, (N, K) in SHAPES.items():
        for M in (1, 2):
            x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
            graphs, copies = {}, {}
            for fmt in ("fp4", "fp8", "bf16"):
                wbytes = N * K * BYTES_PER_WEIGHT[fmt]
                n = int(min(48, max(3, -(-(1 << 30) // int(wbytes)))))
                ws = weights(fmt, N, K, n)
                graphs[fmt] = (_graph(torch, [(lambda w=w: call(fmt, x, w)) for w in ws]), ws)
                copies[fmt] = n
            samples = {fmt: [] for fmt in graphs}
            for _ in range(7):                       # interleaved: same box, same minute
                for fmt, (g, _) in graphs.items():
                    samples[fmt].append(_timed(torch, g, 10) / copies[fmt])
            row = {}
            for fmt in graphs:
                us = statistics.median(samples[fmt])
                row[fmt] = {"us": round(us, 2),
                            "TBps": round(N * K * BYTES_PER_WEIGHT[fmt] / us / 1e6, 2),
                            "min_us": round(min(samples[fmt]), 2),
                            "max_us": round(max(samples[fmt]), 2), "copies": copies[fmt]}
            row["fp4_vs_fp8"] = round(row["fp4"]["us"] / row["fp8"]["us"], 3)
            res["shapes"][f"{name}_M{M}"] = dict(N=N, K=K, M=M, **row)
            print(f"{name:8s} M={M} " + "  ".join(
                f"{f} {row[f]['us']:8.2f} us {row[f]['TBps']:5.2f} TB/s" for f in graphs)
                + f"  fp4/fp8 {row['fp4_vs_fp8']:.3f}", flush=True)
            del graphs
            torch.cuda.empty_cache()
    return res


# ----------------------------------------------------------------------------- tile GEMM
def _linears(dev, fmt, N, K, n):
    """``n`` copies of one [N, K] Linear in weight format ``fmt`` (fp4 / fp8 / bf16)."""
    import copy
    from distributed_llm_inference.models.common import Linear
    base = Linear(K, N, device=dev)
    base.weight.data.normal_(0, 0.02)
    if fmt == "fp4":
        base.quantize_mxfp4()
    elif fmt == "fp8":
        base.quantize_fp8()
    return [base] + [copy.deepcopy(base) for _ in range(n - 1)]


def step_gemm(a):
    """us per product of ``Linear.forward`` (what a decode step pays, activation preparation
    included) per weight format; ``fp4_mfma_gemm`` is the fp4 kernel alone on rows quantised
    outside the timed graph."""
    torch = _torch()
    from distributed_llm_inference import ops
    dev = torch.device("cuda", 0)
    cands = ("fp4_mfma", "fp4_mfma_gemm", "fp4_dequant", "fp8", "bf16")
    wfmt = {"fp4_mfma": "fp4", "fp4_mfma_gemm": "fp4", "fp4_dequant": "fp4", "fp8": "fp8",
            "bf16": "bf16"}

    res = {"unit": "us per product (median of 7 interleaved rounds), dense TFLOP/s",
           "candidates": {"fp4_mfma": "MXFP4 Linear, fp4_mfma=1: MX quantiser + gemm_fp4 (+ reduce)",
                          "fp4_mfma_gemm": "gemm_fp4 (+ reduce) alone, rows quantised beforehand",
                          "fp4_dequant": "MXFP4 Linear, fp4_mfma=0: dequantise + the bf16 path",
                          "fp8": "fp8 Linear: row quantiser + fp8 GEMM", "bf16": "bf16 Linear"},
           "shapes": {}}
    for name, (N, K) in SHAPES.items():
        lins = {}
        for fmt in ("fp4", "fp8", "bf16"):
            # enough copies that the weights stream from HBM (> 512 MiB per replay)
            n = int(min(8, max(3, -(-(1 << 29) // int(N * K * BYTES_PER_WEIGHT[fmt])))))
            lins[fmt] = _linears(dev, fmt, N, K, n)
        for M in (64, 512):
            x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
            xq = ops.quant_mx(x)
            sp = ops.tile_gemm_splits_fp4(M, N, K)

            def call(c, lin):
                if c == "fp4_mfma":
                    with ops.kernel_policy(fp4_mfma=True):
                        return lin(x)
                if c == "fp4_mfma_gemm":
                    return ops.gemm_fp4_mx(xq, lin.weight_fp4, lin.weight_block_scale, sp)
                return lin(x)

            graphs = {c: _graph(torch, [(lambda lin=lin, c=c: call(c, lin)) for lin in lins[wfmt[c]]])
                      for c in cands}
            samples = {c: [] for c in cands}
            for _ in range(7):                       # interleaved: same box, same minute
                for c in cands:
                    samples[c].append(_timed(torch, graphs[c], 10) / len(lins[wfmt[c]]))
            row = {}
            for c in cands:
                us = statistics.median(samples[c])
                row[c] = {"us": round(us, 2), "TFLOPs": round(2.0 * M * N * K / us / 1e6, 1),
                          "min_us": round(min(samples[c]), 2), "max_us": round(max(samples[c]), 2),
                          "copies": len(lins[wfmt[c]])}
            row["fp4_splits"] = sp
            row["mfma_vs_dequant"] = round(row["fp4_mfma"]["us"] / row["fp4_dequant"]["us"], 3)
            row["mfma_vs_fp8"] = round(row["fp4_mfma"]["us"] / row["fp8"]["us"], 3)
            row["mfma_vs_bf16"] = round(row["fp4_mfma"]["us"] / row["bf16"]["us"], 3)
            res["shapes"][f"{name}_M{M}"] = dict(N=N, K=K, M=M, **row)
            print(f"{name:8s} M={M:3d} " + "  ".join(f"{c} {row[c]['us']:8.2f}" for c in cands)
                  + f"  us; mfma/dequant {row['mfma_vs_dequant']:.3f} mfma/fp8 "
                  f"{row['mfma_vs_fp8']:.3f} mfma/bf16 {row['mfma_vs_bf16']:.3f}", flush=True)
            _save(a, "gemm.json", res)
            del graphs
            torch.cuda.empty_cache()
        del lins
        gc.collect()
        torch.cuda.empty_cache()
    return res


# ----------------------------------------------------------------------------- 3-32 rows
SMALL_M = (3, 4, 8, 16, 17, 32)


def step_small(a):
    """us per product at 3-32 rows, as a decode step pays it (activation preparation and, for
    gate|up, the SwiGLU included -- each format on the route LlamaMLP gives it)."""
    torch = _torch()
    from distributed_llm_inference import ops
    dev = torch.device("cuda", 0)
    cands = ("fp4_small", "fp4_dequant", "fp4_mfma", "fp8", "bf16", "fp4_gemv_m2")
    wfmt = {"fp4_small": "fp4", "fp4_dequant": "fp4", "fp4_mfma": "fp4", "fp8": "fp8",
            "bf16": "bf16", "fp4_gemv_m2": "fp4"}
    res = {"unit": "us per product (median of 7 interleaved rounds), effective weight TB/s",
           "bytes_per_weight": BYTES_PER_WEIGHT,
           "candidates": {"fp4_small": "ops.small_gemm_fp4 (fp4_small_m): the weight-streaming MFMA kernel",
                          "fp4_dequant": "MXFP4, default policy: dequantise + the bf16 path",
                          "fp4_mfma": "MXFP4, fp4_mfma=1: MX quantiser + gemm_fp4 (+ reduce)",
                          "fp8": "fp8: row quantiser + fp8 GEMM", "bf16": "bf16",
                          "fp4_gemv_m2": "the fp4 GEMV at M = 2 (the floor), whatever M the row says"},
           "gate_up": "with SwiGLU (fused where the route fuses it, else swiglu_interleaved after)",
           "shapes": {}}

    def dense_gate_up(lin, x):          # LlamaMLP's last fused branch (bf16 / dequantised MXFP4)
        if lin.tile_splits(x):
            return ops.gemm_tile(x, lin.dense_weight(), swiglu=True)
        return ops.swiglu_interleaved(lin(x))

    def fp8_gate_up(lin, x):            # LlamaMLP's fp8 branch, bf16 h
        xq, xs = ops.quant_rowwise(x)
        if ops.tile_gemm_splits_fp8(x.shape[0], lin.out_features, lin.in_features):
            return ops.gemm_tile_fp8(xq, xs, lin.weight_fp8, lin.weight_scale, swiglu=True,
                                     gemm4=ops.policy().fp8_on_gemm4("gate_up"))
        return ops.swiglu_interleaved(lin(None, (xq, xs)))

    for name, (N, K) in SHAPES.items():
        glu = name == "gate_up"
        lins = {}
        for fmt in ("fp4", "fp8", "bf16"):
            n = int(min(8, max(3, -(-(1 << 29) // int(N * K * BYTES_PER_WEIGHT[fmt])))))
            lins[fmt] = _linears(dev, fmt, N, K, n)
        x2 = torch.randn(2, K, device=dev, dtype=torch.bfloat16)
        for M in SMALL_M:
            x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)

            def call(c, lin):
                if c == "fp4_small":
                    return ops.small_gemm_fp4(x, lin.weight_fp4, lin.weight_block_scale, swiglu=glu)
                if c == "fp4_gemv_m2":
                    return ops.skinny_gemm_fp4(x2, lin.weight_fp4, lin.weight_block_scale, swiglu=glu)
                if c == "fp4_mfma":
                    with ops.kernel_policy(fp4_mfma=True):
                        if glu:
                            return ops.gemm_fp4_mx(ops.quant_mx(x), lin.weight_fp4,
                                                   lin.weight_block_scale, swiglu=True)
                        return lin(x)
                if glu:
                    return fp8_gate_up(lin, x) if c == "fp8" else dense_gate_up(lin, x)
                return lin(x)

            graphs = {c: _graph(torch, [(lambda lin=lin, c=c: call(c, lin)) for lin in lins[wfmt[c]]])
                      for c in cands}
            samples = {c: [] for c in cands}
            for _ in range(7):                       # interleaved: same box, same minute
                for c in cands:
                    samples[c].append(_timed(torch, graphs[c], 10) / len(lins[wfmt[c]]))
            row = {}
            for c in cands:
                us = statistics.median(samples[c])
                row[c] = {"us": round(us, 2),
                          "TBps": round(N * K * BYTES_PER_WEIGHT[wfmt[c]] / us / 1e6, 2),
                          "min_us": round(min(samples[c]), 2), "max_us": round(max(samples[c]), 2),
                          "copies": len(lins[wfmt[c]])}
            row["small_vs_dequant"] = round(row["fp4_small"]["us"] / row["fp4_dequant"]["us"], 3)
            row["small_vs_mfma"] = round(row["fp4_small"]["us"] / row["fp4_mfma"]["us"], 3)
            row["small_vs_gemv_m2"] = round(row["fp4_small"]["us"] / row["fp4_gemv_m2"]["us"], 3)
            res["shapes"][f"{name}_M{M}"] = dict(N=N, K=K, M=M, **row)
            print(f"{name:8s} M={M:2d} " + "  ".join(f"{c} {row[c]['us']:8.2f}" for c in cands)
                  + f"  us; small {row['fp4_small']['TBps']:.2f} TB/s, /dequant "
                  f"{row['small_vs_dequant']:.3f} /mfma {row['small_vs_mfma']:.3f}", flush=True)
            _save(a, "small.json", res)
            del graphs
            torch.cuda.empty_cache()
        del lins
        gc.collect()
        torch.cuda.empty_cache()
    # the largest M up to which the kernel beats both existing MXFP4 routes on every shape
    rec = 0
    for M in SMALL_M:
        rows = [res["shapes"][f"{n}_M{M}"] for n in SHAPES]
        if all(r["small_vs_dequant"] < 1 and r["small_vs_mfma"] < 1 for r in rows):
            rec = M
        else:
            break
    res["recommended_fp4_small_m"] = rec
    print("recommended fp4_small_m:", rec, flush=True)
    return res


# ----------------------------------------------------------------------------- engine decode
def _decode_ms_batches(a, quantize, batches, short, long_, kernels=""):
    """ms per decode step for each batch size of ``batches`` on one engine (one graph bucket per
    batch size): two generate() calls that differ only in the number of decode steps (the
    prefill and the start-up cancel in the difference)."""
    torch = _torch()
    from distributed_llm_inference.config import CacheConfig, KernelPolicy, ServeConfig, resolve_model
    from distributed_llm_inference.runtime.engine import EngineConfig, LLMEngine
    from distributed_llm_inference.runtime.sequence import SamplingParams
    spec = resolve_model("llama-3-70b")
    if a.num_layers:
        spec = spec.replace(num_layers=a.num_layers, name=f"{spec.name}-{a.num_layers}L")
    # always an explicit policy: the engine installs it process-wide, and the engines of one
    # step run one after the other in this process
    cfg = EngineConfig(model=spec, random_init=True, seed=0, quantize=quantize,
                       kernels=KernelPolicy().with_overrides(kernels),
                       cache=CacheConfig(block_size=64, gpu_memory_utilization=0.90),
                       serve=ServeConfig(max_batch_size=max(batches), max_num_batched_tokens=2048,
                                         max_seq_len=512, use_graphs=True,
                                         graph_batch_sizes=sorted(batches)))
    eng = LLMEngine(spec, device="cuda:0", cfg=cfg)
    blocks = min(ex.pool.num_blocks for ex in eng.executors)
    out = {}
    for batch in batches:
        prompts = [[(7 * i + j) % 1000 + 1 for j in range(4)] for i in range(batch)]

        def run(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            seqs = eng.generate(prompts, SamplingParams(max_tokens=n, ignore_eos=True))
            torch.cuda.synchronize()
            assert all(len(s.output) == n for s in seqs)
            return time.perf_counter() - t0

        run(short)                                        # warm-up: code objects, graphs
        ms = [(run(long_) - run(short)) / (long_ - short) * 1e3 for _ in range(3)]
        out[batch] = {"ms_per_step": round(statistics.median(ms), 3),
                      "samples_ms": [round(m, 3) for m in ms], "kv_blocks": int(blocks),
                      "layers": spec.num_layers}
    del eng
    gc.collect()
    torch.cuda.empty_cache()
    return out


def _decode_ms(a, quantize, batch, short, long_, kernels=""):
    return _decode_ms_batches(a, quantize, [batch], short, long_, kernels)[batch]


def step_decode(a):
    res = {"model": "llama-3-70b (random init)", "batch": 1, "num_layers": a.num_layers or 80,
           "unit": "ms per token (difference of two generate() calls), KV blocks of 64 tokens"}
    for mode in ("mxfp4", "fp8", "bf16"):
        print(f"batch 1, {mode}: building the engine", flush=True)
        res[mode] = _decode_ms(a, False if mode == "bf16" else mode, 1, 16, 144)
        print(mode, res[mode], flush=True)
        _save(a, "decode_b1.json", res)           # what is measured so far survives a time limit
    return res


def step_batch512(a):
    res = {"model": "llama-3-70b (random init)", "batch": 512, "num_layers": a.num_layers or 80,
           "unit": "ms per 512-sequence decode step (difference of two generate() calls)"}
    for mode in ("mxfp4", "bf16"):
        print(f"batch 512, {mode}: building the engine", flush=True)
        res[mode] = _decode_ms(a, False if mode == "bf16" else mode, 512, 4, 28)
        print(mode, res[mode], flush=True)
        _save(a, "decode_b512.json", res)
    res["mxfp4_vs_bf16"] = round(res["mxfp4"]["ms_per_step"] / res["bf16"]["ms_per_step"], 3)
    # the MFMA-native fp4 tile GEMM (KernelPolicy.fp4_mfma) on and off in this same process,
    # with fp8 and the bf16 run above for scale
    mf = {"model": res["model"], "batch": 512, "num_layers": res["num_layers"], "unit": res["unit"],
          "mxfp4_dequant": res["mxfp4"], "bf16": res["bf16"]}
    for key, mode, kernels in (("mxfp4_mfma", "mxfp4", "fp4_mfma=1"),
                               ("mxfp4_dequant_again", "mxfp4", "fp4_mfma=0"), ("fp8", "fp8", "")):
        print(f"batch 512, {key}: building the engine", flush=True)
        mf[key] = _decode_ms(a, mode, 512, 4, 28, kernels)
        print(key, mf[key], flush=True)
        _save(a, "decode_b512_mfma.json", mf)
    on = mf["mxfp4_mfma"]["ms_per_step"]
    # against the faster of the two flag-off runs (before and after the flag-on engine)
    off = min(mf["mxfp4_dequant"]["ms_per_step"], mf["mxfp4_dequant_again"]["ms_per_step"])
    mf["mfma_vs_dequant"] = round(on / off, 3)
    mf["mfma_vs_fp8"] = round(on / mf["fp8"]["ms_per_step"], 3)
    mf["mfma_vs_bf16"] = round(on / mf["bf16"]["ms_per_step"], 3)
    mf["mfma_faster_than_dequant"] = bool(on < off)
    _save(a, "decode_b512_mfma.json", mf)
    return res


def step_decode_small(a):
    batches = [4, 8, 16, 32]
    res = {"model": "llama-3-70b (random init)", "num_layers": a.num_layers or 80,
           "batches": batches,
           "unit": "ms per decode step of `batch` sequences (difference of two generate() calls)",
           "modes": {}}
    for key, mode, kernels in (("mxfp4_dequant", "mxfp4", "fp4_small_m=0"),
                               ("mxfp4_small32", "mxfp4", "fp4_small_m=32"),
                               ("mxfp4_mfma", "mxfp4", "fp4_mfma=1"),
                               ("fp8", "fp8", ""), ("bf16", False, "")):
        print(f"{key}: building the engine", flush=True)
        r = _decode_ms_batches(a, mode, batches, 8, 72, kernels)
        res["modes"][key] = {str(b): r[b] for b in batches}
        print(key, {b: r[b]["ms_per_step"] for b in batches}, flush=True)
        _save(a, "decode_small.json", res)
    m = res["modes"]
    res["small_vs"] = {
        str(b): {o: round(m["mxfp4_small32"][str(b)]["ms_per_step"] / m[o][str(b)]["ms_per_step"], 3)
                 for o in ("mxfp4_dequant", "mxfp4_mfma", "fp8", "bf16")} for b in batches}
    return res


def _save(a, name, res):
    with open(os.path.join(a.out, name), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


STEPS = {"gemv": (step_gemv, "gemv.json"), "gemm": (step_gemm, "gemm.json"),
         "small": (step_small, "small.json"),
         "decode": (step_decode, "decode_b1.json"),
         "batch512": (step_batch512, "decode_b512.json"),
         "decode_small": (step_decode_small, "decode_small.json")}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("step", nargs="?", default="all", choices=["all"] + list(STEPS))
    ap.add_argument("--num-layers", type=int, default=0,
                    help="decode / batch512 / decode_small: this many of the model's 80 layers (0 = all)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mxfp4"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.step == "all":
        for step in STEPS:
            cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S[step]), sys.executable,
                   os.path.abspath(__file__), step, "--num-layers", str(a.num_layers),
                   "--out", a.out]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                print(f"bench_mxfp4: step {step} ended with status {rc}; stopping", flush=True)
                return rc
        return 0
    fn, name = STEPS[a.step]
    _save(a, name, fn(a))
    return 0


if __name__ == "__main__":
    sys.exit(main())
