#!/usr/bin/env python3
"""The fp8 weight-streaming MFMA kernel for 3-32 rows (``KernelPolicy.fp8_small_m``,
gemm_fp8_small.hip) measured against the fp8 route it replaces (docs/kernels.md, "fp8 weights,
3-32 rows", quotes the results).  scripts/bench_mxfp4.py's protocol and helpers.

    python3 scripts/bench_fp8_small.py [all|small|decode_small] [--num-layers N] [--out DIR]

``small``         the four Llama-3-70B projections (gate|up with its SwiGLU) at M = 3, 4, 8, 15, 16,
                  17 and 32, each candidate's launches captured in one hipGraph over enough weight
                  copies that they stream from HBM, replays interleaved, median of 7 rounds:
                  the new kernel; the fp8 route with the flag off, activation preparation
                  included (row quantiser + torch._scaled_mm below 16 rows, the block-scaled tile
                  GEMM from 16); bf16; and the fp8 GEMV at M = 2 as the floor.  Also derives
                  ``recommended_fp8_small_m``: the largest measured M up to which the kernel beats
                  the flag-off route on all four shapes.
``decode_small``  a decode step of 4, 8, 16 and 32 sequences (one engine per mode, one graph bucket
                  per batch): fp8 with the flag off, fp8 with ``fp8_small_m=32``, fp8 with the flag
                  off again, and bf16, in one process.
``all``           (default) both, each as a child process under its own time limit.
Results: ``<out>/small.json`` and ``<out>/decode_small.json`` (default ``profiles/fp8_small``).
"""
import argparse
import gc
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_mxfp4 as bm  # noqa: E402  (its path set-up makes the package importable too)

STEP_LIMIT_S = {"small": 600, "decode_small": 900}
SMALL_M = (3, 4, 8, 15, 16, 17, 32)
BYTES_PER_WEIGHT = {"fp8": 1.0, "bf16": 2.0}


def step_small(a):
    """us per product at 3-32 rows, as a decode step pays it (activation preparation and, for
    gate|up, the SwiGLU included -- each format on the route LlamaMLP gives it)."""
    torch = bm._torch()
    from distributed_llm_inference import ops
    dev = torch.device("cuda", 0)
    cands = ("fp8_small", "fp8_off", "bf16", "fp8_gemv_m2")
    wfmt = {"fp8_small": "fp8", "fp8_off": "fp8", "bf16": "bf16", "fp8_gemv_m2": "fp8"}
    res = {"unit": "us per product (median of 7 interleaved rounds), effective weight TB/s",
           "bytes_per_weight": BYTES_PER_WEIGHT,
           "candidates": {"fp8_small": "ops.small_gemm_fp8 (fp8_small_m): the weight-streaming MFMA kernel",
                          "fp8_off": "fp8, default policy: row quantiser + torch._scaled_mm / fp8 tile GEMM",
                          "bf16": "bf16",
                          "fp8_gemv_m2": "the fp8 GEMV on 2 bf16 rows (the floor), whatever M the row says"},
           "gate_up": "with SwiGLU (fused where the route fuses it, else swiglu_interleaved after)",
           "shapes": {}}

    def dense_gate_up(lin, x):          # LlamaMLP's last fused branch
        if lin.tile_splits(x):
            return ops.gemm_tile(x, lin.weight, swiglu=True)
        return ops.swiglu_interleaved(lin(x))

    def fp8_gate_up(lin, x):            # LlamaMLP's fp8 branch with the flag off, bf16 h
        xq, xs = ops.quant_rowwise(x)
        if ops.tile_gemm_splits_fp8(x.shape[0], lin.out_features, lin.in_features):
            return ops.gemm_tile_fp8(xq, xs, lin.weight_fp8, lin.weight_scale, swiglu=True,
                                     gemm4=ops.policy().fp8_on_gemm4("gate_up"))
        return ops.swiglu_interleaved(lin(None, (xq, xs)))

    assert ops.policy().fp8_small_m == 0, "the yardstick is the flag-off route"
    for name, (N, K) in bm.SHAPES.items():
        glu = name == "gate_up"
        lins = {}
        for fmt in ("fp8", "bf16"):
            n = int(min(8, max(3, -(-(1 << 29) // int(N * K * BYTES_PER_WEIGHT[fmt])))))
            lins[fmt] = bm._linears(dev, fmt, N, K, n)
            for lin in lins[fmt]:
                lin.role = name
        x2 = torch.randn(2, K, device=dev, dtype=torch.bfloat16)
        for M in SMALL_M:
            x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)

            def call(c, lin):
                if c == "fp8_small":
                    return ops.small_gemm_fp8(x, lin.weight_fp8, lin.weight_scale, swiglu=glu)
                if c == "fp8_gemv_m2":
                    return ops.skinny_gemm_fp8(x2, lin.weight_fp8, lin.weight_scale, swiglu=glu)
                if glu:
                    return fp8_gate_up(lin, x) if c == "fp8_off" else dense_gate_up(lin, x)
                return lin(x)

            graphs = {c: bm._graph(torch, [(lambda lin=lin, c=c: call(c, lin))
                                           for lin in lins[wfmt[c]]]) for c in cands}
            samples = {c: [] for c in cands}
            for _ in range(7):                       # interleaved: same box, same minute
                for c in cands:
                    samples[c].append(bm._timed(torch, graphs[c], 10) / len(lins[wfmt[c]]))
            row = {}
            for c in cands:
                us = statistics.median(samples[c])
                row[c] = {"us": round(us, 2),
                          "TBps": round(N * K * BYTES_PER_WEIGHT[wfmt[c]] / us / 1e6, 2),
                          "min_us": round(min(samples[c]), 2), "max_us": round(max(samples[c]), 2),
                          "copies": len(lins[wfmt[c]])}
            row["small_vs_off"] = round(row["fp8_small"]["us"] / row["fp8_off"]["us"], 3)
            row["small_vs_bf16"] = round(row["fp8_small"]["us"] / row["bf16"]["us"], 3)
            row["small_vs_gemv_m2"] = round(row["fp8_small"]["us"] / row["fp8_gemv_m2"]["us"], 3)
            res["shapes"][f"{name}_M{M}"] = dict(N=N, K=K, M=M, **row)
            print(f"{name:8s} M={M:2d} " + "  ".join(f"{c} {row[c]['us']:8.2f}" for c in cands)
                  + f"  us; small {row['fp8_small']['TBps']:.2f} TB/s, /off "
                  f"{row['small_vs_off']:.3f} /gemv2 {row['small_vs_gemv_m2']:.3f}", flush=True)
            bm._save(a, "small.json", res)
            del graphs
            torch.cuda.empty_cache()
        del lins
        gc.collect()
        torch.cuda.empty_cache()
    # the largest measured M up to which the kernel beats the flag-off route on every shape
    rec = 0
    for M in SMALL_M:
        if all(res["shapes"][f"{n}_M{M}"]["small_vs_off"] < 1 for n in bm.SHAPES):
            rec = M
        else:
            break
    res["recommended_fp8_small_m"] = rec
    print("recommended fp8_small_m:", rec, flush=True)
    return res


def step_decode_small(a):
    batches = [4, 8, 16, 32]
    res = {"model": "llama-3-70b (random init)", "num_layers": a.num_layers or 80,
           "batches": batches,
           "unit": "ms per decode step of `batch` sequences (difference of two generate() calls; "
                   "median and the 3 samples)",
           "modes": {}}
    for key, mode, kernels in (("fp8_off", "fp8", "fp8_small_m=0"),
                               ("fp8_small32", "fp8", "fp8_small_m=32"),
                               ("fp8_off_again", "fp8", "fp8_small_m=0"),
                               ("bf16", False, "")):
        print(f"{key}: building the engine", flush=True)
        r = bm._decode_ms_batches(a, mode, batches, 8, 72, kernels)
        res["modes"][key] = {str(b): r[b] for b in batches}
        print(key, {b: (r[b]["ms_per_step"], r[b]["samples_ms"]) for b in batches}, flush=True)
        bm._save(a, "decode_small.json", res)
    m = res["modes"]
    cmp_ = {}
    for b in map(str, batches):
        on = m["fp8_small32"][b]
        offs = m["fp8_off"][b]["samples_ms"] + m["fp8_off_again"][b]["samples_ms"]
        cmp_[b] = {"small_ms": on["ms_per_step"], "small_samples_ms": on["samples_ms"],
                   "off_ms": round(statistics.median(offs), 3), "off_samples_ms": offs,
                   "small_vs_off": round(on["ms_per_step"] / statistics.median(offs), 3),
                   "small_vs_bf16": round(on["ms_per_step"] / m["bf16"][b]["ms_per_step"], 3),
                   # clear of the spread: the slowest flag-on sample under the fastest flag-off one
                   "clear_of_spread": bool(max(on["samples_ms"]) < min(offs))}
    res["small_vs_off"] = cmp_
    return res


STEPS = {"small": (step_small, "small.json"), "decode_small": (step_decode_small, "decode_small.json")}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("step", nargs="?", default="all", choices=["all"] + list(STEPS))
    ap.add_argument("--num-layers", type=int, default=8,
                    help="decode_small: this many of the model's 80 layers (0 = all)")
    ap.add_argument("--out", default=os.path.join(bm.REPO, "profiles", "fp8_small"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.step == "all":
        for step in STEPS:
            cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S[step]), sys.executable,
                   os.path.abspath(__file__), step, "--num-layers", str(a.num_layers),
                   "--out", a.out]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                print(f"bench_fp8_small: step {step} ended with status {rc}; stopping", flush=True)
                return rc
        return 0
    fn, name = STEPS[a.step]
    bm._save(a, name, fn(a))
    return 0


if __name__ == "__main__":
    sys.exit(main())
