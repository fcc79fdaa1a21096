#!/usr/bin/env python
"""Int4 group-quantised weights: engine decode steps of 1-32 sequences against the other modes.

One process, one GPU: a Llama-3-70B-shaped stage (random init, ``--num-layers`` of its layers)
decodes batches of 1, 4, 8, 16 and 32 sequences under hipGraphs with int4 weights
(``quantize="int4"``: gemm_int4.hip's weight-streaming kernel on every projection), bf16, MXFP4 on
its weight-streaming kernel (``fp4_small_m=32``) and block-scaled fp8 -- bench_mxfp4.py's
measurement (the difference of two generate() calls), one engine per mode, one after the other.
Writes ``decode_small.json`` under ``--out`` (default profiles/int4) after every mode, with the
ratio of int4's step time to each other mode's per batch size.

    python scripts/bench_int4.py --num-layers 8
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_mxfp4 import REPO, _decode_ms_batches, _save   # noqa: E402

BATCHES = [1, 4, 8, 16, 32]
MODES = (("int4", "int4", ""), ("bf16", False, ""), ("mxfp4_small32", "mxfp4", "fp4_small_m=32"),
         ("fp8_block", "fp8_block", ""))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--num-layers", type=int, default=8,
                    help="this many of the model's 80 layers (0 = all)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "int4"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    res = {"model": "llama-3-70b (random init)", "num_layers": a.num_layers or 80,
           "batches": BATCHES,
           "unit": "ms per decode step of `batch` sequences (difference of two generate() calls)",
           "modes": {}}
    for key, mode, kernels in MODES:
        print(f"{key}: building the engine", flush=True)
        r = _decode_ms_batches(a, mode, BATCHES, 8, 72, kernels)
        res["modes"][key] = {str(b): r[b] for b in BATCHES}
        print(key, {b: r[b]["ms_per_step"] for b in BATCHES}, flush=True)
        _save(a, "decode_small.json", res)           # what is measured so far survives a time limit
    m = res["modes"]
    res["int4_vs"] = {
        str(b): {o: round(m["int4"][str(b)]["ms_per_step"] / m[o][str(b)]["ms_per_step"], 3)
                 for o in m if o != "int4"} for b in BATCHES}
    _save(a, "decode_small.json", res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
