"""Microbenchmark of the decode step's RoPE + paged-KV write (rope_cache.hip) at the 70B / 512-row
shape: 3 bf16 split-K partials of the QKV GEMM [3, 512, 10240] summed on load, q rotated and
stored [512, 64, 128], k rotated and v written into the paged caches (one slot per sequence, a
distinct block each).  Partials rotate over 8 sets (past the MALL); calls are replayed from a
hipGraph.

    python scripts/rope_bench.py [--rows 512] [--kv-fp8] [--iters 20]
Prints one JSON line (us per call, TB/s of its HBM bytes).

    python scripts/rope_bench.py --qk-norm [--kv-fp8] [--rounds 15]
times the kernel with and without the per-head q/k RMSNorm (Qwen3) on the same inputs, the two
graphs replayed alternately in one process; prints the median us of each and their ratio."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_llm_inference import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--splits", type=int, default=3)
    ap.add_argument("--kv-fp8", action="store_true")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--no-kv", action="store_true", help="slot -1: no cache writes (diagnostic)")
    ap.add_argument("--qk-norm", action="store_true",
                    help="A/B: with vs without the per-head q/k RMSNorm, interleaved")
    ap.add_argument("--rounds", type=int, default=15, help="--qk-norm: alternating rounds")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    T, S, NSET = a.rows, a.splits, a.sets
    nh, nkv, D, bs = 64, 8, 128, 64
    N = (nh + 2 * nkv) * D
    g = torch.Generator(device=dev).manual_seed(0)
    parts = [torch.randn(S, T, N, device=dev, generator=g).to(torch.bfloat16) for _ in range(NSET)]
    kdt = torch.float8_e4m3fn if a.kv_fp8 else torch.bfloat16
    nblk = 2 * T + 8
    kc = torch.zeros(nblk, nkv, bs, D, device=dev).to(kdt)
    vc = torch.zeros(nblk, nkv, bs // 8, D, 8, device=dev).to(kdt)
    pos = torch.full((T,), 600, device=dev, dtype=torch.int32)
    slots = torch.arange(T, device=dev, dtype=torch.int64) * (2 * bs) + 37
    if a.no_kv:
        slots.fill_(-1)
    cs = ops.reference.build_cos_sin(D, 4096, 500000.0, None, device=dev)
    qo = [torch.empty(T, nh, D, dtype=torch.bfloat16, device=dev) for _ in range(NSET)]

    qw = (1 + 0.3 * torch.randn(D, device=dev, generator=g)).to(torch.bfloat16)
    kw = (1 + 0.3 * torch.randn(D, device=dev, generator=g)).to(torch.bfloat16)

    def capture(norm):
        kwargs = dict(q_norm=qw, k_norm=kw, norm_eps=1e-6) if norm else {}

        def run():
            for i in range(NSET):
                ops.rope_cache(ops.SplitKPartials(parts[i]), pos, slots, cs, nh, nkv, D, kc, vc,
                               q_out=qo[i], k_scale=0.5, v_scale=0.5, **kwargs)

        gr = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            run()
        torch.cuda.current_stream().wait_stream(s)
        with torch.cuda.graph(gr):
            run()
        gr.replay()
        torch.cuda.synchronize()
        return gr

    def time_us(gr):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            gr.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters / NSET

    kvb = 1 if a.kv_fp8 else 2
    nbytes = S * T * N * 2 + T * nh * D * 2 + 2 * T * nkv * D * kvb
    if a.qk_norm:
        graphs = {"base": capture(False), "qk_norm": capture(True)}
        t = {k: [] for k in graphs}
        for _ in range(a.rounds):
            for k, gr in graphs.items():
                t[k].append(time_us(gr))
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        print(json.dumps({"kernel": "rope_cache", "rows": T, "splits": S, "kv_fp8": a.kv_fp8,
                          "no_kv": a.no_kv, "rounds": a.rounds,
                          "us_base": round(med["base"], 2), "us_qk_norm": round(med["qk_norm"], 2),
                          "ratio": round(med["qk_norm"] / med["base"], 3),
                          "us_base_min_max": [round(min(t["base"]), 2), round(max(t["base"]), 2)],
                          "us_qk_norm_min_max": [round(min(t["qk_norm"]), 2),
                                                 round(max(t["qk_norm"]), 2)]}), flush=True)
        return
    us = time_us(capture(False))
    print(json.dumps({"kernel": "rope_cache", "rows": T, "splits": S, "kv_fp8": a.kv_fp8, "no_kv": a.no_kv,
                      "us": round(us, 2), "TBps": round(nbytes / us / 1e6, 2)}), flush=True)


if __name__ == "__main__":
    main()
