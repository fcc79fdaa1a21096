#!/usr/bin/env python3
"""Times of the sampling controls on one MI355X -> profiles/sampling/penalties.json.

* ``ops.sample`` at 512 x 128256 bf16, greedy and top-p 0.9, without min-p (the kernels every
  request without the controls runs) and with an all-zero / 0.05 min-p;
* ``ops.apply_penalties`` at 512 x 128256 with 0, 1 and 512 penalised rows (64 slots, 600 seen
  tokens per slot), and ``ops.penalty_update``;
* ``ops.penalty_feed`` of one 8192-token chunk (reset + prompt segment).

Every case is captured in a hipGraph of ``--launches`` launches and the graph is timed with
device events, ``--repeats`` times, the cases interleaved; the record keeps min / median / max,
so the run-to-run spread stands next to every figure.  (penalty_feed uploads its segment list, so
it is timed eagerly around a synchronise.)  A comparison with a build of the parent commit is not
part of this script: run it on both builds in one session and compare the ``sample`` records.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_llm_inference import ops  # noqa: E402


def graph_of(fn, launches):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for _ in range(launches):
            fn()
    return g


def time_graph(g, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches   # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join("profiles", "sampling", "penalties.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: times are not measured anywhere else")
    ops.native()
    dev = torch.device("cuda:0")
    B, V, S = a.rows, a.vocab, 64
    g = torch.Generator(device=dev).manual_seed(1)
    logits = (torch.randn(B, V, device=dev, generator=g) * 3).to(torch.bfloat16)
    work = logits.clone()
    zeros = torch.zeros(B, device=dev)
    t08 = torch.full((B,), 0.8, device=dev)
    p09 = torch.full((B,), 0.9, device=dev)
    seeds = torch.arange(B, device=dev, dtype=torch.int64)
    ctr = torch.arange(B, device=dev, dtype=torch.int64) + 100
    out = torch.empty(B, dtype=torch.int32, device=dev)
    table = ops.penalty_table(S, V, dev)
    for s in range(S):
        ops.penalty_feed(table, [(s, 0, 1, 300), (s, 1, 0, 300)],
                         torch.randint(0, V, (600,), generator=torch.Generator().manual_seed(s),
                                       dtype=torch.int32))
    one = torch.full((B,), 1.1, device=dev)
    half = torch.full((B,), 0.5, device=dev)
    slot_none = torch.full((B,), -1, dtype=torch.int32, device=dev)
    slot_one = slot_none.clone()
    slot_one[B // 2] = 3
    slot_all = (torch.arange(B, device=dev) % S).to(torch.int32)
    scratch = table.clone()

    def sample(temp, top_p, min_p=None):
        return lambda: ops.sample(logits, temperature=temp, top_p=top_p, seeds=seeds,
                                  counters=ctr, out=out, min_p=min_p)

    def apply(slots):
        return lambda: ops.apply_penalties(work, table, slots, one, half, half)

    cases = {
        "sample_greedy": sample(zeros, None),
        "sample_top_p_0.9": sample(t08, p09),
        "sample_top_p_0.9_min_p_zero": sample(t08, p09, zeros),
        "sample_top_p_0.9_min_p_0.05": sample(t08, p09, torch.full((B,), 0.05, device=dev)),
        "penalty_apply_0_rows": apply(slot_none),
        "penalty_apply_1_row": apply(slot_one),
        f"penalty_apply_{B}_rows": apply(slot_all),
        "penalty_update": lambda: ops.penalty_update(scratch, slot_all, out),
    }
    graphs = {k: graph_of(f, a.launches) for k, f in cases.items()}
    times = {k: [] for k in cases}
    for _ in range(a.repeats):          # interleaved: every case sees the same drift
        for k, gr in graphs.items():
            times[k].append(time_graph(gr, a.launches))
    chunk = torch.randint(0, V, (8192,), dtype=torch.int32).to(dev)
    feed = []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.penalty_feed(scratch, [(5, 0, 1, 8192)], chunk)
        torch.cuda.synchronize()
        feed.append((time.perf_counter() - t0) * 1e6)
    times["penalty_feed_8192_tokens_eager_with_sync"] = feed
    rec = {"device": torch.cuda.get_device_name(0), "rows": B, "vocab": V, "slots": S,
           "launches_per_graph": a.launches, "repeats": a.repeats, "unit": "us per launch",
           "parent_build": "not measured",
           "cases": {k: {"min": round(min(v), 2), "median": round(statistics.median(v), 2),
                         "max": round(max(v), 2)} for k, v in times.items()}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
