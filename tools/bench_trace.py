#!/usr/bin/env python3
"""Time the alignment traceback (chiron_align_trace, csrc/trace.hip) next to the counts-only alignment it rests on, on the workload
of tools/bench_assess.py: 2048 seeded pairs of 10 000-base reads against references mutated at 12 %.

  pairs        assess.align_pairs alone: (E, M) per pair, one chiron_align_pairs launch
  pairs+trace  assess.align_ops: the same align_pairs call, then the traced sweep and the walk for every pair, in as many
               chiron_align_trace calls as --workspace-mb asks for

Each timing is the host clock around the Python call (coding, packing, copies, launches, synchronise).  After one warm-up call of
each, the two alternate for --rounds rounds in the same process; the medians, their ratio, the workspace bytes the planner asked
for and the number of trace calls are written as one JSON record.  The first --check-pairs pairs are compared with the reference
walk of tests/trace_ref.py.

    python tools/bench_trace.py [--pairs 2048] [--length 10000] [--rounds 5] [--workspace-mb 4096] [--out profiles/trace.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2048)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--rate", type=float, default=0.12)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--workspace-mb", dest="workspace_mb", type=int, default=4096)
    ap.add_argument("--check-pairs", dest="check_pairs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_trace.py measures the GPU kernel: no GPU, no number")
    from chiron_amd import assess
    from bench_assess import mutate_codes
    import trace_ref

    rng = np.random.default_rng(20240)
    reads = [rng.integers(0, 4, args.length).astype(np.uint8) for _ in range(args.pairs)]
    refs = [mutate_codes(r, args.rate, rng) for r in reads]

    rows = assess.align_pairs(reads, refs)                 # warm-up: code object load, allocator
    ops = assess.align_ops(reads, refs, args.workspace_mb)
    plan = assess.plan_trace_batches(rows["read_len"], rows["ref_len"], rows["edit"], args.workspace_mb << 20)
    times = {"pairs": [], "pairs_and_trace": []}
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        got = assess.align_pairs(reads, refs)
        times["pairs"].append(time.perf_counter() - t0)
        if got.tobytes() != rows.tobytes():
            sys.exit("bench_trace.py: align_pairs changed between runs")
        t0 = time.perf_counter()
        again = assess.align_ops(reads, refs, args.workspace_mb)
        times["pairs_and_trace"].append(time.perf_counter() - t0)
        if any(x.tobytes() != y.tobytes() for x, y in zip(ops, again)):
            sys.exit("bench_trace.py: align_ops changed between runs")

    to_str = lambda c: "".join(np.array(list("ACGT"))[c])   # noqa: E731
    for k in range(min(args.check_pairs, args.pairs)):
        if trace_ref.trace(to_str(reads[k]), to_str(refs[k])).tobytes() != ops[k].tobytes():
            sys.exit("bench_trace.py: pair %d differs from the reference walk" % k)

    med = {k: float(np.median(v)) for k, v in times.items()}
    sizes = [assess.trace_pair_size(int(r["read_len"]), int(r["ref_len"]), int(r["edit"])) for r in rows]
    record = {"workload": {"pairs": args.pairs, "length": args.length, "mutation_rate": args.rate, "seed": 20240},
              "timing": "host clock around assess.align_pairs and assess.align_ops (which runs align_pairs first); %d rounds, the two "
                        "alternating, after one warm-up call each" % args.rounds,
              "device": torch.cuda.get_device_name(0),
              "pairs": {"seconds_median": med["pairs"], "seconds_min": float(min(times["pairs"])), "seconds_max": float(max(times["pairs"]))},
              "pairs_and_trace": {"seconds_median": med["pairs_and_trace"], "seconds_min": float(min(times["pairs_and_trace"])),
                                  "seconds_max": float(max(times["pairs_and_trace"]))},
              "pairs_and_trace_over_pairs": med["pairs_and_trace"] / med["pairs"],
              "trace_seconds_median": med["pairs_and_trace"] - med["pairs"],
              "workspace_mb": args.workspace_mb, "trace_calls": len(plan), "workspace_bytes_planned": [int(nb) for _, nb in plan],
              "backpointer_bytes": int(sum(s[0] for s in sizes)), "band_diagonals_mean": float(np.mean([s[1] for s in sizes])),
              "columns": int(sum(len(o) for o in ops)), "pairs_checked_against_the_reference_walk": min(args.check_pairs, args.pairs)}
    print(json.dumps(record))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
