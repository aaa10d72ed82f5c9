#!/usr/bin/env python3
"""Time the read-level alignment (chiron_align_pairs, csrc/assess.hip) on a fixed, seeded workload and write one JSON record:

  batch     2048 pairs of 10 000-base reads against references mutated at 12 % (substitutions, insertions and deletions, a third
            each; E / m comes out near 0.10), all in one call
  example   five pairs of the sizes of the example reads (2 589, 10 814, 5 551, 13 052, 11 384 bases), same mutation rate

Each timing is the host clock around assess.align_pairs: coding, packing, the copy to the device, the one launch, the copy back
and the synchronise -- what a user of `chiron assess` waits for.  After one warm-up call per workload the two workloads
alternate for --rounds rounds; the median is reported with the spread.  cell rates are given twice: band cells the kernel
actually updated (every doubling round counted), and the n x m table the result is worth.

Baseline: the single-thread numpy full-table DP of tests/assess_ref.py on the five example pairs and on --baseline-pairs pairs
of the batch, timed on the same host; its batch figure is the per-pair mean of that subset times 2048, an EXTRAPOLATION, and is
labelled so.  The subset's (E, M) must equal the kernel's.

    python tools/bench_assess.py [--pairs 2048] [--length 10000] [--rounds 5] [--baseline-pairs 3] [--out profiles/assess.json]
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

EXAMPLE_LENGTHS = (2589, 10814, 5551, 13052, 11384)


def mutate_codes(codes, rate, rng):
    """Per base: deleted, substituted by a random base, or followed by a random base, a third of `rate` each."""
    r = rng.random(len(codes))
    kind = np.where(r < rate / 3, 0, np.where(r < 2 * rate / 3, 1, np.where(r < rate, 2, 3)))
    reps = np.array([0, 1, 2, 1])[kind]
    out = np.repeat(codes, reps)
    start = np.cumsum(reps) - reps
    rand = rng.integers(0, 4, len(codes)).astype(np.uint8)
    out[start[kind == 1]] = rand[kind == 1]
    out[start[kind == 2] + 1] = rand[kind == 2]
    return out


def band_cells(n, m, E, band0):
    """Cells the kernel updated for a pair that ends with distance E: every band it tried, first to accepted."""
    d_all = np.arange(-n, m + 1)
    diag_len = np.minimum(n, m - d_all) - np.maximum(0, -d_all) + 1
    total, w = 0, band0
    while True:
        dlo, dhi = max(min(0, m - n) - w, -n), min(max(0, m - n) + w, m)
        total += int(diag_len[dlo + n:dhi + n + 1].sum())
        if (dlo == -n and dhi == m) or E <= 2 * w + 1 + abs(m - n):
            return total, w
        w *= 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2048)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--rate", type=float, default=0.12)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--baseline-pairs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assess.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_assess.py measures the GPU kernel: no GPU, no number")
    from chiron_amd import assess
    import assess_ref

    rng = np.random.default_rng(20240)
    work = {}
    for name, lengths in (("batch", [args.length] * args.pairs), ("example", EXAMPLE_LENGTHS)):
        reads = [rng.integers(0, 4, n).astype(np.uint8) for n in lengths]
        refs = [mutate_codes(r, args.rate, rng) for r in reads]
        work[name] = (reads, refs)

    results, times = {}, {k: [] for k in work}
    for name, (reads, refs) in work.items():            # warm-up: code object load, allocator, every shape of the timed window
        results[name] = assess.align_pairs(reads, refs)
    for _ in range(args.rounds):
        for name, (reads, refs) in work.items():
            t0 = time.perf_counter()
            got = assess.align_pairs(reads, refs)
            times[name].append(time.perf_counter() - t0)
            if got.tobytes() != results[name].tobytes():
                sys.exit("bench_assess.py: %s changed between runs" % name)

    to_str = lambda c: "".join(np.array(list("ACGT"))[c])   # noqa: E731
    record = {"workload": {"pairs": args.pairs, "length": args.length, "mutation_rate": args.rate, "seed": 20240,
                           "example_lengths": list(EXAMPLE_LENGTHS)},
              "timing": "host clock around assess.align_pairs (coding, packing, copies, one launch, synchronise); %d rounds, the two "
                        "workloads alternating, after one warm-up call each" % args.rounds,
              "device": torch.cuda.get_device_name(0)}
    for name, (reads, refs) in work.items():
        got = results[name]
        n, m, E = got["read_len"].astype(np.int64), got["ref_len"].astype(np.int64), got["edit"].astype(np.int64)
        cells = [band_cells(int(a), int(b), int(e), assess.BAND0) for a, b, e in zip(n, m, E)]
        if [c[1] for c in cells] != got["band"].tolist():
            sys.exit("bench_assess.py: the kernel's bands are not the ones the rule gives")
        t = float(np.median(times[name]))
        bands, band_counts = np.unique(got["band"], return_counts=True)
        # baseline subset: every example pair; the first --baseline-pairs pairs of the batch
        sub = range(len(reads)) if name == "example" else range(min(args.baseline_pairs, len(reads)))
        base_s = []
        for k in sub:
            a, b = to_str(reads[k]), to_str(refs[k])
            t0 = time.perf_counter()
            want = assess_ref.full_table(a, b)
            base_s.append(time.perf_counter() - t0)
            if want != (int(got["edit"][k]), int(got["match"][k])):
                sys.exit("bench_assess.py: %s pair %d differs from the reference DP" % (name, k))
        base_total = float(np.mean(base_s)) * len(reads)
        record[name] = {
            "pairs": len(reads), "seconds_median": t, "seconds_min": float(min(times[name])), "seconds_max": float(max(times[name])),
            "pairs_per_second": len(reads) / t,
            "band_cell_updates_per_second": sum(c[0] for c in cells) / t,
            "table_cells_per_second": float((n * m).sum()) / t,
            "band_cells_over_table_cells": sum(c[0] for c in cells) / float(max((n * m).sum(), 1)),
            "edit_over_ref_len_mean": float(np.mean(E / np.maximum(m, 1))),
            "final_band_distribution": {str(int(b)): int(c) for b, c in zip(bands, band_counts)},
            "baseline": {"what": "tests/assess_ref.py full_table (numpy, one thread), same host",
                         "pairs_timed": len(base_s), "seconds_per_pair_mean": float(np.mean(base_s)),
                         "seconds_for_the_workload": base_total,
                         "extrapolated": len(base_s) != len(reads),
                         "speedup_over_baseline": base_total / t},
        }
    line = json.dumps(record)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
