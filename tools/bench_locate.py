#!/usr/bin/env python
"""Time chiron_signal_locate (csrc/locate.hip) on the shape `locate` meets: 2048 synthetic queries of 2000 samples against both
strands of a random 50 kb genome under a random 5-mer table (sd 15 x 25.6 int16 units) -- 100,001 columns, 4.1 x 10^11 cells.  A
query walks the row from a random column at a geometric dwell of mean 9, its samples the columns' levels plus noise of sd 3 x 25.6.
One chiron_signal_locate call is timed, arrays prepared beforehand: the host's checking walk, the copies in, the launches, the copy
out.  Against it, in the same run, the numpy rows of tests/locate_ref.py on one core over the first --ref-queries queries, scaled to
the whole by cells; its triples must equal the library's on those queries or the tool exits non-zero.  The rounds alternate -- a
library call, then the numpy subset -- and the medians of --rounds rounds after a warm-up are taken.  The result goes to
profiles/locate.json.

The one performance condition is checked here: the ratio numpy over library call must be above 1, or the tool exits non-zero.
--library-only times nothing and runs the call --rounds times: the form to put behind `rocprofv3 --kernel-trace --stats`, whose
kernel time goes to profiles/locate_kernel_trace.txt.  Needs a GPU: there is nothing to time without one."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_case(rng, genome_len, queries, q_len, mean_dwell):
    """(int32 row, column map, int16 [queries, q_len], the column of every query's last sample)."""
    from chiron_amd import locate, map as map_mod
    genome = map_mod.Genome([("ctg", "".join("ACGT"[v] for v in rng.integers(0, 4, genome_len)))])
    table = np.clip(np.rint(25.6 * 15.0 * rng.standard_normal(4 ** 5)), -32767, 32767).astype(np.int32)
    row, cmap = locate.reference_levels(genome, table, 5)
    flat = np.where(row == locate.BREAK, 0, row).astype(np.int64)
    span = q_len                                                     # a walk moves at most one column a sample
    first = np.where(rng.integers(0, 2, queries) == 0, rng.integers(2, genome_len - span, queries),
                     genome_len + 3 + rng.integers(0, genome_len - span - 3, queries))
    cols = first[:, None] + np.cumsum(rng.random((queries, q_len)) < 1.0 / mean_dwell, axis=1)
    x = flat[cols] + rng.normal(0.0, 25.6 * 3.0, (queries, q_len))
    return row, cmap, np.clip(np.rint(x), -32767, 32767).astype(np.int16), cols[:, -1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=2000)
    ap.add_argument("--genome", type=int, default=50000)
    ap.add_argument("--dwell", type=float, default=9.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ref-queries", dest="ref_queries", type=int, default=1, help="queries the numpy reference runs on; its time is scaled by cells")
    ap.add_argument("--library-only", dest="library_only", action="store_true", help="only run the call --rounds times, write nothing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "locate.json"))
    args = ap.parse_args()
    import torch
    from chiron_amd import _lib, locate
    import locate_ref as ref
    if not torch.cuda.is_available():
        sys.exit("bench_locate: no GPU")
    rng = np.random.default_rng(20261020)
    row, cmap, x, true_end = make_case(rng, args.genome, args.queries, args.samples, args.dwell)
    items, ref_len = args.queries, len(row)
    samples = np.ascontiguousarray(x.reshape(-1))
    sample_off = np.arange(items + 1, dtype=np.int64) * args.samples
    nbytes = locate.workspace_size(items, items * args.samples, ref_len)
    lib, ws, stream = _lib.device_workspace(nbytes, 0, "bench_locate", "locate kernel")
    out = np.zeros((items, locate.blocks_of_ref(ref_len), 3), dtype=np.int32)

    def call():
        _lib.check(lib.chiron_signal_locate(0, samples.ctypes.data, sample_off.ctypes.data, items, row.ctypes.data, ref_len, out.ctypes.data, ws.data_ptr(),
                                            nbytes, 0, stream))

    launches = (args.samples + locate.CHUNK - 1) // locate.CHUNK
    cells = items * args.samples * ref_len
    if args.library_only:
        for _ in range(args.rounds):
            call()
        print("bench_locate: %d calls of %d queries of %d samples on %d columns, %d launches each" % (args.rounds, items, args.samples, ref_len, launches))
        return
    torch.set_num_threads(1)
    for _ in range(args.warmup):
        call()
    sub = min(args.ref_queries, items)
    call_ms, numpy_sub_ms = [], []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        call()
        call_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        want = ref.locate(list(x[:sub]), row)
        numpy_sub_ms.append((time.perf_counter() - t0) * 1e3)
        if not np.array_equal(out[:sub], want):
            sys.exit("bench_locate: the library call and the numpy reference differ on the first %d queries" % sub)
    summary = [locate.summarise(b, args.samples) for b in out]
    end_err = np.array([abs(s["best"][1] - t) for s, t in zip(summary, true_end)])
    margins = np.array([s["margin"] for s in summary if s["margin"] is not None])
    med = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    numpy_ms = float(np.median(numpy_sub_ms)) * items / sub                                 # every query has the same cells
    ratio = numpy_ms / float(np.median(call_ms))
    result = {"device": torch.cuda.get_device_name(0), "queries": items, "samples_per_query": args.samples, "genome": args.genome, "columns": ref_len,
              "mean_dwell": args.dwell, "cells": cells, "launches": launches, "workspace_bytes": int(nbytes), "rounds": args.rounds,
              "call_ms": med(call_ms), "cells_per_second": cells / (float(np.median(call_ms)) * 1e-3), "numpy_queries": sub,
              "numpy_subset_ms": med(numpy_sub_ms), "numpy_ms_scaled": numpy_ms, "numpy_over_call": ratio,
              "ends_within_3_columns": float((end_err <= 3).mean()), "ends_within_32_columns": float((end_err <= 32).mean()),
              "margin": med(margins) if len(margins) else None, "queries_with_margin": int(len(margins)),
              "note": "call_ms is the whole library call on prepared arrays: the host's checking walk, copies in, the launches, the copy out; "
                      "numpy_ms_scaled is tests/locate_ref.py's numpy rows on one core over numpy_queries queries, scaled to all by cells"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result))
    if not ratio > 1.0:
        sys.exit("bench_locate: the library call is not faster than the numpy reference on one core")


if __name__ == "__main__":
    main()
