#!/usr/bin/env python
"""Time chiron_signal_refine (csrc/refine.hip) on the shape `squiggle --refine` meets: the generator of tools/bench_squiggle.py,
2048 synthetic reads of 10,000 bases at a geometric dwell of mean 9 -- 2.0 x 10^7 bases, 1.8 x 10^8 samples, 1.3 x 10^9 cells of
64 candidates a border -- each read one item.  A base's samples are the level of its 5-mer in a random table (sd 15 x 25.6 int16
units) plus noise; the starts handed in are the true ones jittered by up to 6 samples and sorted.  One chiron_signal_refine call is
timed, arrays prepared beforehand: the host's checking walk, the copies in, the launch, the copies out; median of --rounds calls
after a warm-up.  Against it, in the same run, the numpy rows of tests/refine_ref.py on one core over the first --ref-reads reads,
scaled to the whole by cells; its results must equal the library's on those reads or the tool exits non-zero.  The result goes to
profiles/refine.json.

The one performance condition is checked here: the ratio numpy over library call must be above 1, or the tool exits non-zero.
--library-only times nothing and runs the call --rounds times: the form to put behind `rocprofv3 --kernel-trace --stats`, whose
kernel time goes to profiles/refine_kernel_trace.txt.  Needs a GPU: there is nothing to time without one."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_items(rng, reads, bases, mean_dwell, jitter):
    """The flat arrays of the call: (samples, sample_off, level, start_in, base_off) and the true starts [reads, bases + 1]."""
    dwell = rng.geometric(1.0 / mean_dwell, (reads, bases)).astype(np.int64)
    true = np.zeros((reads, bases + 1), dtype=np.int64)
    np.cumsum(dwell, axis=1, out=true[:, 1:])
    sample_off = np.concatenate([[0], np.cumsum(true[:, -1])]).astype(np.int64)
    table = np.rint(25.6 * 15.0 * rng.standard_normal(4 ** 5)).astype(np.int32)
    codes = rng.integers(0, 4, (reads, bases + 4))
    kmer = sum(codes[:, j:j + bases] * 4 ** (4 - j) for j in range(5))
    level = table[kmer].astype(np.int32)                                                   # [reads, bases]
    samples = np.empty(int(sample_off[-1]) + 1, dtype=np.int16)
    samples[-1] = 0
    for r in range(reads):
        x = np.repeat(level[r], dwell[r]) + rng.normal(0.0, 25.6 * 3.0, int(true[r, -1]))
        samples[sample_off[r]:sample_off[r + 1]] = np.clip(np.rint(x), -32767, 32767)
    start = true.copy()
    start[:, 1:-1] = np.sort(np.clip(true[:, 1:-1] + rng.integers(-jitter, jitter + 1, (reads, bases - 1)), 0, true[:, -1:]), axis=1)
    base_off = np.arange(reads + 1, dtype=np.int64) * bases
    flat = lambda a, t: np.ascontiguousarray(np.concatenate([a.reshape(-1).astype(t), np.zeros(1, t)]))
    return samples, sample_off, flat(level, np.int32), flat(start, np.int32), base_off, true


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2048)
    ap.add_argument("--bases", type=int, default=10000)
    ap.add_argument("--dwell", type=float, default=9.0)
    ap.add_argument("--jitter", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ref-reads", dest="ref_reads", type=int, default=8, help="reads the numpy reference runs on; its time is scaled by cells")
    ap.add_argument("--library-only", dest="library_only", action="store_true", help="only run the call --rounds times, write nothing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine.json"))
    args = ap.parse_args()
    import torch
    from chiron_amd import _lib, squiggle
    import refine_ref as ref
    if not torch.cuda.is_available():
        sys.exit("bench_refine: no GPU")
    rng = np.random.default_rng(20261020)
    samples, sample_off, level, start, base_off, true = make_items(rng, args.reads, args.bases, args.dwell, args.jitter)
    n_bases, n_samples = int(base_off[-1]), int(sample_off[-1])
    nbytes = squiggle.refine_workspace_size(args.reads, n_samples, n_bases)
    lib, ws, stream = _lib.device_workspace(nbytes, 0, "bench_refine", "refine kernel")
    out = np.zeros(n_bases + args.reads, dtype=np.int32)
    cost = np.zeros(args.reads, dtype=np.int64)

    def call():
        _lib.check(lib.chiron_signal_refine(0, samples.ctypes.data, sample_off.ctypes.data, level.ctypes.data, start.ctypes.data, base_off.ctypes.data,
                                            args.reads, 0, out.ctypes.data, cost.ctypes.data, ws.data_ptr(), stream))

    if args.library_only:
        for _ in range(args.rounds):
            call()
        print("bench_refine: %d calls of %d items, %d bases, %d samples" % (args.rounds, args.reads, n_bases, n_samples))
        return
    torch.set_num_threads(1)
    for _ in range(args.warmup):
        call()
    call_ms = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        call()
        call_ms.append((time.perf_counter() - t0) * 1e3)
    sub = min(args.ref_reads, args.reads)
    item = lambda r: (samples[sample_off[r]:sample_off[r + 1]], level[base_off[r]:base_off[r + 1]], start[base_off[r] + r:base_off[r + 1] + r + 1])
    t0 = time.perf_counter()
    want, want_cost = ref.refine(*zip(*[item(r) for r in range(sub)]))
    numpy_sub_ms = (time.perf_counter() - t0) * 1e3
    rows = out.reshape(args.reads, args.bases + 1)
    if not (np.array_equal(rows[:sub], np.array(want)) and np.array_equal(cost[:sub], want_cost)):
        sys.exit("bench_refine: the library call and the numpy reference differ on the first %d reads" % sub)
    numpy_ms = numpy_sub_ms * n_bases / (sub * args.bases)                                  # 64 cells a base row: scaling by cells is scaling by bases
    ok = cost != squiggle.INFEASIBLE
    inner = lambda a: a[ok][:, 1:-1]
    med = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    ratio = numpy_ms / float(np.median(call_ms))
    result = {"device": torch.cuda.get_device_name(0), "items": args.reads, "bases_per_item": args.bases, "mean_dwell": args.dwell, "jitter": args.jitter,
              "bases": n_bases, "samples": n_samples, "cells": 64 * n_bases, "workspace_bytes": int(nbytes), "rounds": args.rounds,
              "call_ms": med(call_ms), "numpy_reads": sub, "numpy_subset_ms": numpy_sub_ms, "numpy_ms_scaled": numpy_ms, "numpy_over_call": ratio,
              "call_ns_per_base": float(np.median(call_ms)) * 1e6 / n_bases, "infeasible": int((~ok).sum()),
              "exact_borders_in": float((inner(start[:-1].reshape(args.reads, -1)) == inner(true)).mean()),
              "exact_borders_out": float((inner(rows) == inner(true)).mean()),
              "note": "call_ms is the whole library call on prepared arrays: the host's checking walk, copies in, the launch, copies out; "
                      "numpy_ms_scaled is tests/refine_ref.py's numpy rows on one core over numpy_reads reads, scaled to all by cells"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result))
    if not ratio > 1.0:
        sys.exit("bench_refine: the library call is not faster than the numpy reference on one core")


if __name__ == "__main__":
    main()
