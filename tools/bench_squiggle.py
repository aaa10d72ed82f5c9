#!/usr/bin/env python
"""Time chiron_signal_levels (csrc/signal.hip) on the shape `squiggle` meets: 2048 synthetic reads of 10,000 bases at a geometric
dwell of mean 9 -- 2.0 x 10^7 bases, 1.8 x 10^8 samples -- placed on both strands of a 500,000-base genome (10^6 bins).  One
chiron_signal_levels call is timed, arrays prepared beforehand: the host's checking walk and its records, the copies in, the
launch, the copies out.  Against it, in the same run, the numpy formulation of tests/squiggle_ref.py (np.add.reduceat over the
spans, np.add.at into the planes) on one core.  The two results must be equal or the tool exits non-zero.  Rounds alternate between
the two and are reported by their medians; the result goes to profiles/squiggle.json.

The one performance condition is checked here: the ratio numpy over library call must be above 1, or the tool exits non-zero.
--library-only times nothing and runs the call --rounds times: the form to put behind `rocprofv3 --kernel-trace --stats`, whose
kernel time goes to profiles/squiggle_kernel_trace.txt.  Needs a GPU: there is nothing to time without one."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_reads(rng, reads, bases, mean_dwell, genome):
    """The flat arrays of the call: (samples, sample_off, start, base_off, bins, n_bins)."""
    dwell = rng.geometric(1.0 / mean_dwell, (reads, bases)).astype(np.int64)
    start = np.zeros((reads, bases + 1), dtype=np.int64)
    np.cumsum(dwell, axis=1, out=start[:, 1:])
    sample_off = np.concatenate([[0], np.cumsum(start[:, -1])]).astype(np.int64)
    samples = rng.integers(-2000, 2000, int(sample_off[-1]) + 1, dtype=np.int16)
    pos = rng.integers(0, genome - bases + 1, reads)
    strand = rng.integers(0, 2, reads)
    along = np.arange(bases, dtype=np.int64)[None, :]
    g = np.where(strand[:, None] == 1, pos[:, None] + bases - 1 - along, pos[:, None] + along)       # signal order
    bins = (strand[:, None] * genome + g).astype(np.int32)
    bins[rng.random((reads, bases)) < 0.1] = -1                                                       # inserted and clipped bases
    base_off = (np.arange(reads + 1, dtype=np.int64) * bases)
    flat = lambda a, t: np.ascontiguousarray(np.concatenate([a.reshape(-1).astype(t), np.zeros(1, t)]))
    return samples, sample_off, flat(start, np.int32), base_off, flat(bins, np.int32), 2 * genome


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2048)
    ap.add_argument("--bases", type=int, default=10000)
    ap.add_argument("--dwell", type=float, default=9.0)
    ap.add_argument("--genome", type=int, default=500000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--library-only", dest="library_only", action="store_true", help="only run the call --rounds times, write nothing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "squiggle.json"))
    args = ap.parse_args()
    import torch
    from chiron_amd import _lib, squiggle
    import squiggle_ref as ref
    if not torch.cuda.is_available():
        sys.exit("bench_squiggle: no GPU")
    rng = np.random.default_rng(20261020)
    samples, sample_off, start, base_off, bins, n_bins = make_reads(rng, args.reads, args.bases, args.dwell, args.genome)
    n_bases, n_samples = int(base_off[-1]), int(sample_off[-1])
    nbytes = squiggle.workspace_size(args.reads, n_samples, n_bases, n_bins, True)
    lib, ws, stream = _lib.device_workspace(nbytes, 0, "bench_squiggle", "level kernel")
    planes = np.zeros((squiggle.PLANES, n_bins), dtype=np.int64)
    level = np.zeros(n_bases, dtype=np.int32)

    def call():
        _lib.check(lib.chiron_signal_levels(0, samples.ctypes.data, sample_off.ctypes.data, start.ctypes.data, base_off.ctypes.data, bins.ctypes.data,
                                            args.reads, n_bins, 0, planes.ctypes.data, level.ctypes.data, ws.data_ptr(), stream))

    def cpu():
        return ref.reduce_flat(samples, sample_off, start, base_off, bins, n_bins)

    def timed(fn):
        t0 = time.perf_counter()
        got = fn()
        return (time.perf_counter() - t0) * 1e3, got

    if args.library_only:
        for _ in range(args.rounds):
            call()
        print("bench_squiggle: %d calls of %d bases, %d samples" % (args.rounds, n_bases, n_samples))
        return
    torch.set_num_threads(1)
    for _ in range(args.warmup):
        call()
        cpu()
    call_ms, numpy_ms = [], []
    for _ in range(args.rounds):              # alternating: both see the same machine state
        call_ms.append(timed(call)[0])
        t, (want_planes, want_level) = timed(cpu)
        numpy_ms.append(t)
    if not (np.array_equal(planes, want_planes) and np.array_equal(level, want_level)):
        sys.exit("bench_squiggle: the library call and the numpy formulation differ (%d plane elements, %d levels)"
                 % (int((planes != want_planes).sum()), int((level != want_level).sum())))
    med = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    ratio = float(np.median(numpy_ms)) / float(np.median(call_ms))
    result = {"device": torch.cuda.get_device_name(0), "reads": args.reads, "bases_per_read": args.bases, "mean_dwell": args.dwell,
              "bases": n_bases, "samples": n_samples, "bins": n_bins, "events": int(planes[0].sum()), "workspace_bytes": int(nbytes),
              "rounds": args.rounds, "call_ms": med(call_ms), "numpy_ms": med(numpy_ms), "numpy_over_call": ratio,
              "call_ns_per_base": float(np.median(call_ms)) * 1e6 / n_bases, "call_ns_per_sample": float(np.median(call_ms)) * 1e6 / n_samples,
              "note": "call_ms is the whole library call on prepared arrays: the host's checking walk and its records, copies in, the launch, "
                      "copies out; numpy_ms is np.add.reduceat + np.add.at on one core over the same arrays"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result))
    if not ratio > 1.0:
        sys.exit("bench_squiggle: the library call is not faster than the numpy formulation on one core")


if __name__ == "__main__":
    main()
