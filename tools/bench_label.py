#!/usr/bin/env python
"""Time chiron_ctc_align (csrc/ctc_align.hip) on the shape `label` meets: 512 synthetic reads of 4,000 bases at about 9 frames a
base (dwell geometric with mean 9), the true base's class raised by 6 over N(0,1) noise, the command's default band (256, doubling
to 8192 at most) and workspace budget, so the reads go through label.plan_batches as the command's do.  In the same run the
vectorised numpy restatement of tests/ctc_align_ref.py aligns a subset of the reads one at a time on the CPU, and its results
must equal the GPU's.  The two are timed in interleaved rounds and reported by their medians; the result, the band distribution
and the workspace bytes go to profiles/label.json.  Needs a GPU: there is nothing to time without one."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_read(rng, bases, mean_dwell):
    lab = rng.integers(0, 4, size=bases).astype(np.uint8)
    dwell = rng.geometric(1.0 / mean_dwell, size=bases)
    classes = []
    for j in range(bases):
        if j and lab[j] == lab[j - 1]:
            classes.append(4)
        classes += [int(lab[j])] * int(dwell[j])
    F = len(classes)
    x = rng.standard_normal((F, 5)).astype(np.float32)
    x[np.arange(F), classes] += np.float32(6)
    return x, lab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=512)
    ap.add_argument("--bases", type=int, default=4000)
    ap.add_argument("--dwell", type=float, default=9.0)
    ap.add_argument("--band", type=int, default=256)
    ap.add_argument("--max-band", dest="max_band", type=int, default=8192)
    ap.add_argument("--workspace-mb", dest="workspace_mb", type=int, default=4096)
    ap.add_argument("--cpu-reads", dest="cpu_reads", type=int, default=2, help="reads the numpy reference aligns per round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label.json"))
    args = ap.parse_args()
    import torch
    from chiron_amd import label
    import ctc_align_ref as ref
    if not torch.cuda.is_available():
        sys.exit("bench_label: no GPU")
    rng = np.random.default_rng(20261017)
    reads = [make_read(rng, args.bases, args.dwell) for _ in range(args.reads)]
    xs, labs = [r[0] for r in reads], [r[1] for r in reads]
    frames, bases = [x.shape[0] for x in xs], [len(l) for l in labs]
    batches = label.plan_batches(frames, bases, args.band, args.max_band, args.workspace_mb << 20)
    ws_bytes = [label.workspace_size([frames[i] for i in b], [bases[i] for i in b], args.band, args.max_band) for b in batches]

    def gpu():
        out = [None] * len(xs)
        for b in batches:
            got = label.align([xs[i] for i in b], [labs[i] for i in b], band0=args.band, max_band=args.max_band)
            for k, i in enumerate(b):
                out[i] = (got["start"][k], got["score"][k], int(got["band"][k]), int(got["status"][k]))
        torch.cuda.synchronize()
        return out

    def cpu():
        return [ref.align_one(xs[i], labs[i], args.band, args.max_band) for i in range(min(args.cpu_reads, len(xs)))]

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t0) * 1e3, out

    for _ in range(args.warmup):
        gpu()
    gpu_ms, cpu_ms = [], []
    for _ in range(args.rounds):          # interleaved: both see the same machine state
        t, got = timed(gpu)
        gpu_ms.append(t)
        t, want = timed(cpu)
        cpu_ms.append(t)
    for i, w in enumerate(want):
        g = got[i]
        assert np.array_equal(g[0], w[0]) and g[1] == w[1] and g[2:] == (w[2], w[3]), "read %d: the GPU and the numpy reference differ" % i
    bands, counts = np.unique([g[2] for g in got], return_counts=True)
    n_cpu = len(want)
    result = {"device": torch.cuda.get_device_name(0), "reads": len(xs), "bases_per_read": args.bases, "frames_total": int(sum(frames)),
              "band0": args.band, "max_band": args.max_band, "batches": len(batches), "workspace_bytes_max": int(max(ws_bytes)),
              "workspace_bytes_sum": int(sum(ws_bytes)), "rounds": args.rounds,
              "gpu_ms": {"median": float(np.median(gpu_ms)), "min": float(np.min(gpu_ms)), "max": float(np.max(gpu_ms))},
              "gpu_ms_per_read": float(np.median(gpu_ms)) / len(xs),
              "numpy_cpu_reads": n_cpu,
              "numpy_cpu_ms_per_read": float(np.median(cpu_ms)) / max(n_cpu, 1),
              "band_distribution": {str(int(b)): int(c) for b, c in zip(bands, counts)},
              "status_counts": {str(s): int(sum(1 for g in got if g[3] == s)) for s in (0, 1, 2)},
              "gpu_equals_numpy_on_cpu_reads": True,
              "note": "gpu_ms is the whole call per batch: host checks, copies in, the launch, copies out; the numpy time is one core"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
