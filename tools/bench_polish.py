#!/usr/bin/env python
"""Time chiron_ctc_score (csrc/ctc_score.hip) on the shape `polish` meets: 2048 candidate variants on reads of 10,000 bases --
`--depth` synthetic reads (dwell geometric with mean 9 frames a base, the true base's class raised by 6 over N(0,1) noise), every
variant scored by every read against two alleles of 2 * 8 + 1 bases, the frames of each window found as `polish` finds them (here
from the planted dwell, not from a forced alignment).  One chiron_ctc_score call over all items (polish.score_call) is timed; for
context the same (segment, allele) pairs are run through ctc.ctc_loss, which wants them dense -- every segment copied once per
allele and padded to the longest -- and the numpy restatement of tests/polish_ref.py scores a sample on the CPU, where the GPU's
values must agree with it within 1e-9.  Rounds are interleaved and reported by their medians; the result goes to
profiles/polish.json.  The tool sets no bar.  Needs a GPU: there is nothing to time without one."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_read(rng, lab, mean_dwell):
    """-> (scores float32 [F, 5], start int64 [bases + 1]: the first frame of every base, then F)."""
    dwell = rng.geometric(1.0 / mean_dwell, size=len(lab))
    classes, start = [], []
    for j in range(len(lab)):
        if j and lab[j] == lab[j - 1]:
            classes.append(4)
        start.append(len(classes))
        classes += [int(lab[j])] * int(dwell[j])
    F = len(classes)
    x = rng.standard_normal((F, 5)).astype(np.float32)
    x[np.arange(F), classes] += np.float32(6)
    return x, np.array(start + [F], dtype=np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", type=int, default=2048)
    ap.add_argument("--bases", type=int, default=10000)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--dwell", type=float, default=9.0)
    ap.add_argument("--flank", type=int, default=8)
    ap.add_argument("--workspace-mb", dest="workspace_mb", type=int, default=4096)
    ap.add_argument("--cpu-items", dest="cpu_items", type=int, default=256, help="items the numpy reference scores per round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polish.json"))
    args = ap.parse_args()
    import torch
    from chiron_amd import ctc, polish
    import polish_ref as ref
    if not torch.cuda.is_available():
        sys.exit("bench_polish: no GPU")
    rng = np.random.default_rng(20261019)
    f = args.flank
    genome = rng.integers(0, 4, size=args.bases).astype(np.uint8)
    sites = np.sort(rng.choice(np.arange(f, args.bases - f), size=args.variants, replace=False))
    items, cands, parts, frame0 = [], [], [], 0
    for _ in range(args.depth):                                    # items in frame order: read after read, site after site
        x, start = make_read(rng, genome, args.dwell)
        parts.append(x)
        for g in sites:
            allele = genome[g - f:g + f + 1]
            alt = allele.copy()
            alt[f] = (alt[f] + 1) % 4
            items.append((frame0 + int(start[g - f]), frame0 + int(start[g + f + 1])))
            cands.append([allele, alt])
        frame0 += len(x)
    scores = np.concatenate(parts)
    keep = [i for i, (b, e) in enumerate(items) if e - b <= polish.MAX_FRAMES]
    items, cands = [items[i] for i in keep], [cands[i] for i in keep]
    n_cand = 2 * len(items)
    ws_bytes = polish.workspace_size(scores.shape[0], len(items), n_cand, n_cand * (2 * f + 1))
    if ws_bytes > args.workspace_mb << 20:
        sys.exit("bench_polish: one call needs %d bytes of workspace, --workspace-mb allows %d" % (ws_bytes, args.workspace_mb << 20))
    # the dense form ctc_loss takes: [candidates, longest segment, 5], labels [candidates, longest allele]
    T = np.array([e - b for b, e in items for _ in range(2)], dtype=np.int32)
    dense = np.zeros((n_cand, int(T.max()), 5), dtype=np.float32)
    labels = np.zeros((n_cand, 2 * f + 1), dtype=np.int32)
    for i, ((b, e), pair) in enumerate(zip(items, cands)):
        for k in range(2):
            dense[2 * i + k, :e - b] = scores[b:e]
            labels[2 * i + k] = pair[k]
    label_len = np.full(n_cand, 2 * f + 1, dtype=np.int32)
    sample = list(range(0, len(items), max(len(items) // args.cpu_items, 1)))[:args.cpu_items]

    def gpu():
        out = polish.score_call(scores, items, cands)      # ONE chiron_ctc_score call; it synchronises its stream itself
        return out[0]

    def gpu_dense():
        loss = ctc.ctc_loss(dense, T, labels, label_len)
        torch.cuda.synchronize()
        return loss

    def cpu():
        return ref.score(scores, [items[i] for i in sample], [cands[i] for i in sample])

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t0) * 1e3, out

    for _ in range(args.warmup):
        gpu()
        gpu_dense()
    gpu_ms, dense_ms, cpu_ms = [], [], []
    for _ in range(args.rounds):          # interleaved: all three see the same machine state
        t, got = timed(gpu)
        gpu_ms.append(t)
        t, loss = timed(gpu_dense)
        dense_ms.append(t)
        t, want = timed(cpu)
        cpu_ms.append(t)
    worst = 0.0
    for k, i in enumerate(sample):
        for a, b in zip(got[2 * i:2 * i + 2], want["loglik"][k]):
            worst = max(worst, abs(a - b) / max(1.0, abs(b)))
    assert worst <= 1e-9, "the GPU and the numpy reference differ by %g relative" % worst
    flat = got
    float_gap = float(np.max(np.abs(-np.asarray(loss, dtype=np.float64) - flat) / np.maximum(1.0, np.abs(flat))))
    med = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    result = {"device": torch.cuda.get_device_name(0), "variants": args.variants, "bases_per_read": args.bases, "depth": args.depth,
              "flank": f, "items": len(items), "candidates": n_cand, "frames_total": int(scores.shape[0]),
              "frames_per_item": {"mean": float(T.mean()), "max": int(T.max())},
              "workspace_bytes": int(ws_bytes), "rounds": args.rounds,
              "gpu_ms": med(gpu_ms), "gpu_us_per_candidate": float(np.median(gpu_ms)) * 1e3 / n_cand,
              "dense_ctc_loss_ms": med(dense_ms), "dense_bytes": int(dense.nbytes), "ragged_bytes": int(scores.nbytes),
              "dense_float_loss_vs_double_loglik_max_rel": float_gap,
              "numpy_cpu_items": len(sample), "numpy_cpu_ms_per_candidate": float(np.median(cpu_ms)) / (2 * len(sample)),
              "gpu_vs_numpy_max_rel": worst,
              "note": "gpu_ms and dense_ctc_loss_ms are whole calls: host checks, copies in, the launches, copies out; building the dense "
                      "tensor on the host is not in dense_ctc_loss_ms; the numpy time is one core, vectorised over the sample"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
