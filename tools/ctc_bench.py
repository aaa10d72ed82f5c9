#!/usr/bin/env python3
"""Time the CTC kernels (csrc/ctc_loss.hip) at the headline geometry -- batch 1100, T = 400 frames, about 45 labels per window --
with torch.cuda.Event around each call, after warm-up, and print one JSON line:
  loss_ms        chiron_ctc_loss, loss only
  loss_grad_ms   chiron_ctc_loss with CHIRON_CTC_WANT_GRAD (alpha to the workspace, beta + posteriors)
  score_ms       Engine.score on a collected DNA_default batch (label upload, loss, edit distance, copies, synchronise)
  batch_ms       the same engine's submit + collect of that batch (greedy), for the share score adds
Each call includes chiron_ctc_loss's read-back of the int32 operands (the argument check).

    python tools/ctc_bench.py [--batch 1100] [--T 400] [--labels 45] [--iters 20]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, iters, torch):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(iters):
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1100)
    ap.add_argument("--T", type=int, default=400)
    ap.add_argument("--labels", type=int, default=45)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import chiron_amd as ca
    from chiron_amd import ctc
    B, T = args.batch, args.T
    rng = np.random.default_rng(0)
    dev = torch.device("cuda", 0)
    x = torch.tensor(rng.normal(scale=3.0, size=(B, T, 5)).astype(np.float32), device=dev)
    sl = torch.full((B,), T, dtype=torch.int32, device=dev)
    ll_h = rng.integers(args.labels - 8, args.labels + 9, B).astype(np.int32)
    lab_h = rng.integers(0, 4, (B, int(ll_h.max()))).astype(np.int32)
    lab = torch.tensor(lab_h, device=dev)
    ll = torch.tensor(ll_h, device=dev)
    out = {"batch": B, "T": T, "labels_mean": float(ll_h.mean())}
    out["loss_ms"] = timed(lambda: ctc.ctc_loss(x, sl, lab, ll), args.iters, torch)
    out["loss_grad_ms"] = timed(lambda: ctc.ctc_loss(x, sl, lab, ll, want_grad=True), args.iters, torch)
    spec = ca.dna_default_spec()
    w = ca.synthetic_weights(spec, seed=7)
    sig = ca.synthetic_signal(1, 390 * B + 400, seed=3)[0]
    xs = np.stack([sig[i * 390:i * 390 + 400] for i in range(B)]).astype(np.float32)
    with ca.Engine(spec, w, max_batch=B, segment_len=400) as eng:
        esl = ca.seq_len_for_engine(np.full(B, 400), eng.ratio)
        out["batch_ms"] = timed(lambda: eng.infer(xs, esl, beam_width=0, want_prob=False), args.iters, torch)
        out["score_ms"] = timed(lambda: eng.score(0, lab_h, ll_h), args.iters, torch)
    out["score_share_of_batch"] = out["score_ms"] / out["batch_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
