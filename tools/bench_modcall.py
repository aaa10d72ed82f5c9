#!/usr/bin/env python
"""Time chiron_signal_score (csrc/site_score.hip) on the shape `modcall` meets: the generator of tools/bench_squiggle.py, 2048
synthetic reads of 10,000 bases at a geometric dwell of mean 9, with a planted CG alternative table.  A base's samples are the level
of its 5-mer in a random table (sd 15 x 25.6 int16 units) plus noise; the alternative table shifts every 5-mer that holds CG by N(0,
1 table sd), and every CG group of every read (occurrences fewer than 5 bases apart) is modified with probability 1/2.  Every group
whose window -- 4 bases either side of its sites -- has at most 16 columns and lies inside the read is one segment, cut at the true
borders jittered by up to 6 samples, with two candidates: the canonical row and the alternative one.  About 1.0 x 10^6 segments, 2.0
x 10^6 candidates, 8.7 x 10^7 samples and 1.7 x 10^9 cells.  One chiron_signal_score call is timed, arrays prepared beforehand: the
host's checking walk, the copies in, the launch, the copy out; median of --rounds calls after a warm-up.  Against it, in the same
run, the numpy rows of tests/site_ref.py on one core over the candidates of the first --ref-reads reads, scaled to the whole by
cells (samples times columns); its costs must equal the library's on every one of those candidates or the tool exits non-zero.  The
result goes to profiles/modcall.json.

The one performance condition is checked here: the ratio numpy over library call must be above 1, or the tool exits non-zero.  No
time is promised.  --library-only times nothing and runs the call --rounds times: the form to put behind `rocprofv3 --kernel-trace
--stats`, whose kernel time goes to profiles/modcall_kernel_trace.txt.  Needs a GPU: there is nothing to time without one."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K, FLANK, COLUMNS = 5, 2, 16


def holds_cg(code):
    bases = [(code >> (2 * (K - 1 - j))) & 3 for j in range(K)]
    return any(bases[j] == 1 and bases[j + 1] == 2 for j in range(K - 1))


def make_call(rng, reads, bases, mean_dwell, jitter):
    """The flat arrays of the call -- (samples, sample_off, level, level_off, seg) -- the planted state of every segment and the
    number of segments of every read."""
    table = np.rint(25.6 * 15.0 * rng.standard_normal(4 ** K)).astype(np.int32)
    shift = np.rint(25.6 * 15.0 * rng.standard_normal(4 ** K)).astype(np.int32)
    alt = np.clip(table + np.where([holds_cg(c) for c in range(4 ** K)], shift, 0), -32767, 32767).astype(np.int32)
    h, reach = K // 2, K // 2 + FLANK
    cols = np.arange(COLUMNS)
    sig, lens, rows, widths, truth, per_read = [], [], [], [], [], []
    for _ in range(reads):
        codes = rng.integers(0, 4, bases + K - 1)
        kmer = sum(codes[j:j + bases] * 4 ** (K - 1 - j) for j in range(K))                  # base b is codes[b + h], its 5-mer codes[b .. b + 4]
        occ = np.flatnonzero((codes[:-1] == 1) & (codes[1:] == 2))                          # where a CG begins, in codes
        gid = np.concatenate([[0], np.cumsum(np.diff(occ) >= K)]) if len(occ) else np.zeros(0, np.int64)
        n_groups = int(gid[-1]) + 1 if len(occ) else 0
        state = rng.integers(0, 2, n_groups).astype(bool)
        owner = np.full(len(codes) + K, -1, dtype=np.int64)                                 # the group of the CG that begins at a position
        owner[occ] = gid
        held = np.stack([owner[j:j + bases] for j in range(K - 1)])                         # [4, bases]: the CGs base b's 5-mer holds whole
        modified = ((held >= 0) & state[np.maximum(held, 0)]).any(axis=0) if n_groups else np.zeros(bases, bool)
        level = np.where(modified, alt[kmer], table[kmer])
        dwell = rng.geometric(1.0 / mean_dwell, bases).astype(np.int64)
        true = np.concatenate([[0], np.cumsum(dwell)])
        x = np.clip(np.rint(np.repeat(level, dwell) + rng.normal(0.0, 25.6 * 3.0, int(true[-1]))), -32767, 32767).astype(np.int16)
        start = true.copy()
        start[1:-1] = np.sort(np.clip(true[1:-1] + rng.integers(-jitter, jitter + 1, bases - 1), 0, true[-1]))
        first = np.full(n_groups, len(codes), dtype=np.int64)
        last = np.full(n_groups, -1, dtype=np.int64)
        np.minimum.at(first, gid, occ - h)                                                  # the sites as bases: the C of a CG at p is base p - h
        np.maximum.at(last, gid, occ - h)
        w0, width = first - reach, last - first + 1 + 2 * reach
        ok = (width <= COLUMNS) & (w0 >= 0) & (w0 + width <= bases)
        w0, width, groups = w0[ok], width[ok], np.flatnonzero(ok)
        at = np.minimum(w0[:, None] + cols[None, :], bases - 1)                             # [segments, 16]; columns past the width are cut below
        own = (held[:, at] == groups[None, :, None]).any(axis=0)
        row0, row1 = table[kmer[at]], np.where(own, alt[kmer[at]], table[kmer[at]])
        real = cols[None, :] < width[:, None]
        both = np.stack([row0, row1], axis=1)                                               # [segments, 2, 16]: the two candidates are adjacent
        rows.append(both[np.broadcast_to(real[:, None, :], both.shape)])
        widths.append(np.repeat(width, 2))
        s0, s1 = start[w0], start[w0 + width]
        sig += [x[a:b] for a, b in zip(s0, s1)]
        lens.append(s1 - s0)
        truth.append(state[groups])
        per_read.append(len(groups))
    lens = np.concatenate(lens)
    widths = np.concatenate(widths)
    off = lambda n: np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    samples = np.ascontiguousarray(np.concatenate(sig + [np.zeros(1, np.int16)]))
    level = np.ascontiguousarray(np.concatenate(rows + [np.zeros(1, np.int32)]).astype(np.int32))
    seg = np.repeat(np.arange(len(lens), dtype=np.int32), 2)
    return samples, off(lens), level, off(widths), seg, np.concatenate(truth), np.asarray(per_read, dtype=np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2048)
    ap.add_argument("--bases", type=int, default=10000)
    ap.add_argument("--dwell", type=float, default=9.0)
    ap.add_argument("--jitter", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ref-reads", dest="ref_reads", type=int, default=16, help="reads whose candidates the numpy reference scores; its time is scaled by cells")
    ap.add_argument("--library-only", dest="library_only", action="store_true", help="only run the call --rounds times, write nothing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "modcall.json"))
    args = ap.parse_args()
    import torch
    from chiron_amd import _lib, modcall
    import site_ref as ref
    if not torch.cuda.is_available():
        sys.exit("bench_modcall: no GPU")
    rng = np.random.default_rng(20261021)
    samples, sample_off, level, level_off, seg, truth, per_read = make_call(rng, args.reads, args.bases, args.dwell, args.jitter)
    n_seg, n_cand, n_samples, n_levels = len(sample_off) - 1, len(seg), int(sample_off[-1]), int(level_off[-1])
    nbytes = modcall.score_workspace_size(n_seg, n_samples, n_cand, n_levels)
    lib, ws, stream = _lib.device_workspace(nbytes, 0, "bench_modcall", "site kernel")
    cost = np.zeros(n_cand, dtype=np.int32)

    def call():
        _lib.check(lib.chiron_signal_score(0, samples.ctypes.data, sample_off.ctypes.data, n_seg, level.ctypes.data, level_off.ctypes.data, seg.ctypes.data,
                                           n_cand, cost.ctypes.data, ws.data_ptr(), nbytes, 0, stream))

    if args.library_only:
        for _ in range(args.rounds):
            call()
        print("bench_modcall: %d calls of %d segments, %d candidates, %d samples" % (args.rounds, n_seg, n_cand, n_samples))
        return
    torch.set_num_threads(1)
    for _ in range(args.warmup):
        call()
    call_ms = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        call()
        call_ms.append((time.perf_counter() - t0) * 1e3)
    cells_of = lambda g, c: int(((sample_off[1:g + 1] - sample_off[:g])[seg[:c]] * (level_off[1:c + 1] - level_off[:c])).sum())
    sub_seg = int(per_read[:min(args.ref_reads, args.reads)].sum())
    sub = 2 * sub_seg                                                                       # the first reads' candidates: they name the first segments only
    t0 = time.perf_counter()
    want = ref.score_flat(samples, sample_off[:sub_seg + 1], level, level_off[:sub + 1], seg[:sub])
    numpy_sub_ms = (time.perf_counter() - t0) * 1e3
    if not np.array_equal(cost[:sub], want):
        sys.exit("bench_modcall: the library call and the numpy reference differ on the candidates of the first %d reads" % args.ref_reads)
    cells, sub_cells = cells_of(n_seg, n_cand), cells_of(sub_seg, sub)
    numpy_ms = numpy_sub_ms * cells / sub_cells
    ratio = numpy_ms / float(np.median(call_ms))
    ok = (cost[0::2] != modcall.INFEASIBLE) & (cost[1::2] != modcall.INFEASIBLE)
    delta = (cost[0::2].astype(np.int64) - cost[1::2])[ok] / np.maximum(sample_off[1:] - sample_off[:-1], 1)[ok]
    med = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    result = {"device": torch.cuda.get_device_name(0), "reads": args.reads, "bases_per_read": args.bases, "mean_dwell": args.dwell, "jitter": args.jitter,
              "segments": n_seg, "candidates": n_cand, "samples": n_samples, "levels": n_levels, "cells": cells, "workspace_bytes": int(nbytes),
              "rounds": args.rounds, "call_ms": med(call_ms), "numpy_reads": min(args.ref_reads, args.reads), "numpy_candidates": sub,
              "numpy_subset_ms": numpy_sub_ms, "numpy_ms_scaled": numpy_ms, "numpy_over_call": ratio,
              "call_ns_per_candidate": float(np.median(call_ms)) * 1e6 / n_cand, "infeasible_segments": int((~ok).sum()),
              "sign_names_the_planted_state": float(((delta > 0) == truth[ok]).mean()),
              "note": "call_ms is the whole library call on prepared arrays: the host's checking walk, copies in, the launch, the copy out; "
                      "numpy_ms_scaled is tests/site_ref.py's numpy rows on one core over numpy_candidates candidates, scaled to all by cells"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result))
    if not ratio > 1.0:
        sys.exit("bench_modcall: the library call is not faster than the numpy reference on one core")


if __name__ == "__main__":
    main()
