#!/usr/bin/env python3
"""Time the overlap alignment (chiron_amd/overlap.py, chiron_align_overlap in csrc/overlap.hip) on a fixed, seeded workload and
write one JSON record:

  2048 reads of 10 000 bases cut from a 1 Mb random genome (about 20-fold coverage) and mutated at 12 % (substitutions,
  insertions and deletions, a third each), every other one reverse-complemented.

The index and the candidates (overlap.candidates, host numpy) are computed once and timed with the host clock; they are reported
and take no part in the ratio.  The candidate pairs at band 256 are planned into calls once (overlap.plan_batches).  After one
warm-up of that sequence of calls, --rounds rounds alternate (a) the whole sequence -- packing, copies, the launches, the
synchronise inside each call -- and (b) the numpy reference of tests/overlap_ref.py on the first --baseline-pairs pairs, one
thread, same host.  The reference's figure for the workload is its time scaled by band cells (the cells of the diagonals inside
each pair's band), an EXTRAPOLATION, and is labelled so.  The subset's (cost, M, s, e) must equal the library's.  The one
performance condition is extrapolated reference seconds over library seconds above 1; without it the tool exits non-zero.

    python tools/bench_overlap.py [--reads 2048] [--length 10000] [--genome 1000000] [--rounds 3] [--baseline-pairs 4] [--out profiles/overlap.json]
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


def band_cells(n, m, dlo, dhi):
    """Cells of the (n+1) x (m+1) table on the diagonals dlo .. dhi (already clipped)."""
    d = np.arange(dlo, dhi + 1)
    return int((np.minimum(n, m - d) - np.maximum(0, -d) + 1).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2048)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--genome", type=int, default=1000000)
    ap.add_argument("--rate", type=float, default=0.12)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--baseline-pairs", type=int, default=4)
    ap.add_argument("--workspace-mb", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlap.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_overlap.py measures the GPU kernel: no GPU, no number")
    from chiron_amd import assess, overlap
    from bench_assess import mutate_codes
    import overlap_ref

    rng = np.random.default_rng(20251)
    genome = rng.integers(0, 4, args.genome).astype(np.uint8)
    reads, spans = [], []
    for k in range(args.reads):
        start = int(rng.integers(0, args.genome - args.length))
        piece = mutate_codes(genome[start:start + args.length], args.rate, rng)
        reads.append(assess.reverse_complement(piece) if k % 2 else piece)
        spans.append((start, start + args.length))

    t0 = time.perf_counter()
    index = overlap.build_index(reads)
    t_index = time.perf_counter() - t0
    t0 = time.perf_counter()
    cands = overlap.candidates(index, reads)
    t_cand = time.perf_counter() - t0
    true_pairs = sum(1 for c in cands if min(spans[c["a"]][1], spans[c["b"]][1]) - max(spans[c["a"]][0], spans[c["b"]][0]) >= overlap.MIN_OVERLAP)

    R = len(reads)
    seqs = reads + [assess.reverse_complement(r) for r in reads]
    lens = np.array([len(r) for r in seqs], dtype=np.int64)
    pairs = overlap.band_pairs(lens, R, cands, [overlap.BAND] * len(cands))
    runs = overlap.plan_batches(lens, pairs, args.workspace_mb << 20)

    def sequence():
        out = np.zeros(len(pairs), dtype=overlap.OVERLAP_DTYPE)
        for first, last in runs:
            out[first:last] = overlap.align_overlap(seqs, pairs[first:last])
        return out

    first = sequence()                                           # warm-up: code object load, allocator
    sub = pairs[:min(args.baseline_pairs, len(pairs))]
    t_gpu, t_ref = [], []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        got = sequence()                                         # every call ends in a stream synchronise
        t_gpu.append(time.perf_counter() - t0)
        if got.tobytes() != first.tobytes():
            sys.exit("bench_overlap.py: the results changed between runs")
        t0 = time.perf_counter()
        want = overlap_ref.rows(seqs, sub)
        t_ref.append(time.perf_counter() - t0)
        if want.tobytes() != first[:len(sub)].tobytes():
            sys.exit("bench_overlap.py: the first pairs differ from the reference")

    cells = [band_cells(int(lens[a]), int(lens[b]), dlo, dhi) for a, b, dlo, dhi in pairs.tolist()]
    steps = [int(lens[a] + lens[b] + 1) for a, b, _, _ in pairs.tolist()]
    t, tr = float(np.median(t_gpu)), float(np.median(t_ref))
    scaled = tr * sum(cells) / max(sum(cells[:len(sub)]), 1)
    kinds = {}
    for (a, b, dlo, dhi), r in zip(pairs.tolist(), first):
        n, m = int(lens[a]), int(lens[b])
        key = "band_edge" if overlap.touches_edge(n, m, dlo, dhi, int(r["start"]), int(r["end"])) else overlap.classify(n, m, int(r["start"]), int(r["end"]))[0]
        kinds[key] = kinds.get(key, 0) + 1
    record = {
        "workload": {"reads": args.reads, "length": args.length, "genome": args.genome, "mutation_rate": args.rate, "seed": 20251, "k": overlap.K,
                     "max_occ": overlap.MAX_OCC, "min_votes": overlap.MIN_VOTES, "max_overlaps": overlap.MAX_OVERLAPS, "band": overlap.BAND},
        "timing": "host clock; index and candidates once; the planned calls %d rounds alternating with the numpy reference after a warm-up; "
                  "every call ends in a stream synchronise" % args.rounds,
        "device": torch.cuda.get_device_name(0),
        "index_seconds": t_index, "candidates_seconds": t_cand, "candidates_seconds_per_read": t_cand / max(R, 1),
        "candidate_pairs": len(cands), "candidate_pairs_sharing_500_genome_bases": true_pairs,
        "align": {"pairs": len(pairs), "calls": len(runs), "seconds_median": t, "seconds_min": float(min(t_gpu)), "seconds_max": float(max(t_gpu)),
                  "pairs_per_second": len(pairs) / t, "band_cell_updates_per_second": sum(cells) / t,
                  "barrier_steps_per_pair_mean": float(np.mean(steps)) if steps else 0.0, "first_pass_results": kinds},
        "baseline": {"what": "tests/overlap_ref.py rows (numpy, one thread), same host", "pairs_timed": len(sub), "seconds_median": tr,
                     "seconds_for_the_workload": scaled, "extrapolated": True, "scaled_by": "band cells"},
        "ratio_reference_over_library": scaled / t,
    }
    print(json.dumps(record))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    if not scaled / t > 1:
        sys.exit("bench_overlap.py: the library is not faster than the numpy reference (ratio %.3f)" % (scaled / t))


if __name__ == "__main__":
    main()
