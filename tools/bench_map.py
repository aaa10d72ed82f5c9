#!/usr/bin/env python3
"""Time the read mapper (chiron_amd/map.py, chiron_align_infix in csrc/map.hip) on a fixed, seeded workload and write one JSON
record:

  2048 reads of 10 000 bases cut from a 5 Mb random genome (two contigs) and mutated at 12 % (substitutions, insertions and
  deletions, a third each), every other one reverse-complemented.

Indexing (once), seeding (the votes of every read, host numpy) and alignment (map.align_in_batches on the windows the seeding
chose: coding, packing, copies, the launches, synchronise) are timed separately with the host clock.  The GPU seeding
(map.vote_reads, chiron_seed_reads in csrc/seed.hip: the index conversion, packing, copies, the launch, synchronise, the Python
dicts) is timed on the same reads and index in the same alternating rounds, after a warm-up of its own; its votes must equal the
host's, and both times and their ratio are recorded.  After one warm-up of the
alignment, the infix alignment and -- for context -- chiron_align_pairs on same-sized global pairs (each read against its window)
alternate for --rounds rounds; medians are reported with the spread.  Band cells count every band a pair tried.  The numpy
reference of tests/map_ref.py is timed on --baseline-pairs reads; its workload figure is the per-read mean times the number of
reads, an EXTRAPOLATION, and is labelled so.  The subset's (E, M, s, e) must equal the kernel's.

    python tools/bench_map.py [--reads 2048] [--length 10000] [--genome 5000000] [--rounds 3] [--baseline-pairs 2] [--out profiles/map.json]
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


def band_cells(n, m, E, band0):
    """Cells the kernel updated for a pair that ends with cost E: every band it tried, first to accepted; -> (cells, w, bands tried)."""
    d_all = np.arange(-n, m + 1)
    diag_len = np.minimum(n, m - d_all) - np.maximum(0, -d_all) + 1
    total, w, tried = 0, band0, 0
    while True:
        dlo, dhi = max(min(0, m - n) - w, -n), min(max(0, m - n) + w, m)
        total += int(diag_len[dlo + n:dhi + n + 1].sum())
        tried += 1
        if (dlo == -n and dhi == m) or E <= w:
            return total, w, tried
        w *= 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2048)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--genome", type=int, default=5000000)
    ap.add_argument("--rate", type=float, default=0.12)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--baseline-pairs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_map.py measures the GPU kernel: no GPU, no number")
    from chiron_amd import assess, map as cmap
    from bench_assess import mutate_codes
    import map_ref

    rng = np.random.default_rng(20241)
    codes = rng.integers(0, 4, args.genome).astype(np.uint8)
    cut = args.genome * 2 // 5
    genome = cmap.Genome([("ctgA", codes[:cut]), ("ctgB", codes[cut:])])
    reads, truth = [], []
    for k in range(args.reads):
        c = k % 2
        start = int(rng.integers(0, int(genome.lengths[c]) - args.length))
        piece = mutate_codes(genome.codes[int(genome.starts[c]) + start:int(genome.starts[c]) + start + args.length], args.rate, rng)
        reads.append(assess.reverse_complement(piece) if k % 4 < 2 else piece)
        truth.append((c, start, "reverse" if k % 4 < 2 else "forward"))

    t0 = time.perf_counter()
    index = cmap.build_index(genome.codes)
    t_index = time.perf_counter() - t0
    t0 = time.perf_counter()
    votes = [cmap.vote(index, r) for r in reads]
    t_seed = time.perf_counter() - t0
    a, wins, placed = [], [], 0
    for r, v, (c, start, strand) in zip(reads, votes, truth):
        if v["votes"] < cmap.MIN_VOTES:
            continue
        contig = genome.contig_of(v["g"])
        placed += int(contig == c and v["strand"] == strand and abs(v["delta"] - int(genome.starts[c]) - start) < args.length // 8)
        n = len(r)
        lo, hi = cmap.window_of(genome, contig, v["delta"], n, max(cmap.BIN, n // 8))
        a.append(r if v["strand"] == "forward" else assess.reverse_complement(r))
        wins.append(genome.codes[lo:hi])

    first = cmap.align_in_batches(a, wins)                       # warm-up: code object load, allocator
    glob = assess.align_pairs(a, wins)
    if cmap.vote_reads(index, reads) != votes:                   # warm-up of the seeding kernel, and its check
        sys.exit("bench_map.py: the GPU votes differ from the host votes")
    t_infix, t_glob, t_gpu_seed = [], [], []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        gpu_votes = cmap.vote_reads(index, reads)
        t_gpu_seed.append(time.perf_counter() - t0)
        if gpu_votes != votes:
            sys.exit("bench_map.py: the GPU votes differ from the host votes")
        t0 = time.perf_counter()
        got = cmap.align_in_batches(a, wins)
        t_infix.append(time.perf_counter() - t0)
        if got.tobytes() != first.tobytes():
            sys.exit("bench_map.py: the infix alignment changed between runs")
        t0 = time.perf_counter()
        assess.align_pairs(a, wins)
        t_glob.append(time.perf_counter() - t0)

    cells = [band_cells(len(r), len(w), int(e), cmap.BAND0) for r, w, e in zip(a, wins, first["edit"])]
    if [c[1] for c in cells] != first["band"].tolist():
        sys.exit("bench_map.py: the kernel's bands are not the ones the rule gives")
    touches = int(np.sum((first["start"] == 0) | (first["end"] == np.array([len(w) for w in wins]))))
    base_s = []
    for k in range(min(args.baseline_pairs, len(a))):
        t0 = time.perf_counter()
        want = map_ref.full_table(map_ref.as_str(a[k]), map_ref.as_str(wins[k]))
        base_s.append(time.perf_counter() - t0)
        if want != tuple(int(first[f][k]) for f in ("edit", "match", "start", "end")):
            sys.exit("bench_map.py: pair %d differs from the reference DP" % k)
    t = float(np.median(t_infix))
    t_gs = float(np.median(t_gpu_seed))
    bands, band_counts = np.unique(first["band"], return_counts=True)
    tried, tried_counts = np.unique([c[2] for c in cells], return_counts=True)
    steps = sum((len(r) + len(w) + 1) * c[2] for r, w, c in zip(a, wins, cells))
    record = {
        "workload": {"reads": args.reads, "length": args.length, "genome": args.genome, "contigs": 2, "mutation_rate": args.rate,
                     "seed": 20241, "k": cmap.K, "max_occ": cmap.MAX_OCC, "band0": cmap.BAND0},
        "timing": "host clock; index once, host votes once, GPU votes and alignment %d rounds alternating with chiron_align_pairs after a warm-up" % args.rounds,
        "device": torch.cuda.get_device_name(0),
        "index_seconds": t_index, "seeding_seconds": t_seed, "seeding_seconds_per_read": t_seed / max(len(reads), 1),
        "seeding_gpu": {"what": "map.vote_reads on the same reads and index, equal to the host votes", "seconds_median": t_gs,
                        "seconds_min": float(min(t_gpu_seed)), "seconds_max": float(max(t_gpu_seed)), "seconds_per_read": t_gs / max(len(reads), 1),
                        "host_over_gpu": t_seed / t_gs},
        "reads_seeded": len(a), "reads_seeded_at_their_planted_place": placed,
        "align": {"pairs": len(a), "seconds_median": t, "seconds_min": float(min(t_infix)), "seconds_max": float(max(t_infix)),
                  "pairs_per_second": len(a) / t, "band_cell_updates_per_second": sum(c[0] for c in cells) / t,
                  "barrier_steps_per_pair_mean": steps / max(len(a), 1),
                  "accepted_band_distribution": {str(int(b)): int(c) for b, c in zip(bands, band_counts)},
                  "bands_tried_distribution": {str(int(b)): int(c) for b, c in zip(tried, tried_counts)},
                  "pairs_touching_a_window_edge": touches,
                  "edit_over_read_len_mean": float(np.mean(first["edit"] / np.maximum([len(r) for r in a], 1)))},
        "host_share_of_map_time": (t_seed) / (t_seed + t),
        "host_share_with_indexing": (t_index + t_seed) / (t_index + t_seed + t),
        "seeding_share_of_map_time_with_gpu_seeding": t_gs / (t_gs + t),
        "context_global_align_pairs": {"what": "chiron_align_pairs on the same pairs (read against its whole window, global)",
                                       "seconds_median": float(np.median(t_glob)), "pairs_per_second": len(a) / float(np.median(t_glob)),
                                       "accepted_band_distribution": {str(int(b)): int(c) for b, c in zip(*np.unique(glob["band"], return_counts=True))}},
        "baseline": {"what": "tests/map_ref.py full_table (numpy, one thread), same host", "pairs_timed": len(base_s),
                     "seconds_per_pair_mean": float(np.mean(base_s)) if base_s else None,
                     "seconds_for_the_workload": float(np.mean(base_s)) * len(a) if base_s else None, "extrapolated": True},
    }
    print(json.dumps(record))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
