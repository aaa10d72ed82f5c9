#!/usr/bin/env python3
"""Time what `map --candidates 4` costs over `map` on tools/bench_map.py's workload and write one JSON record:

  2048 reads of 10 000 bases cut from a 5 Mb random, repeat-free genome (two contigs) and mutated at 12 %, every other one
  reverse-complemented (the same seed and construction as bench_map.py).

Two comparisons, each timed with the host clock in alternating rounds after a warm-up of both sides, in one run:
  seeding   map.vote_reads_top at max_cand 4, min_score map.MIN_VOTES (chiron_seed_candidates) against map.vote_reads
            (chiron_seed_reads) on the same reads and index: the index conversion, packing, copies, the launch, synchronise, the
            Python dicts.
  map       the whole map.map_reads (seeding, windows, chiron_align_infix, records) at candidates 4 against candidates 1, the
            index built once outside.
The tool exits unless pick 0 of every read equals the single-candidate result, and unless the primary placement at candidates 4
is the one at candidates 1 (the genome has no repeats).  Medians are reported with the spread, and the two ratios.

    python tools/bench_map_candidates.py [--reads 2048] [--length 10000] [--genome 5000000] [--rounds 3] [--out profiles/map_candidates.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

MAX_CAND = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2048)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--genome", type=int, default=5000000)
    ap.add_argument("--rate", type=float, default=0.12)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_candidates.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_map_candidates.py measures the GPU kernels: no GPU, no number")
    from chiron_amd import assess, map as cmap
    from bench_assess import mutate_codes

    rng = np.random.default_rng(20241)
    codes = rng.integers(0, 4, args.genome).astype(np.uint8)
    cut = args.genome * 2 // 5
    genome = cmap.Genome([("ctgA", codes[:cut]), ("ctgB", codes[cut:])])
    reads = []
    for k in range(args.reads):
        c = k % 2
        start = int(rng.integers(0, int(genome.lengths[c]) - args.length))
        piece = mutate_codes(genome.codes[int(genome.starts[c]) + start:int(genome.starts[c]) + start + args.length], args.rate, rng)
        reads.append(assess.reverse_complement(piece) if k % 4 < 2 else piece)
    index = cmap.build_index(genome.codes)
    named = {"read%05d" % k: r for k, r in enumerate(reads)}
    seeder, top_seeder = cmap.seeder_of("gpu"), cmap.top_seeder_of("gpu")

    def seed_one():
        return cmap.vote_reads(index, reads)

    def seed_top():
        return cmap.vote_reads_top(index, reads, MAX_CAND, cmap.MIN_VOTES)

    def map_one():
        return cmap.map_reads(named, genome, index=index, seeder=seeder)

    def map_top():
        return cmap.map_reads(named, genome, index=index, seeder=seeder, top_seeder=top_seeder, candidates=MAX_CAND)

    votes, picks = seed_one(), seed_top()                                    # warm-up: code object load, allocator; and the check
    for v, p in zip(votes, picks):
        want = [{key: v[key] for key in ("votes", "strand", "delta", "g")}] if v["votes"] >= cmap.MIN_VOTES else []
        if p[:1] != want:
            sys.exit("bench_map_candidates.py: pick 0 differs from the single-candidate result")
    one, top = map_one(), map_top()
    place = ("contig", "strand", "start", "end", "edit", "match", "status")
    if [[r[key] for key in place] for r in one["reads"]] != [[r[key] for key in place] for r in top["reads"]]:
        sys.exit("bench_map_candidates.py: a read's placement changed with the candidates on a repeat-free genome")
    times = {"seed_one": [], "seed_top": [], "map_one": [], "map_top": []}
    for _ in range(args.rounds):
        for name, fn in (("seed_one", seed_one), ("seed_top", seed_top), ("map_one", map_one), ("map_top", map_top)):
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    med = {name: float(np.median(t)) for name, t in times.items()}
    aligned = sum(r["candidates"] for r in top["reads"])
    record = {
        "workload": {"reads": args.reads, "length": args.length, "genome": args.genome, "contigs": 2, "mutation_rate": args.rate, "seed": 20241,
                     "k": cmap.K, "max_occ": cmap.MAX_OCC, "max_cand": MAX_CAND, "min_score": cmap.MIN_VOTES, "second_ratio": 0.5},
        "timing": "host clock; %d rounds of seed 1, seed %d, map 1, map %d in turn after a warm-up of each" % (args.rounds, MAX_CAND, MAX_CAND),
        "device": torch.cuda.get_device_name(0),
        "seconds": {name: {"median": med[name], "min": float(min(t)), "max": float(max(t))} for name, t in times.items()},
        "seed_candidates_over_seed_reads": med["seed_top"] / med["seed_one"],
        "map_candidates_over_map": med["map_top"] / med["map_one"],
        "picks_per_read_mean": float(np.mean([len(p) for p in picks])),
        "candidates_aligned": aligned, "reads_mapped": top["totals"]["mapped"], "ambiguity": top["ambiguity"],
    }
    print(json.dumps(record))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
