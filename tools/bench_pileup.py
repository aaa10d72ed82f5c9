#!/usr/bin/env python3
"""Time the pileup (chiron_pileup, csrc/pileup.hip) on the workload of tools/bench_map.py: 2048 seeded reads of 10 000 bases at 12 %
against a 5 Mb genome, the genome one tile.  The generator that mutates a read writes its op array directly, so no alignment runs.

  gpu      one chiron_pileup call on packed host arrays with a workspace allocated beforehand: the copies in, the clear of the
           count planes, pileup_count_kernel, pileup_call_kernel, the copies out (the 27 count planes included), the synchronise
  gpu_call_only   the same call with counts_out = NULL: depth and call records come back, the planes stay on the device
  numpy    the same counts from q, i and k computed with cumulative sums over all columns at once and np.add.at into the planes

Each timing is the host clock around the call.  After one warm-up of each, the three alternate for --rounds rounds in one
process; the medians, their spread, the number of counts added and the add rate are written as one JSON record.  The two count
arrays are asserted equal.  The numpy time is context, not a bar.

    python tools/bench_pileup.py [--reads 2048] [--length 10000] [--genome 5000000] [--rounds 5] [--out profiles/pileup.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def mutated_alignment(ref, rate, rng):
    """A read that is `ref` with substitutions, deletions and insertions at a third of `rate` each per base, and the op array that
    says so.  -> (read codes, ops)."""
    m = len(ref)
    u = rng.random(m)
    dele, sub, ins = u < rate / 3, (u >= rate / 3) & (u < 2 * rate / 3), (u >= 2 * rate / 3) & (u < rate)
    per = 1 + ins.astype(np.int64)
    first = np.cumsum(per) - per
    ops = np.zeros(int(per.sum()), dtype=np.uint8)
    ops[first] = np.where(dele, 3, np.where(sub, 1, 0))
    ops[first[ins] + 1] = 2
    base = np.zeros(len(ops), dtype=np.uint8)
    base[first] = np.where(sub, (ref + 1 + rng.integers(0, 3, m)) & 3, ref)
    base[first[ins] + 1] = rng.integers(0, 4, int(ins.sum()))
    return base[ops != 3], ops


def numpy_counts(ops, ops_off, codes, read_off, pos, tile, planes, slots):
    """The count planes of the tile [0, tile) from all columns at once."""
    n = len(pos)
    lens = np.diff(ops_off)
    aln = np.repeat(np.arange(n), lens)
    col = np.arange(len(ops), dtype=np.int64)
    on_ref, on_read = ops != 2, ops != 3
    cq = np.cumsum(on_ref) - on_ref
    ci = np.cumsum(on_read) - on_read
    q = cq - cq[ops_off[:-1]][aln]
    i = ci - ci[ops_off[:-1]][aln] + read_off[:-1][aln]
    m = np.add.reduceat(on_ref.astype(np.int64), ops_off[:-1])[aln] if len(ops) else np.zeros(0, np.int64)
    last = np.maximum.accumulate(np.where(on_ref, col, -1))
    k = col - last - 1
    g = pos[aln] + q
    code = codes[np.minimum(i, len(codes) - 1)].astype(np.int64)
    is_ins = ops == 2
    live_ins = is_ins & (q != 0) & (q != m)
    plane = np.where(ops < 2, code, np.where(ops == 3, 5, np.where(k < slots, 6 + 5 * np.minimum(k, slots - 1) + code, planes - 1)))
    g = np.where(is_ins, g - 1, g)
    keep = (g >= 0) & (g < tile) & (~is_ins | (live_ins & (k <= slots)))
    out = np.zeros(planes * tile, dtype=np.int32)
    np.add.at(out, plane[keep] * tile + g[keep], 1)
    return out.reshape(planes, tile)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2048)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--genome", type=int, default=5000000)
    ap.add_argument("--rate", type=float, default=0.12)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-depth", dest="min_depth", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pileup.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_pileup.py measures the GPU kernel: no GPU, no number")
    from chiron_amd import _lib, pileup

    rng = np.random.default_rng(20260)
    genome = rng.integers(0, 4, args.genome).astype(np.uint8)
    alns = []
    for _ in range(args.reads):
        start = int(rng.integers(0, args.genome - args.length))
        read, ops = mutated_alignment(genome[start:start + args.length], args.rate, rng)
        alns.append((start, read, ops))
    codes, read_off, ops, ops_off, pos = pileup.pack(alns)
    tile = args.genome
    nbytes = pileup.workspace_size(len(alns), int(read_off[-1]), int(ops_off[-1]), tile)
    lib = _lib.load()
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    counts = np.zeros((pileup.PLANES, tile), dtype=np.int32)
    depth = np.zeros(tile, dtype=np.int32)
    call = np.zeros((tile, 8), dtype=np.uint8)
    clipped = C.c_int64()

    def gpu(with_counts):
        t0 = time.perf_counter()
        _lib.check(lib.chiron_pileup(0, codes.ctypes.data, read_off.ctypes.data, ops.ctypes.data, ops_off.ctypes.data, pos.ctypes.data, len(alns),
                                     0, tile, genome.ctypes.data, args.min_depth, 0, counts.ctypes.data if with_counts else None,
                                     depth.ctypes.data, call.ctypes.data, C.byref(clipped), ws.data_ptr(), stream))
        return time.perf_counter() - t0

    def host():
        t0 = time.perf_counter()
        out = numpy_counts(ops[:-1], ops_off, codes, read_off, pos, tile, pileup.PLANES, pileup.INS_SLOTS)
        return time.perf_counter() - t0, out

    gpu(True)                                              # warm-up: code object load
    first = counts.copy()
    _, want = host()
    if not np.array_equal(first, want):
        sys.exit("bench_pileup.py: the GPU counts differ from the numpy counts at %s" % (np.argwhere(first != want)[:5].tolist(),))
    times = {"gpu": [], "gpu_call_only": [], "numpy": []}
    for _ in range(args.rounds):
        times["gpu"].append(gpu(True))
        if not np.array_equal(counts, first):
            sys.exit("bench_pileup.py: the counts changed between runs")
        times["gpu_call_only"].append(gpu(False))
        t, again = host()
        times["numpy"].append(t)
        if not np.array_equal(again, want):
            sys.exit("bench_pileup.py: the numpy counts changed between runs")
    added = int(first.astype(np.int64).sum())
    stat = lambda v: {"seconds_median": float(np.median(v)), "seconds_min": float(min(v)), "seconds_max": float(max(v))}   # noqa: E731
    record = {"workload": {"reads": args.reads, "length": args.length, "genome": args.genome, "mutation_rate": args.rate, "seed": 20260,
                           "min_depth": args.min_depth, "tiles": 1},
              "timing": "host clock around one chiron_pileup call (copies in, clear, both kernels, copies out, synchronise) and around the "
                        "numpy formulation; %d rounds, alternating, after one warm-up each" % args.rounds,
              "device": torch.cuda.get_device_name(0),
              "gpu": stat(times["gpu"]), "gpu_call_only": stat(times["gpu_call_only"]), "numpy": stat(times["numpy"]),
              "numpy_over_gpu": float(np.median(times["numpy"]) / np.median(times["gpu"])),
              "columns": int(ops_off[-1]), "counts_added": added, "clipped": int(clipped.value),
              "counts_per_second_whole_call": added / float(np.median(times["gpu"])),
              "counts_per_second_call_without_planes_copy": added / float(np.median(times["gpu_call_only"])),
              "workspace_bytes": nbytes, "count_plane_bytes": int(first.nbytes), "mean_depth": float(depth.mean()),
              "counts_equal_numpy": True}
    print(json.dumps(record))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
