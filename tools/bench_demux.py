#!/usr/bin/env python
"""Time chiron_demux_windows (csrc/demux.hip) on the shape `demux` meets: 100,000 synthetic reads, which is 200,000 windows of 150
bases (a head and a reversed tail each, four fifths of them with a 24-base barcode mutated at 10 % behind 0 to 40 junk bases),
against 96 barcodes of 24 bases, and again against 12.  One chiron_demux_windows call per end is timed, arrays prepared beforehand:
the host checks and packing, the copies in, the launch, the copies out.  For context a sample of the same (pattern, window) pairs
goes through the existing chiron_align_infix, one workgroup a pair, timed the same way; its E values must equal this kernel's or the
tool exits non-zero.  The numpy column DP of tests/demux_ref.py runs a smaller sample on the CPU and must agree as well.  Rounds
alternate between the kernels and are reported by their medians; the result goes to profiles/demux.json.

The one performance condition of the kernel is checked here: per pair it must be faster than the infix kernel on the same pairs
(ratio > 1, both measured in this run), or the tool exits non-zero.  Needs a GPU: there is nothing to time without one."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

COMPLEMENT = np.array([3, 2, 1, 0, 4], dtype=np.uint8)


def make_windows(rng, reads, window, barcodes, tail):
    """uint8 [reads, window]: random bases; in four of five a barcode mutated at 10 % (substitutions only, so the block keeps its
    shape) behind 0 to 40 junk bases.  tail: the barcodes' complements, as a reversed tail window shows them."""
    wins = rng.integers(0, 4, (reads, window)).astype(np.uint8)
    pats = COMPLEMENT[barcodes] if tail else barcodes
    n = pats.shape[1]
    which = rng.integers(0, len(pats), reads)
    junk = rng.integers(0, 41, reads)
    for r in range(reads):
        if r % 5 != 4:
            p = pats[which[r]].copy()
            hit = rng.random(n) < 0.10
            p[hit] = (p[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
            wins[r, junk[r]:junk[r] + n] = p
    return wins


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--window", type=int, default=150)
    ap.add_argument("--barcode-len", dest="barcode_len", type=int, default=24)
    ap.add_argument("--infix-pairs", dest="infix_pairs", type=int, default=8192, help="pairs of the sample the infix kernel aligns per round")
    ap.add_argument("--cpu-windows", dest="cpu_windows", type=int, default=256, help="windows the numpy reference searches per round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "demux.json"))
    args = ap.parse_args()
    import torch
    from chiron_amd import _lib, demux, map as cmap
    import demux_ref as ref
    if not torch.cuda.is_available():
        sys.exit("bench_demux: no GPU")
    rng = np.random.default_rng(20261019)
    med = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    result = {"device": torch.cuda.get_device_name(0), "reads": args.reads, "window": args.window, "barcode_len": args.barcode_len,
              "rounds": args.rounds, "kits": {},
              "note": "demux_ms and infix_ms are whole library calls on prepared arrays: host checks and packing, copies in, the launch, "
                      "copies out; the numpy time is one core, vectorised over the sample's windows"}
    ok = True
    for kit in (96, 12):
        barcodes = rng.integers(0, 4, (kit, args.barcode_len)).astype(np.uint8)
        groups = np.arange(kit, dtype=np.int32)
        ends = []
        for tail in (False, True):
            wins = make_windows(rng, args.reads, args.window, barcodes, tail)
            pats = COMPLEMENT[barcodes] if tail else barcodes
            win_codes = np.ascontiguousarray(np.concatenate([wins.reshape(-1), np.zeros(1, np.uint8)]))
            win_off = (np.arange(args.reads + 1, dtype=np.int64) * args.window)
            pat_codes = np.ascontiguousarray(np.concatenate([pats.reshape(-1), np.zeros(1, np.uint8)]))
            pat_off = (np.arange(kit + 1, dtype=np.int64) * args.barcode_len)
            ends.append((wins, pats, win_codes, win_off, pat_codes, pat_off))
        nbytes = demux.workspace_size(args.reads, args.reads * args.window, kit, True)
        lib, ws, stream = _lib.device_workspace(nbytes, 0, "bench_demux", "barcode search")
        out = [np.zeros(args.reads, np.int32) for _ in range(4)]
        pair_dist = np.zeros((args.reads, kit), np.int16)
        pair_end = np.zeros((args.reads, kit), np.int16)

        def search(end, matrix):
            _, _, win_codes, win_off, pat_codes, pat_off = ends[end]
            _lib.check(lib.chiron_demux_windows(0, win_codes.ctypes.data, win_off.ctypes.data, args.reads, pat_codes.ctypes.data,
                                                pat_off.ctypes.data, groups.ctypes.data, kit, 0, out[0].ctypes.data, out[1].ctypes.data,
                                                out[2].ctypes.data, out[3].ctypes.data, pair_dist.ctypes.data if matrix else None,
                                                pair_end.ctypes.data if matrix else None, ws.data_ptr(), stream))

        # the sample of pairs the infix kernel aligns: head windows, every pattern in turn
        n_pairs = min(args.infix_pairs, args.reads)
        sample_w = rng.choice(args.reads, n_pairs, replace=False)
        sample_q = np.arange(n_pairs) % kit
        wins, pats = ends[0][0], ends[0][1]
        codes, lens_a, lens_b, read_off, infix_off = _lib.pack_pairs([pats[q] for q in sample_q], [wins[w] for w in sample_w])
        infix_ws = torch.empty(max(cmap.workspace_size(n_pairs, args.barcode_len, args.window), 256), dtype=torch.uint8, device="cuda:0")
        infix_out = [np.zeros(n_pairs, np.int32) for _ in range(5)]

        def infix():
            _lib.check(lib.chiron_align_infix(0, codes.ctypes.data, read_off.ctypes.data, infix_off.ctypes.data, n_pairs, cmap.BAND0, 0,
                                              *[a.ctypes.data for a in infix_out], infix_ws.data_ptr(), stream))

        cpu_w = sample_w[:args.cpu_windows]

        def cpu():
            return ref.matrix([wins[w] for w in cpu_w], list(pats))

        def timed(fn, *a):
            t0 = time.perf_counter()
            got = fn(*a)
            return (time.perf_counter() - t0) * 1e3, got

        for _ in range(args.warmup):
            search(0, False)
            search(1, False)
            infix()
        head_ms, tail_ms, infix_ms, cpu_ms = [], [], [], []
        for _ in range(args.rounds):          # alternating: every kernel sees the same machine state
            head_ms.append(timed(search, 0, False)[0])
            tail_ms.append(timed(search, 1, False)[0])
            infix_ms.append(timed(infix)[0])
        t, (want_E, want_e) = timed(cpu)
        cpu_ms.append(t)
        matrix_ms, _ = timed(search, 0, True)              # the head windows once more, with the matrix, for the comparisons
        if not np.array_equal(pair_dist[sample_w, sample_q], infix_out[0]):
            bad = np.flatnonzero(pair_dist[sample_w, sample_q] != infix_out[0])
            sys.exit("bench_demux: %d of %d sampled pairs differ from chiron_align_infix in E (first: window %d pattern %d, %d against %d)"
                     % (len(bad), n_pairs, sample_w[bad[0]], sample_q[bad[0]], pair_dist[sample_w[bad[0]], sample_q[bad[0]]], infix_out[0][bad[0]]))
        if not (np.array_equal(pair_dist[cpu_w], want_E) and np.array_equal(pair_end[cpu_w], want_e)):
            sys.exit("bench_demux: the kernel and the numpy reference differ on the sampled windows")
        pairs = args.reads * kit
        demux_ns = float(np.median(head_ms + tail_ms)) * 1e6 / pairs
        infix_ns = float(np.median(infix_ms)) * 1e6 / n_pairs
        result["kits"][str(kit)] = {
            "barcodes": kit, "windows": 2 * args.reads, "pairs_per_end": pairs, "workspace_bytes": int(nbytes),
            "head_call_ms": med(head_ms), "tail_call_ms": med(tail_ms), "head_call_with_matrix_ms": matrix_ms,
            "demux_ns_per_pair": demux_ns,
            "infix_pairs": n_pairs, "infix_call_ms": med(infix_ms), "infix_ns_per_pair": infix_ns,
            "infix_over_demux_per_pair": infix_ns / demux_ns,
            "numpy_windows": len(cpu_w), "numpy_ns_per_pair": float(np.median(cpu_ms)) * 1e6 / (len(cpu_w) * kit),
            "hits_at_defaults": int(demux.hits({"best": out[0], "dist": out[1], "second": out[3]}, [args.barcode_len] * kit).sum())}
        ok = ok and infix_ns / demux_ns > 1.0
        del ws, infix_ws
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result))
    if not ok:
        sys.exit("bench_demux: the bit-vector kernel is not faster per pair than chiron_align_infix on the same pairs")


if __name__ == "__main__":
    main()
