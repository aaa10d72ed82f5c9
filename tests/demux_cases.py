"""Shared inputs of the demux tests: the planted multiplexed run, and the edge-case windows and patterns of the GPU tests."""
import numpy as np

import assess_ref
import map_ref

SEED = 3
KINDS = ("both", "head", "tail", "none", "two")


def planted(seed=SEED, barcodes=12, reads=300, rate=0.10):
    """A multiplexed run: `barcodes` random 24-base barcodes bc01..; `reads` reads of 200 to 400 random insert bases with qualities.
    A planted barcode is mutated at `rate` (assess_ref.mutate) and sits behind 0 to 40 junk bases: junk + barcode + insert at the
    head, insert + reverse complement of the barcode + junk at the tail.  Read r is of kind KINDS[r % 5]: the same barcode at both
    ends, at the head only, at the tail only, none, or two different barcodes.
    -> dict(barcodes=[(name, seq)], reads=[(name, seq, qual)], truth={name: (kind, head barcode or None, tail barcode or None)})."""
    rng = np.random.default_rng(seed)
    codes = [("bc%02d" % (k + 1), assess_ref.random_seq(24, rng)) for k in range(barcodes)]
    out, truth = [], {}
    for r in range(reads):
        kind = KINDS[r % len(KINDS)]
        insert = assess_ref.random_seq(int(rng.integers(200, 401)), rng)
        first = int(rng.integers(0, barcodes))
        other = (first + 1 + int(rng.integers(0, barcodes - 1))) % barcodes
        head = first if kind in ("both", "head", "two") else None
        tail = first if kind in ("both", "tail") else other if kind == "two" else None
        seq = insert
        if head is not None:
            seq = assess_ref.random_seq(int(rng.integers(0, 41)), rng) + assess_ref.mutate(codes[head][1], rate, rng) + seq
        if tail is not None:
            seq = seq + map_ref.revcomp(assess_ref.mutate(codes[tail][1], rate, rng)) + assess_ref.random_seq(int(rng.integers(0, 41)), rng)
        qual = "".join(chr(33 + int(v)) for v in rng.integers(2, 40, len(seq)))
        name = "read%03d" % r
        out.append((name, seq, qual))
        truth[name] = (kind, None if head is None else codes[head][0], None if tail is None else codes[tail][0])
    return {"barcodes": codes, "reads": out, "truth": truth}


def write_planted(case, folder):
    """reads.fastq and barcodes.fasta of a planted case under folder -> their paths."""
    reads, barcodes = "%s/reads.fastq" % folder, "%s/barcodes.fasta" % folder
    with open(reads, "w") as f:
        f.write("".join("@%s\n%s\n+\n%s\n" % rec for rec in case["reads"]))
    with open(barcodes, "w") as f:
        f.write("".join(">%s\n%s\n" % rec for rec in case["barcodes"]))
    return reads, barcodes


def random_codes(n, rng, with_n=False):
    return rng.integers(0, 5 if with_n else 4, n).astype(np.uint8)


def edge_case(seed=11):
    """(windows, patterns, groups) of the edge-case launch: patterns of 1, 2, 31, 32, 33, 63, 64 bases (one of each also with code 4
    in it) and windows of 0, 1, 2, 63, 64, 65, 150, 4096 bases, random, with code 4, and with an exact copy of each pattern planted at
    the window's start (e = n) and at its end (e = m); a 64-base pattern against its own copy and against its copy with one base
    deleted."""
    rng = np.random.default_rng(seed)
    patterns = [random_codes(n, rng) for n in (1, 2, 31, 32, 33, 63, 64)]
    patterns += [random_codes(n, rng, with_n=True) for n in (2, 33, 64)]
    full = patterns[6]
    windows = []
    for m in (0, 1, 2, 63, 64, 65, 150, 4096):
        windows.append(random_codes(m, rng))
        windows.append(random_codes(m, rng, with_n=True))
        for p in patterns[:7]:
            if len(p) <= m:
                at_start, at_end = random_codes(m, rng), random_codes(m, rng)
                at_start[:len(p)] = p
                at_end[m - len(p):] = p
                windows += [at_start, at_end]
    windows.append(full.copy())
    windows.append(np.delete(full, 20))
    windows.append(np.concatenate([random_codes(7, rng), np.delete(full, 63), random_codes(9, rng)]))
    groups = np.array([0, 1, 2, 3, 4, 5, 6, 1, 4, 6], dtype=np.int32)
    return windows, patterns, groups
