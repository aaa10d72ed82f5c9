"""Inputs shared by tests/test_pileup_cpu.py and tests/test_gpu_pileup.py: random alignment sets and the end-to-end case."""
import numpy as np

import assess_ref
import map_ref
import pileup_ref
import trace_ref


def random_alignment(rng, columns, pos, p_ins=0.15, p_del=0.15, letters=4, n_rate=0.0):
    """(pos, read, ops): `columns` columns drawn with the given 'I' and 'D' rates, 'X' for a tenth of the diagonal ones; the read
    from `letters` codes, with code 4 at n_rate."""
    u = rng.random(columns)
    ops = np.where(u < p_ins, 2, np.where(u < p_ins + p_del, 3, np.where(u < p_ins + p_del + 0.08, 1, 0))).astype(np.uint8)
    n = int((ops != 3).sum())
    read = rng.integers(0, letters, n).astype(np.uint8)
    read[rng.random(n) < n_rate] = 4
    return int(pos), read, ops


def random_set(rng, count, tile, max_columns=60, **kw):
    """`count` alignments around [0, tile): some start before 0, some end past it."""
    out = []
    for _ in range(count):
        columns = int(rng.integers(0, max_columns + 1))
        out.append(random_alignment(rng, columns, rng.integers(-max_columns // 2, tile), **kw))
    return out


def run_alignment(n, pos, at, kind, length, rng):
    """n columns, all '=' but one run of `length` columns of `kind` (2 or 3) that starts at column `at` (clipped to the alignment)."""
    ops = np.zeros(n, dtype=np.uint8)
    ops[max(at, 0):max(min(at + length, n), 0)] = kind
    return int(pos), rng.integers(0, 4, int((ops != 3).sum())).astype(np.uint8), ops


def end_to_end_case(seed=2):
    """A two-contig truth of about 2 kb; the genome handed to the tool is the truth with substitutions and indels planted at 2 %;
    60 reads of 300 .. 400 bases cut from the TRUTH and mutated at 12 %, every other one reverse-complemented; and the seeds=
    hook of map_reads for them (the candidate diagonal in the given genome's concatenated coordinates).
    -> (truth [(name, seq)], given [(name, seq)], reads {name: seq}, seeds {name: dict})."""
    rng = np.random.default_rng(seed)
    truth = [("ctgA", assess_ref.random_seq(1200, rng)), ("ctgB", assess_ref.random_seq(900, rng))]
    given = [(name, assess_ref.mutate(seq, 0.02, rng)) for name, seq in truth]
    given_start = [0, len(given[0][1]) + 15]
    reads, seeds = {}, {}
    for k in range(60):
        c = k % 2
        seq = truth[c][1]
        n = int(rng.integers(300, 401))
        start = int(rng.integers(0, len(seq) - n + 1))
        piece = assess_ref.mutate(seq[start:start + n], 0.12, rng)
        reverse = (k // 2) % 2 == 1
        reads["read%02d" % k] = map_ref.revcomp(piece) if reverse else piece
        seeds["read%02d" % k] = {"strand": "reverse" if reverse else "forward", "delta": given_start[c] + start, "contig": c}
    return truth, given, reads, seeds


def edits_against(truth, sequences):
    """The summed edit distance of {contig: sequence} against the truth's contigs, by the full table."""
    return sum(assess_ref.full_table(sequences[name], seq)[0] for name, seq in truth)


def reference_tracer(reads, refs):
    return [trace_ref.trace(map_ref.as_str(a), map_ref.as_str(b)) for a, b in zip(reads, refs)]


def reference_consensus(source, genome, min_depth=3):
    """The reference pipeline from a pileup source (read_sam / from_map) on: counts, calls, consensus, variants."""
    total = len(genome.codes)
    planes, clipped = pileup_ref.count_columns(source["alignments"], 0, total)
    depth, call = pileup_ref.call_tile(planes, genome.codes, min_depth)
    seqs = pileup_ref.consensus(call, genome.names, genome.starts, genome.lengths)
    recs = pileup_ref.variants(call, depth, planes, genome.codes, genome.names, genome.starts, genome.lengths)
    return {"counts": planes, "depth": depth, "call": call, "clipped": clipped, "consensus": seqs, "variants": recs}
