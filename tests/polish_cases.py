"""Inputs shared by tests/test_polish_cpu.py and tests/test_gpu_polish.py: planted score matrices and the end-to-end case."""
import numpy as np

from chiron_amd import assess, map as cmap, pileup, polish

import assess_ref
import ctc_align_ref
import map_ref
import pileup_cases
import pileup_ref
import polish_ref

SEED = 5
BLANK = polish_ref.BLANK


def planted(rng, lab, dwell_p=0.4, weak=0.0):
    """A score matrix planted over the bases `lab` in the way of _planted_exact of tests/test_gpu_label.py: unit normal noise, +6 on
    the path's class, a geometric dwell per base (mean 1 / dwell_p) and a blank frame between equal neighbours.  At a share `weak`
    of the bases the path's class is weakened to +2 and one of the four other classes (blank included) is lifted half a unit above
    it on every frame of the base: the greedy decode goes wrong exactly where the scores are ambiguous."""
    lab = np.asarray(lab, dtype=np.uint8)
    dwell = rng.geometric(dwell_p, size=len(lab))
    soft = rng.random(len(lab)) < weak
    classes, wrong = [], []
    for j in range(len(lab)):
        if j and lab[j] == lab[j - 1]:
            classes.append(BLANK)
            wrong.append(-1)
        other = int((lab[j] + rng.integers(1, 5)) % 5) if soft[j] else -1
        classes += [int(lab[j])] * int(dwell[j])
        wrong += [other] * int(dwell[j])
    F = len(classes)
    x = rng.standard_normal((F, 5)).astype(np.float32)
    classes, wrong = np.array(classes), np.array(wrong)
    rows = np.arange(F)
    x[rows, classes] += np.float32(6)
    w = wrong >= 0
    x[rows[w], classes[w]] -= np.float32(4)
    x[rows[w], wrong[w]] = x[rows[w], classes[w]] + np.float32(0.5)
    return x


def end_to_end_case(seed=SEED):
    """A two-contig truth of about 2 kb; the draft is the truth mutated at 2 %; 60 reads of 300 .. 400 bases cut from the TRUTH,
    every other pair reverse-complemented.  A read is its score matrix, planted over the truth with 12 % of its bases made
    ambiguous, and its called sequence is the greedy decode of that matrix.
    -> (truth [(name, seq)], draft [(name, seq)], called {name: seq}, logits {name: float32 [F, 5]}, seeds for map_reads)."""
    rng = np.random.default_rng(seed)
    truth = [("ctgA", assess_ref.random_seq(1200, rng)), ("ctgB", assess_ref.random_seq(900, rng))]
    draft = [(name, assess_ref.mutate(seq, 0.02, rng)) for name, seq in truth]
    draft_start = [0, len(draft[0][1]) + cmap.SEPARATOR]
    called, logits, seeds = {}, {}, {}
    for k in range(60):
        c = k % 2
        seq = truth[c][1]
        n = int(rng.integers(300, 401))
        start = int(rng.integers(0, len(seq) - n + 1))
        reverse = (k // 2) % 2 == 1
        piece = map_ref.revcomp(seq[start:start + n]) if reverse else seq[start:start + n]
        name = "read%02d" % k
        logits[name] = planted(rng, assess.encode(piece), weak=0.12)
        called[name] = map_ref.as_str(polish_ref.greedy_decode(logits[name]))
        seeds[name] = {"strand": "reverse" if reverse else "forward", "delta": draft_start[c] + start, "contig": c}
    return truth, draft, called, logits, seeds


def reads_of(result, called, logits, genome):
    """The read dicts of chiron_amd.polish from a map_reads result that went through add_cigars, in memory (what
    polish.reads_from_sam makes of a mapped.sam)."""
    contig = {name: c for c, name in enumerate(genome.names)}
    out = []
    for r in result["reads"]:
        if r["status"] != "mapped" or "cigar" not in r:
            continue
        out.append({"name": r["name"], "pos": int(genome.starts[contig[r["contig"]]]) + r["start"], "ops": pileup.ops_from_cigar(r["cigar"], r["name"]),
                    "reverse": r["strand"] == "reverse", "lead": 0, "called": assess.encode(called[r["name"]]), "logits": logits[r["name"]]})
    return out


def reference_pipeline(draft, called, logits, seeds, **kw):
    """map_reads, add_cigars, pileup.count and polish.polish on the numpy references alone.
    -> (genome, pileup result, polish result)."""
    genome = cmap.Genome(draft)
    res = cmap.map_reads(called, genome, seeds=seeds, aligner=lambda rs, ws, b: map_ref.infix_rows(rs, ws, b, cmap.INFIX_DTYPE))
    cmap.add_cigars(res, called, genome, tracer=pileup_cases.reference_tracer)
    source = pileup.from_map(res, called, genome)
    piled = pileup.count(source["alignments"], genome, counter=pileup_ref.counter, want_counts=True)
    out = polish.polish(reads_of(res, called, logits, genome), genome, piled["counts"], piled["depth"], scorer=polish_ref.score,
                        frame_aligner=ctc_align_ref.align, **kw)
    return genome, piled, out


def edits_against(truth, sequences):
    return pileup_cases.edits_against(truth, sequences)
