"""The planted case of the overlap stage, shared by tests/test_overlap_cpu.py (the reference alone) and tests/test_gpu_overlap.py
(the GPU against the reference): reads cut from both strands of a random genome and mutated, so that which pairs overlap, how,
and where is known from where they were cut.

planted(seed): a 20 kb genome, 76 reads of 1.5 to 3 kb and 4 of 0.7 to 1.2 kb cut wholly inside one of the others, 12 % errors (a
    third each deletion, substitution, insertion -- the generator of map_ref.mutate_counted, which here also records where every
    genome base went).  Every other read is reverse-complemented.
truth: every pair whose genome intervals share MIN_SHARED = 500 bases or more.
evaluate: a result of chiron_amd.overlap.find_overlaps against the truth -- the figures of DESIGN's table.
"""
import numpy as np

import assess_ref
import map_ref
import overlap_ref

MIN_SHARED = 500
SEEDS = (11, 12, 13)


def mutate_mapped(seq, rate, rng):
    """map_ref.mutate_counted's walk.  -> (mutated, pos): pos[t] is where genome base t of the piece starts in the mutated read
    (pos[len(seq)] its length)."""
    out, pos = [], []
    for ch in seq:
        pos.append(len(out))
        r = rng.random()
        if r < rate / 3:
            continue
        if r < 2 * rate / 3:
            out.append("ACGT"[rng.integers(4)])
            continue
        out.append(ch)
        if r < rate:
            out.append("ACGT"[rng.integers(4)])
    pos.append(len(out))
    return "".join(out), np.array(pos)


_CACHE = {}


def planted(seed, genome_len=20000, reads=76, inside=4, rate=0.12):
    """-> (reads {name: seq}, truth {name: dict(start, end, strand, pos)}); computed once a seed, never changed."""
    if (seed, genome_len, reads, inside, rate) in _CACHE:
        return _CACHE[seed, genome_len, reads, inside, rate]
    rng = np.random.default_rng(seed)
    g = assess_ref.random_seq(genome_len, rng)
    spans = []
    for k in range(reads):
        n = int(rng.integers(1500, 3001))
        start = int(rng.integers(0, genome_len - n + 1))
        spans.append((start, start + n))
    for k in range(inside):
        lo, hi = spans[int(rng.integers(reads))]
        n = int(rng.integers(700, 1201))
        start = int(rng.integers(lo, hi - n + 1))
        spans.append((start, start + n))
    out, truth = {}, {}
    for k, (lo, hi) in enumerate(spans):
        piece, pos = mutate_mapped(g[lo:hi], rate, rng)
        strand = "reverse" if k % 2 else "forward"
        name = "read%02d" % k
        out[name] = map_ref.revcomp(piece) if strand == "reverse" else piece
        truth[name] = {"start": lo, "end": hi, "strand": strand, "pos": pos}
    _CACHE[seed, genome_len, reads, inside, rate] = (out, truth)
    return out, truth


def shared(ta, tb):
    return min(ta["end"], tb["end"]) - max(ta["start"], tb["start"])


def true_pairs(names, truth):
    """{(i, j), i < j in index order} of the reads whose genome intervals share MIN_SHARED bases or more."""
    return {(i, j) for i in range(len(names)) for j in range(i + 1, len(names)) if shared(truth[names[i]], truth[names[j]]) >= MIN_SHARED}


def expected(ta, tb):
    """What the overlap of a (query) and b (target) should be: (strand, acceptable types, a's span, b's span), the spans in the
    orientation the pair is aligned in -- b as given, a turned onto b's strand."""
    lo, hi = max(ta["start"], tb["start"]), min(ta["end"], tb["end"])

    def span(t, flip):
        x0, x1 = int(t["pos"][lo - t["start"]]), int(t["pos"][hi - t["start"]])
        n = int(t["pos"][-1])
        return (n - x1, n - x0) if flip else (x0, x1)

    flip = tb["strand"] == "reverse"                       # b as given reads the genome backwards: so does the aligned a
    a, b = (ta["start"], ta["end"]), (tb["start"], tb["end"])
    if flip:
        a, b = (-a[1], -a[0]), (-b[1], -b[0])
    kinds = set()
    if a[0] >= b[0] and a[1] <= b[1]:
        kinds.add("contained")
    if b[0] >= a[0] and b[1] <= a[1]:
        kinds.add("contains")
    if not kinds:
        kinds.add("dovetail_ab" if a[0] < b[0] else "dovetail_ba")
    return ("forward" if ta["strand"] == tb["strand"] else "reverse"), kinds, span(ta, flip), span(tb, flip)


def evaluate(names, result, truth):
    """-> dict(true_pairs, found, false_kept, type_right, strand_right, max_end_error) of a find_overlaps result."""
    want = true_pairs(names, truth)
    kept = {}
    for o in result["overlaps"]:
        kept.setdefault((o["a"], o["b"]), []).append(o)
    found = false_kept = type_right = strand_right = worst = 0
    no_shared = 0
    for (i, j), recs in kept.items():
        ta, tb = truth[names[i]], truth[names[j]]
        if shared(ta, tb) <= 0:
            no_shared += len(recs)
        if (i, j) not in want:
            false_kept += len(recs)
            continue
        found += 1
        strand, kinds, a_span, b_span = expected(ta, tb)
        o = recs[0]
        strand_right += o["strand"] == strand
        type_right += o["type"] in kinds
        if o["strand"] == strand:
            worst = max(worst, abs(o["a_start"] - a_span[0]), abs(o["a_end"] - a_span[1]), abs(o["b_start"] - b_span[0]), abs(o["b_end"] - b_span[1]))
    return {"true_pairs": len(want), "found": found, "false_kept": false_kept, "no_shared_bases": no_shared, "type_right": type_right,
            "strand_right": strand_right, "max_end_error": int(worst)}


def typed_case(kind, strand, seed, shared_len=300):
    """Two reads "a" and "b" that share one exact stretch S of shared_len bases in the arrangement `kind`, a given as its reverse
    complement for strand "reverse".  -> (reads, want): want holds what a plain walk over the strings gives -- the type, the
    matches, and the PAF coordinates: where S (or its reverse complement) lies in a as given, and where S lies in b."""
    rng = np.random.default_rng(seed)
    S = assess_ref.random_seq(shared_len, rng)
    f = [assess_ref.random_seq(int(rng.integers(150, 201)), rng) for _ in range(2)]
    a, b = {"contained": (S, f[0] + S + f[1]), "contains": (f[0] + S + f[1], S), "dovetail_ab": (f[0] + S, S + f[1]),
            "dovetail_ba": (S + f[0], f[1] + S)}[kind]
    given = map_ref.revcomp(a) if strand == "reverse" else a
    q0 = given.find(map_ref.revcomp(S) if strand == "reverse" else S)
    t0 = b.find(S)
    assert q0 >= 0 and t0 >= 0
    want = {"type": kind, "strand": strand, "match": shared_len, "edit": 0,
            "paf": ("a", len(a), q0, q0 + shared_len, "+" if strand == "forward" else "-", "b", len(b), t0, t0 + shared_len, shared_len, shared_len, 255)}
    return {"a": given, "b": b}, want


TYPED = [(kind, strand) for kind in ("contained", "contains", "dovetail_ab", "dovetail_ba") for strand in ("forward", "reverse")]


def edge_case():
    """A pair that needs one doubling.  b = F1 + S1 + I + S2 + F2 and a = S1 + S2 with |F| = 50, |S| = 100, |I| = 12 and S2 of period
    4, I twelve T: S1 lies on diagonal 50 and S2 on diagonal 62.  Seeded at diagonal 50 with w = 8 the band is [42, 58]; the best
    path inside it leaves S1 for diagonal 58, where S2 matches itself one period late (8 gaps, 3 mismatches and 1 match against
    I's end, 96 matches: cost -175, against -174 on diagonal 54 and -173 on 50), and ends there, on the band's upper edge.  At
    w = 16 the band [34, 66] holds diagonal 62: S1, twelve gaps, S2, cost -176, away from both edges.
    -> (codes of a and b, the hand-made candidate, the band to start with)."""
    rng = np.random.default_rng(77)
    s1 = assess_ref.random_seq(100, rng)
    f1, f2 = assess_ref.random_seq(50, rng), assess_ref.random_seq(50, rng)
    s2 = "ACGT" * 25
    ins = "T" * 12
    a, b = s1 + s2, f1 + s1 + ins + s2 + f2
    reads = [np.array(overlap_ref.codes_of(x), dtype=np.uint8) for x in (a, b)]
    return reads, {"a": 0, "b": 1, "strand": "forward", "votes": 4, "delta": 50}, 8


def small_forms():
    """Every form at small shapes: n and m of 0, 1, 2, 3 and 17; for each, a band of one diagonal (the lowest, diagonal 0 or the
    nearest to it, the highest), the whole table, a band that touches -n and one that touches m without being the table, bands
    that exclude diagonal 0 from either side, and a band that is clipped on both sides; over a two-letter alphabet, so that ties
    in M, s and e are common, plain and with a code 4 in either read.  -> (reads, pairs)."""
    rng = np.random.default_rng(4242)
    reads, pairs = [], []
    for n in (0, 1, 2, 3, 17):
        for m in (0, 1, 2, 3, 17):
            bands = {(-n, -n), (0, 0), (m, m), (-n, m), (-n, min(m, -n + 2)), (max(-n, m - 2), m), (1, m), (-n, -1), (-n - 5, m + 9),
                     (-(n // 2), m // 2), (max(-n, -2), min(m, 1))}
            for dlo, dhi in sorted(bands):
                if max(dlo, -n) > min(dhi, m):
                    continue
                for form in range(3):
                    a = rng.integers(0, 2, n).astype(np.uint8)
                    b = rng.integers(0, 2, m).astype(np.uint8)
                    if form == 1 and n:
                        a[int(rng.integers(n))] = 4
                    if form == 2 and m:
                        b[int(rng.integers(m))] = 4
                    reads += [a, b]
                    pairs.append((len(reads) - 2, len(reads) - 1, dlo, dhi))
    return reads, np.array(pairs, dtype=np.int64)


_ALIGNED = {}


def reference_aligner(seqs, pairs):
    """chiron_amd.overlap's aligner interface on the reference.  A call is computed once a session: the CPU and the GPU tests ask
    for the same planted calls."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 4)
    key = (pairs.tobytes(),) + tuple(np.asarray(seqs[i], dtype=np.uint8).tobytes() for i in np.unique(pairs[:, :2]))
    if key not in _ALIGNED:
        _ALIGNED[key] = overlap_ref.rows(seqs, pairs)
    return _ALIGNED[key].copy()
