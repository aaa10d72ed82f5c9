"""Inputs for the modcall tests, seeded and independent of the code under test: random calls for chiron_signal_score, the small
cases a brute force can enumerate, and the planted per-read modification case.

The planted case (planted()).  The genome and the 5-mer level table of squiggle_cases.planted(seed) (600 bases; mean 100, sd TABLE_SD
= 15), the genome through within_scope (below).  The alternative table shifts every 5-mer that contains CG by N(0, 1 TABLE_SD).  A read is generated as there -- a base's
samples are its 5-mer's level plus noise of sd 3 for a geometric dwell of mean 9, then the read's own gain, offset and unlabelled
head; error-free, both strands -- except that the level comes from the alternative table for every base whose 5-mer holds a whole CG
of a group that is modified IN THIS READ.  On one strand CG occurrences fewer than 5 bases apart are one group (groups_of, a plain
walk); a read draws a state for every group of its strand.
  a        30 reads, every (read, group) modified with probability 1/2; the truth is kept in read["truth"]: {sites: state}, the key
           being the group's site positions (the position of the C on the read's strand)
  b        30 reads, nothing modified
  train0   TRAIN reads, nothing modified; train1: TRAIN reads, every group modified.  tables_of() learns the two tables from them
           as a user would: `squiggle --kmer 5` at the true borders, at least 5 events a 5-mer
  a_jit, b_jit   a and b with every border moved by up to JITTER = 6 samples, as refine_cases.jittered does

Figures of this module with the numpy reference (tests/site_ref.py) as the scorer, flank 2, min_delta 8, seeds 1 .. 5; asserted, at
the worst seed less (or plus) a margin of 0.02, by tests/test_modcall_cpu.py, which prints them:
  sign of delta names the truth, a                    0.9811 .. 0.9892 of 271 .. 380 scored pairs a seed
  the same among |delta| >= 8                         0.9923 .. 1.0000, with 0.853 .. 0.956 of the pairs above the threshold
  b's pairs called `modified`                         0.0000 .. 0.0031
  after squiggle.refine with the canonical table (numpy refiner), a: sign 0.9779 .. 0.9901, above the threshold 0.9922 .. 1.0000:
  the borders that refinement pulls wrong at a modified site do not matter, the window's borders being free
  share of the (read, group) pairs that are scored    a: 0.9633, 0.9377, 0.9500, 0.9755, 0.9463; b: 0.9527, 0.9615, 0.9725, 0.9492,
                                                      0.9615.  The condition is 0.9 at every seed, so that dropped pairs cannot
                                                      hide failures.  The drops are windows that leave the read (7 .. 19 a sample)
                                                      and 5-mers the training runs saw fewer than 5 times (0 .. 4).
The genome is kept inside the stage's stated scope (within_scope): a CG chain whose window would be above 16 columns at the default
flank is cut at its last CG, whose G becomes an A.  §19's genome needs that at seed 1 only -- chains at 60, 64, 68; 185, 189, 191,
194; 355, 359, 363, of 17 and 18 columns -- and three bases change there (69, 195, 364); left as they were, 41 of a's 355 pairs at
that seed would be dropped as `too_wide` for every read and 0.8535 of them scored."""
import numpy as np

import refine_cases
import squiggle_cases
from squiggle_cases import RATIO, SEGMENT_LEN, TABLE_SD  # noqa: F401  the tests take them from here

K = 5
FLANK, COLUMNS = 2, 16                   # the stage's default flank and the columns a candidate may have, restated
JITTER = refine_cases.JITTER
TRAIN = 200
SEEDS = (1, 2, 3, 4, 5)
PLANTED_SEED = 3
_COMPLEMENT = np.array([3, 2, 1, 0, 4], dtype=np.uint8)


# ----------------------------------------------------------------------------------------------------------------------------
# calls for the kernel
# ----------------------------------------------------------------------------------------------------------------------------
def samples_of(rng, n, wide):
    lo, hi = ((-32768, 32768) if wide else (-40, 41))
    return rng.integers(lo, hi, n).astype(np.int16)


def levels_of(rng, n, wide):
    lo, hi = ((-32767, 32768) if wide else (-40, 41))
    return rng.integers(lo, hi, n).astype(np.int32)


def random_call(rng, segments, candidates, max_samples=300, max_levels=16, wide=None):
    """(segments, candidates): segments of 0 .. max_samples samples, candidates of 1 .. max_levels levels on random segments."""
    segs, cands = [], []
    kinds = [bool(rng.integers(0, 2)) if wide is None else wide for _ in range(segments)]
    for g in range(segments):
        segs.append(samples_of(rng, int(rng.integers(0, max_samples + 1)), kinds[g]))
    for _ in range(candidates):
        g = int(rng.integers(0, segments))
        cands.append((g, levels_of(rng, int(rng.integers(1, max_levels + 1)), kinds[g])))
    return segs, cands


def small_case(rng):
    """(x, e) small enough to enumerate: 0 .. 7 samples, 1 .. 5 levels; half of them from few values, so that ties occur."""
    S, L = int(rng.integers(0, 8)), int(rng.integers(1, 6))
    wide = bool(rng.integers(0, 2))
    x, e = samples_of(rng, S, wide), levels_of(rng, L, wide)
    if not wide:
        x, e = (x // 20).astype(np.int16), (e // 20).astype(np.int32)
    return x, e


# ----------------------------------------------------------------------------------------------------------------------------
# the planted case
# ----------------------------------------------------------------------------------------------------------------------------
def holds_cg(code, k=K):
    bases = [(code >> (2 * (k - 1 - j))) & 3 for j in range(k)]
    return any(bases[j] == 1 and bases[j + 1] == 2 for j in range(k - 1))


def alternative_table(rng, table, k=K):
    shift = rng.normal(0.0, TABLE_SD, len(table))
    return np.array([table[c] + (shift[c] if holds_cg(c, k) else 0.0) for c in range(len(table))])


def groups_of(codes, reverse, k=K):
    """A plain walk.  [[p, ...]]: the forward positions p of the C of every CG dinucleotide (CG is its own reverse complement, so
    both strands have the same occurrences), cut into groups wherever two are k or more apart.  The site of an occurrence is p on the
    forward strand and p + 1, where the reverse strand has its C, on the reverse one."""
    groups = []
    for p in range(len(codes) - 1):
        if codes[p] == 1 and codes[p + 1] == 2:
            if groups and p - groups[-1][-1] < k:
                groups[-1].append(p)
            else:
                groups.append([p])
    return groups


def sites_key(group, reverse):
    return tuple(p + 1 if reverse else p for p in group)


def _level(table, alt, codes, g, reverse, modified_at, k=K):
    """The level of the base at genome position g: its 5-mer in the read's orientation, from the alternative table when it holds a
    whole CG whose C (forward position) is in modified_at; the table's mean where the window leaves the genome."""
    h = k // 2
    window = [g + h - j for j in range(k)] if reverse else [g - h + j for j in range(k)]
    if min(window) < 0 or max(window) >= len(codes):
        return float(table.mean())
    code = 0
    for p in window:
        code = code * 4 + (3 - int(codes[p]) if reverse else int(codes[p]))
    lo = min(window)
    hit = any(p in modified_at for p in range(lo, lo + k - 1))         # both bases of the CG inside the window
    return float(alt[code] if hit else table[code])


def planted_sample(rng, codes, table, alt, n_reads, mode, prefix):
    """mode: 'half' (a state per (read, group) with probability 1/2), 'none' or 'all'."""
    per_strand = [groups_of(codes, False), groups_of(codes, True)]
    reads = []
    for i in range(n_reads):
        n = int(rng.integers(150, 301))
        pos = int(rng.integers(0, len(codes) - n + 1))
        reverse = i % 2 == 1
        piece = codes[pos:pos + n]
        called = _COMPLEMENT[piece[::-1]] if reverse else piece.copy()
        gs = (pos + n - 1 - np.arange(n)) if reverse else (pos + np.arange(n))
        truth, modified_at = {}, set()
        for group in per_strand[int(reverse)]:
            state = {"half": bool(rng.integers(0, 2)), "none": False, "all": True}[mode]
            truth[sites_key(group, reverse)] = state
            if state:
                modified_at.update(group)
        dwell = rng.geometric(1.0 / 9.0, n)
        head = int(rng.integers(0, 51))
        starts = head + np.concatenate([[0], np.cumsum(dwell)])
        x = np.empty(int(starts[-1]), dtype=np.float64)
        x[:head] = table.mean() + rng.normal(0, 3.0, head)
        for b in range(n):
            x[starts[b]:starts[b + 1]] = _level(table, alt, codes, int(gs[b]), reverse, modified_at) + rng.normal(0, 3.0, int(dwell[b]))
        raw = (x * rng.uniform(0.8, 1.2) + rng.uniform(-20, 20)).astype(np.float32)
        windows = (len(raw) + SEGMENT_LEN - 1) // SEGMENT_LEN
        seq_lens = np.minimum(len(raw) - SEGMENT_LEN * np.arange(windows), SEGMENT_LEN).astype(np.int64)
        reads.append({"name": "%s%d" % (prefix, i), "pos": pos, "ops": np.zeros(n, np.uint8), "reverse": reverse, "lead": 0,
                      "called": called.astype(np.uint8), "raw": raw, "logits": np.zeros((len(raw), 5), np.float32), "seq_lens": seq_lens,
                      "true_starts": starts[:-1].astype(np.int32), "truth": truth})
    return reads


def within_scope(codes, k=K, flank=FLANK, columns=COLUMNS):
    """A copy of the genome in which no CG chain is wider than a window may be, and the chains that were cut.  A group whose first
    and last C are more than columns - k - 2 flank = 7 positions apart has a window above `columns` = 16 at the default flank, which
    the stage states as out of scope and drops for every read; a case that planted states there could not have them called, and the
    drops would hide what else goes wrong.  So the case plants none: while a chain is too wide the G of its last CG becomes an A
    (which makes no new CG), chain by chain from the left.  Only the genome and the stated limit enter this rule."""
    codes = np.array(codes, dtype=np.uint8)
    cut = []
    while True:
        wide = [g for g in groups_of(codes, False, k) if g[-1] - g[0] > columns - k - 2 * flank]
        if not wide:
            return codes, cut
        codes[wide[0][-1] + 1] = 0
        cut.append(wide[0][-1])


def planted(seed=PLANTED_SEED):
    """dict(genome, table, alt, a, b, train0, train1, a_jit, b_jit, cut: the CGs within_scope took out)."""
    base = squiggle_cases.planted(seed)
    table = base["table"]
    codes, cut = within_scope(base["genome"].codes)
    genome = squiggle_cases.PlainGenome(codes)
    rng = np.random.default_rng(2000 + seed)
    alt = alternative_table(rng, table)
    case = {"genome": genome, "table": table, "alt": alt, "cut": cut,
            "a": planted_sample(rng, codes, table, alt, 30, "half", "a"), "b": planted_sample(rng, codes, table, alt, 30, "none", "b"),
            "train0": planted_sample(rng, codes, table, alt, TRAIN, "none", "t"), "train1": planted_sample(rng, codes, table, alt, TRAIN, "all", "u")}
    case["a_jit"], case["b_jit"] = refine_cases.jittered(case["a"], rng), refine_cases.jittered(case["b"], rng)
    return case


def tables_of(case, min_events=5):
    """(canonical, alternative) int32 [4^5]: what `squiggle --kmer 5` learns from the two training runs at their true borders, with
    the numpy reference as the reducer."""
    import squiggle_ref
    from chiron_amd import squiggle
    out = []
    for name in ("train0", "train1"):
        got = squiggle.sample(case[name], case["genome"], SEGMENT_LEN, RATIO, reducer=squiggle_ref.reduce_numpy,
                              frame_aligner=squiggle_cases.frame_aligner_of(case[name]), kmer=K)
        out.append(squiggle.table_of(got["kmer_planes"], min_events))
    return tuple(out)


def prepared(reads):
    """The reads as modcall takes them: squiggle.prepare with the forced alignment the case knows."""
    from chiron_amd import squiggle
    kept, drops = squiggle.prepare(reads, SEGMENT_LEN, RATIO, frame_aligner=squiggle_cases.frame_aligner_of(reads))
    assert len(kept) == len(reads) and not any(drops.values())
    return kept


def judge(rows, reads, min_delta):
    """rows of modcall.modcall against the reads' truth -> dict(scored, sign: share whose sign of delta names the truth, sure: share of
    the pairs with |delta| >= min_delta, sign_sure: the share right among those, modified: share called modified)."""
    truth = {r["name"]: r["truth"] for r in reads}
    right = sure = right_sure = modified = 0
    for row in rows:
        state = truth[row["read"]][tuple(row["sites"])]
        ok = (row["delta"] > 0) == state
        right += ok
        if abs(row["delta"]) >= min_delta:
            sure += 1
            right_sure += ok
        modified += row["call"] == "modified"
    n = max(len(rows), 1)
    return {"scored": len(rows), "sign": right / n, "sure": sure / n, "sign_sure": right_sure / max(sure, 1), "modified": modified / n}
