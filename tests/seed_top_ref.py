"""The candidates kernel's scheme (chiron_seed_candidates, csrc/seed.hip) restated in numpy, pass by pass, and the cases the CPU
and the GPU tests of it share.

chiron_amd.map.vote_top is the definition: it builds the bins and their scores per strand, sorts, and masks.  The kernel keeps
seed_ref.Workgroup's counters and its arithmetic and loops over the picks: the count pass once, then per pick a winner pass that
replays the hits and skips those whose bin lies within n // 256 + 2 of an earlier pick of that strand, the 512-counter delta
histogram over the winning two bins and the two rank passes; the clear pass once, after the last pick.  `TopWorkgroup` is that,
on ONE counter array over all the reads it takes.  test_seed_top_cpu.py checks it against vote_top.
"""
import numpy as np

import assess_ref
import map_ref
import seed_ref
from seed_ref import BIN, SHIFT, THREADS, TOP, rank_find

MAX_CANDIDATES = 8


class TopWorkgroup(seed_ref.Workgroup):
    def seed_top(self, codes, max_cand, min_score=1, clear=True):
        assert 1 <= max_cand <= MAX_CANDIDATES and min_score >= 1
        n = len(codes)
        reach = (n >> SHIFT) + 2
        per = self.hits(codes)
        bins = [(g - r + self.off) >> SHIFT for r, g in per]
        for s in range(2):                                                    # 1: count, once
            assert len(bins[s]) == 0 or (bins[s].min() >= 0 and bins[s].max() + 1 < self.nbins)
            np.add.at(self.cnt[s], bins[s], 1)
        picks, taken = [], ([], [])                                           # taken: the betas of the earlier picks, per strand
        while len(picks) < max_cand:
            best = []
            for s in range(2):                                                # 2: the winner among the hits that are not suppressed
                live = np.ones(len(bins[s]), bool)
                for beta in taken[s]:
                    live &= np.abs(bins[s] - beta) > reach
                b = bins[s][live]
                score = self.cnt[s][b].astype(np.int64) + self.cnt[s][b + 1]
                best.append(int(((score << 32) | (TOP - b)).max()) if len(b) else 0)
            w = 1 if (best[1] >> 32) > (best[0] >> 32) else 0
            votes = best[w] >> 32
            if votes < min_score:
                break
            beta = TOP - (best[w] & 0xFFFFFFFF)
            (r, g), b = per[w], bins[w]
            two = (b == beta) | (b == beta + 1)                               # 3: the deltas of the two bins
            dh = np.zeros(2 * BIN, np.int64)
            np.add.at(dh, (g - r + self.off)[two] - (beta << SHIFT), 1)
            dl, j = rank_find(dh, (votes - 1) // 2)
            assert dl >= 0, "the counters of the two bins do not reach the rank: a stale counter"
            delta = (beta << SHIFT) + dl - self.off
            on = r[g - r == delta]                                            # 4: the j-th read position on that diagonal
            blocks = np.zeros(2 * THREADS, np.int64)
            np.add.at(blocks, on >> SHIFT, 1)
            block, j2 = rank_find(blocks, j)
            flags = np.zeros(2 * THREADS, np.int64)
            np.add.at(flags, on[(on >> SHIFT) == block] - block * THREADS, 1)
            assert flags.max() <= 1
            at, rest = rank_find(flags, j2)
            assert block >= 0 and at >= 0 and rest == 0
            picks.append({"votes": int(votes), "strand": ("forward", "reverse")[w], "delta": int(delta), "g": int(delta + block * THREADS + at)})
            taken[w].append(beta)
        if clear:                                                             # 5: clear by replay, once
            for s in range(2):
                self.cnt[s][bins[s]] = 0
        return picks


def seed_top_all(index, reads, max_cand, min_score=1):
    """Every read through ONE workgroup, in order; its counters are all zero at the end."""
    wg = TopWorkgroup(index, max([len(r) for r in reads] + [0]))
    out = [wg.seed_top(r, max_cand, min_score) for r in reads]
    assert not wg.cnt.any()
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# hand cases: name -> (index, [uint8 code arrays], max_cand, min_score)
# ------------------------------------------------------------------------------------------------------------------------------
def hand_cases():
    from chiron_amd import assess, map as cmap
    enc = assess.encode
    rs = assess_ref.random_seq
    rng = np.random.default_rng(6161)
    cases = {}

    def add(name, text, reads, max_cand=4, min_score=1):
        genome = cmap.Genome([("g", text)])
        cases[name] = (cmap.build_index(genome.codes), [enc(r) for r in reads], max_cand, min_score)

    plant = rs(300, rng)                                                      # n = 300: the radius n // 256 + 2 is 3 bins
    for name, bins_apart in (("copies_at_radius", 3), ("copies_past_radius", 4)):
        add(name, rs(256 * 20, rng) + plant + rs(256 * bins_apart - 300, rng) + plant + rs(8000, rng), [plant, map_ref.revcomp(plant)])
    add("reverse_copy", rs(5000, rng) + plant + rs(6000, rng) + map_ref.revcomp(plant) + rs(4000, rng), [plant, map_ref.revcomp(plant)])
    five = rs(3000, rng)
    for _ in range(5):
        five += plant + rs(2500, rng)
    add("five_copies", five, [plant, map_ref.revcomp(plant)])
    add("five_copies_all", five, [plant], max_cand=8)
    half = rs(150, rng)
    pal = half + map_ref.revcomp(half)                                        # its own reverse complement: equal scores across strands
    add("equal_scores", rs(4000, rng) + pal + rs(5000, rng) + pal + rs(3000, rng), [pal])
    weak = plant[:100] + rs(200, rng)
    add("min_score_cuts", rs(4000, rng) + plant + rs(6000, rng) + weak + rs(4000, rng), [plant], min_score=100)
    add("min_score_one", rs(4000, rng) + plant + rs(6000, rng) + weak + rs(4000, rng), [plant], min_score=1)
    g = rs(6000, rng)
    add("short_reads", g, [g[1000:1000 + n] for n in (0, 1, 14, 15, 16)] + ["N" * 40, rs(300, rng)])
    add("overhang", g, [rs(200, rng) + g[:300], g[-300:] + rs(200, rng), map_ref.revcomp(rs(200, rng) + g[:300])])
    return cases


def random_reads(count=300, size=20000, seed=6262):
    """One genome of `size` bases with planted repeats (three units of 100 .. 500 bases, each at three or four places on either
    strand) and `count` reads of 15 .. 600 bases: cut from it (exact or mutated, often across a repeat), unrelated, or hanging over
    the genome's start (negative deltas) or its end; every other one reverse-complemented.  -> (index, [codes])."""
    from chiron_amd import assess, map as cmap
    rng = np.random.default_rng(seed)
    rs = assess_ref.random_seq
    g = list(rs(size, rng))
    spots = []
    for _ in range(3):
        unit = rs(int(rng.integers(100, 501)), rng)
        for _ in range(int(rng.integers(3, 5))):
            at = int(rng.integers(0, size - len(unit)))
            g[at:at + len(unit)] = unit if rng.integers(2) else map_ref.revcomp(unit)
            spots.append(at)
    g = "".join(g)
    out = []
    for k in range(count):
        n = int(rng.integers(15, 601))
        kind = k % 6
        at = int(rng.integers(0, size - n))
        if kind in (0, 1):
            at = min(max(spots[int(rng.integers(len(spots)))] - int(rng.integers(0, 100)), 0), size - n)
        if kind == 2:
            read = rs(n, rng)
        elif kind == 3:
            read = rs(n // 3, rng) + g[:n - n // 3]                          # overhangs the start
        elif kind == 4:
            read = g[size - (n - n // 3):] + rs(n // 3, rng)                  # overhangs the end
        elif kind == 1:
            read = (assess_ref.mutate(g[at:at + n + 60], 0.1, rng) + "A" * n)[:n]
        else:
            read = g[at:at + n]
        assert len(read) == n
        out.append(map_ref.revcomp(read) if k % 2 else read)
    return cmap.build_index(cmap.Genome([("g", g)]).codes), [assess.encode(r) for r in out]


def hygiene_reads(count=2100):
    """More reads than workgroups, at most 200 bases each, against seed_ref's 30 kb genome with a 150-base unit planted at three
    places: every third read repeats its predecessor, every fifth hits nothing, the others are cut from the genome (every
    other one reverse-complemented), half of them from a copy of the unit."""
    from chiron_amd import assess, map as cmap
    rng = np.random.default_rng(6363)
    g = list(assess_ref.random_seq(seed_ref.HYGIENE_GENOME, rng))
    unit = assess_ref.random_seq(150, rng)
    for at in (3000, 12000, 25000):
        g[at:at + 150] = unit
    g = "".join(g)
    out = []
    for k in range(count):
        n = int(rng.integers(40, 201))
        if k % 3 == 2:
            out.append(out[-1])
        elif k % 5 == 4:
            out.append("N" * n)                                              # no k-mer at all: no hit, whatever the genome
        else:
            at = (3000, 12000, 25000)[k % 3] - 20 if rng.integers(2) else int(rng.integers(0, len(g) - n))
            seq = g[at:at + n]
            out.append(map_ref.revcomp(seq) if k % 2 else seq)
    return cmap.build_index(cmap.Genome([("g", g)]).codes), [assess.encode(r) for r in out]


# ------------------------------------------------------------------------------------------------------------------------------
# the planted repeat: a 3 kb segment copied 10 kb downstream at 1 % substitutions, reads cut from the second copy
# ------------------------------------------------------------------------------------------------------------------------------
REPEAT_SEED = 7
_REPEAT = {}


def repeat_case(seed=REPEAT_SEED, reads=100, controls=20):
    """-> (genome records, {name: read}, truth {name: (start, end)} in the contig).  20 kb random; [4000, 7000) copied to
    [14000, 17000) with 1 % substitutions.  rep<k>: 600 bases cut from the second copy, 12 % errors (a third each deletion,
    insertion, substitution).  ctl<k>: the same from [8000, 13000), unique sequence."""
    if (seed, reads, controls) not in _REPEAT:
        rng = np.random.default_rng(seed)
        g = list(assess_ref.random_seq(20000, rng))
        copy = [("ACGT".replace(ch, "")[int(rng.integers(3))] if rng.random() < 0.01 else ch) for ch in g[4000:7000]]
        g[14000:17000] = copy
        g = "".join(g)
        out, truth = {}, {}
        for k in range(reads + controls):
            name = ("rep%03d" % k) if k < reads else ("ctl%03d" % (k - reads))
            lo, hi = (14000, 17000 - 600) if k < reads else (8000, 13000 - 600)
            at = int(rng.integers(lo, hi))
            out[name] = map_ref.mutate_counted(g[at:at + 600], 0.12, rng)[0]
            truth[name] = (at, at + 600)
        _REPEAT[(seed, reads, controls)] = ([("chr", g)], out, truth)
    return _REPEAT[(seed, reads, controls)]


def on_wrong_copy(rec, truth):
    """A mapped record that overlaps the first copy's image of the read's true interval more than the true interval itself."""
    if rec["status"] != "mapped":
        return False
    lo, hi = truth
    here = max(0, min(rec["end"], hi) - max(rec["start"], lo))
    there = max(0, min(rec["end"], hi - 10000) - max(rec["start"], lo - 10000))
    return there > here
