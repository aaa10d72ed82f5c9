"""Reads for the device consensus (chiron_consensus_device, csrc/consensus.hip) at the segment lengths real runs have and the
existing test does not: overlaps of 5 to 39 bases, the clamp of the overlap range by a short segment, ties of the glue score, empty
segments, segment counts around the 1024-segment chunks of the start scan, and a longest segment that a later chunk owns.
tests/test_consensus_cpu.py proves every claim made here with tests/consensus_ref.py alone; tests/test_gpu_consensus.py runs them.

cases() -> [(name, segments, qs, kernal)]: 'ACGT' strings, one float64 quality per segment, "glue" or "stick".  Every read runs
under both kernels unless it is about the glue score.  info(name) holds what a read claims about itself (segment indices)."""
import functools

import numpy as np

CHUNK = 1024                                   # segments per pass of the start scan
CHUNK_COUNTS = (2, 1023, 1024, 1025, 2047, 2048, 2049, 3073)
CLAMP_PREV = (9, 10, 11, 19, 20, 21)


def _s(codes):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.asarray(codes, dtype=np.intp)].tobytes().decode("ascii")


def _rand(rng, n):
    return _s(rng.integers(0, 4, n))


def _tie_column_pair(rng):
    """Two segments that glue overlaps by 3 with one mismatch: overlap 3 scores 2 * 2 - 3 = 1, overlaps 1 and 2 match nowhere.
    Their last shared column holds one G and one T: n1 == n2 == 1, and the base and the quality come from different rows."""
    return [_rand(rng, 56) + "TACG", "ACT" + "C" + _rand(rng, 46)]


def _read_from_genome(rng, n_seg, lo, hi, overlap_hi, p_sub):
    """segments of lo..hi bases cut from one random genome, each overlapping its predecessor by 0..overlap_hi - 1 true bases"""
    genome = rng.integers(0, 4, n_seg * hi + hi)
    segs, true_overlap, pos = [], [0], 0
    for k in range(n_seg):
        ln = int(rng.integers(lo, hi + 1))
        seg = genome[pos:pos + ln].copy()
        flip = rng.random(ln) < p_sub
        seg[flip] = (seg[flip] + rng.integers(1, 4, int(flip.sum()))) % 4
        segs.append(_s(seg))
        o = int(rng.integers(0, overlap_hi))
        true_overlap.append(o)
        pos += ln - o
    return segs, true_overlap[:n_seg]


def _long_overlaps(rng):
    segs, true_overlap = _read_from_genome(rng, 300, 100, 400, 40, 0.03)
    return {"long_overlaps": (segs, {"true_overlap": true_overlap})}


def _clamp(rng):
    segs, pairs = [], []          # pairs: (index of the later segment, which side decides the min(), the overlap glue chooses)

    def pair(prev, cur, side, overlap, then):
        segs.append(prev)
        pairs.append((len(segs), side, overlap))
        segs.append(cur)
        segs.append(then)

    # floor(0.1 * 200) = 20 > n.  The tail has period 4, so every multiple of 4 would score its own length: among the overlaps
    # below n = 6 that is 4, while a loop that ran on to 20 would read into the NEXT segment and choose 16
    pair(_rand(rng, 180) + "ACGT" * 5, "ACGTAC", "n", 4, "GTACGTACGTAC" + _rand(rng, 88))
    pair(_rand(rng, 199) + "G", "G", "n", 0, "G" + _rand(rng, 99))               # n = 1: no overlap is tried
    pair(_rand(rng, 199) + "T", "TA", "n", 1, _rand(rng, 100))                   # n = 2: overlap 1 alone
    for pn in CLAMP_PREV:                                                         # floor(0.1 * pn) = 0, 1, 1, 1, 2, 2
        pair(_rand(rng, pn - 1) + "C", "CA" + _rand(rng, 48), "prev", 1 if pn >= 20 else 0, _rand(rng, 30))
    segs += _tie_column_pair(rng)
    return {"clamp": (segs, {"pairs": pairs})}


def _ties(rng):
    segs, at = [], []             # at: (index of the later segment, the overlaps that share the highest score)

    def pair(prev, cur, tied):
        segs.append(prev)
        at.append((len(segs), tied))
        segs.append(cur)

    pair(_rand(rng, 72) + "ACACACAC", "ACTTACG" + _rand(rng, 40), [2, 6])                    # score 2 twice
    pair(_rand(rng, 71) + "C" + "AAAAAAAA", "ACACCCC" + _rand(rng, 40), [1, 3])              # score 1 twice
    pair(_rand(rng, 91) + "ACGACGACG", "ACGTTTACG" + _rand(rng, 40), [3, 9])                 # score 3 twice
    pair(_rand(rng, 118) + "ACACACACACAC", "ACTTACTTACGG" + _rand(rng, 40), [2, 6, 10])      # score 2 three times
    segs += _tie_column_pair(rng)
    return {"ties": (segs, {"tied": at})}


def _empties(rng):
    head, _ = _read_from_genome(rng, 6, 50, 80, 7, 0.03)
    tail, _ = _read_from_genome(rng, 6, 50, 80, 7, 0.03)
    base = head + _tie_column_pair(rng) + tail                                    # 14 segments
    out = {}
    for name, at in (("first", [0]), ("second", [1]), ("middle", [5]), ("two_in_a_row", [10, 10]), ("last", [len(base)])):
        segs = list(base)
        for k in at:
            segs.insert(k, "")
        out["empties.%s" % name] = (segs, {"empty": sorted(i for i, s in enumerate(segs) if not s)})
    out["empties.all"] = ([""] * 5, {"empty": list(range(5))})
    return out


def _chunks(rng):
    return {"chunks.n%d" % n: ([_rand(rng, int(k)) for k in rng.integers(1, 13, n)], {}) for n in CHUNK_COUNTS}


def _longest_late(rng):
    """2500 segments of 1..3 bases and one of 600.  The segment after the long one repeats its last two bases, so glue overlaps
    the two by 2: the only columns of the read where the vote has to walk back to a segment that starts more than 3 columns
    earlier, which it does only if the scan's `maxn` is the 600 of the long segment.  A third read puts a 30-base and a 3-base
    segment behind the long one, all three sharing the long one's last column: the walk back crosses a segment to reach it."""
    out = {}
    for at in (1500, 2300):                                                       # a full second chunk / the partial third
        segs = [_rand(rng, int(k)) for k in rng.integers(1, 4, 2500)]
        segs.insert(at, _rand(rng, 600))
        segs[at + 1] = segs[at][-2:] + _rand(rng, 1)
        out["longest_late.index%d" % at] = (segs, {"longest": at})
    segs = [_rand(rng, int(k)) for k in rng.integers(1, 4, 2500)]
    long = _rand(rng, 600)
    z = "ACGT".replace(long[-1], "")[int(rng.integers(0, 3))]
    segs[1500:1500] = [long, long[-29:] + z, long[-1] + z + _rand(rng, 1)]       # overlaps 29 and 2: both start inside the long one
    out["longest_late.crossed"] = (segs, {"longest": 1500})
    return out


GLUE_ONLY = ("clamp", "ties")


@functools.lru_cache(maxsize=None)
def _build():
    reads = {}
    for seed, builder in enumerate((_long_overlaps, _clamp, _ties, _empties, _chunks, _longest_late)):
        reads.update(builder(np.random.default_rng([4711, seed])))                # a stream each: a new read moves no other
    rng = np.random.default_rng([4711, 99])
    qs = {name: rng.uniform(0.0, 25.0, len(segs)) for name, (segs, _) in reads.items()}
    return reads, qs


def names():
    return list(_build()[0])


def read(name):
    """-> (segments, qs)"""
    reads, qs = _build()
    return list(reads[name][0]), qs[name].copy()


def info(name):
    return _build()[0][name][1]


def kernals(name):
    return ("glue",) if name in GLUE_ONLY else ("glue", "stick")


def cases():
    return [(name,) + read(name) + (kernal,) for name in names() for kernal in kernals(name)]
