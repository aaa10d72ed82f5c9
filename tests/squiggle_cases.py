"""Inputs for the squiggle tests, seeded and independent of the code under test: random reduction sets, random alignments, and the
planted sample-compare case.

The planted case (planted()).  A 600-base genome, a random 5-mer level table (mean 100, sd TABLE_SD = 15), two samples of 30 reads of
150 to 300 bases on both strands.  A base's samples are its 5-mer's level (the genome 5-mer around it in the read's orientation; the
table's mean where the window leaves the genome) plus noise of sd 3, for a geometric dwell of mean 9; every read then gets its own
gain (0.8 .. 1.2) and offset (-20 .. 20) and an unlabelled head of 0 .. 50 samples.  In sample A's forward reads the bases at
positions 298 .. 302 -- the ones whose 5-mer covers position 300 -- are 1.5 TABLE_SD higher.  The reads are error-free ('=' columns
only), so the frames are tied to bases by a forced alignment the case itself knows (frame_aligner_of): with segment_len 400 and
ratio 1 a frame is a sample.

Margin of this module, from the numpy reference: at each of the seeds 1 .. 5 the five largest |t| of `compare` (min_events 5) are
forward 298 .. 302.  At PLANTED_SEED = 3 the smallest of the five is 16.6 and the sixth largest |t| anywhere is 4.02; over the five
seeds the fifth is at least 10.8 and the sixth at most 4.99.  test_squiggle_cpu.py asserts the order and prints both figures."""
import numpy as np

PLANTED_SEED = 3
TABLE_SD = 15.0
SEGMENT_LEN, RATIO = 400, 1.0
_COMPLEMENT = np.array([3, 2, 1, 0, 4], dtype=np.uint8)


def random_set(rng, reads=None, n_bins=None, max_span=12, empty=0.1):
    """(signals, starts, bins, n_bins): reads of 0 to 40 bases with an unlabelled head, spans of 0 .. max_span samples (a share
    `empty` of them empty), unowned samples behind the last base, samples over all of int16, bins -1 .. n_bins - 1."""
    reads = int(rng.integers(0, 6)) if reads is None else reads
    n_bins = int(rng.integers(0, 9)) if n_bins is None else n_bins
    signals, starts, bins = [], [], []
    for _ in range(reads):
        bases = int(rng.integers(0, 41))
        spans = rng.integers(1, max_span + 1, bases)
        spans[rng.random(bases) < empty] = 0
        head, tail = int(rng.integers(0, 5)), int(rng.integers(0, 4))
        st = head + np.concatenate([[0], np.cumsum(spans)])
        n = int(st[-1]) + tail
        lo, hi = ((-32768, 32768) if rng.random() < 0.5 else (-40, 41))
        signals.append(rng.integers(lo, hi, n).astype(np.int16))
        starts.append(st.astype(np.int32))
        bins.append(rng.integers(-1, n_bins, bases).astype(np.int32) if n_bins else np.full(bases, -1, np.int32))
    return signals, starts, bins, n_bins


def spans_set(rng, spans_per_read, n_bins, heads=None, low=-32768, high=32768):
    """Reads whose bases have exactly the given sample counts; heads[r] unowned samples in front of read r."""
    signals, starts, bins = [], [], []
    for r, spans in enumerate(spans_per_read):
        head = 0 if heads is None else heads[r]
        st = head + np.concatenate([[0], np.cumsum(np.asarray(spans, dtype=np.int64))])
        signals.append(rng.integers(low, high, int(st[-1])).astype(np.int16))
        starts.append(st.astype(np.int32))
        bins.append(rng.integers(-1, n_bins, len(spans)).astype(np.int32) if n_bins else np.full(len(spans), -1, np.int32))
    return signals, starts, bins, n_bins


def random_read(rng, genome_len, name="r", reverse=None, lead=None, pos=None, columns=None):
    """A read dict of polish.py with random '=', 'X', 'I', 'D' columns somewhere on a genome of genome_len positions.  The called
    sequence is random: only the columns matter to the bins."""
    columns = int(rng.integers(1, 60)) if columns is None else columns
    ops = rng.choice(np.array([0, 0, 0, 1, 2, 3], dtype=np.uint8), columns)
    m = int((ops != 2).sum())
    pos = int(rng.integers(0, max(genome_len - m, 0) + 1)) if pos is None else pos
    lead = int(rng.integers(0, 6)) if lead is None else lead
    n = lead + int((ops != 3).sum()) + int(rng.integers(0, 4))           # a trailing clip as well
    return {"name": name, "pos": pos, "ops": ops, "reverse": bool(rng.integers(0, 2)) if reverse is None else reverse, "lead": lead,
            "called": rng.integers(0, 4, n).astype(np.uint8)}


class PlainGenome(object):
    """What the module uses of map.Genome, for one contig."""

    def __init__(self, codes, name="ctg"):
        self.codes = np.asarray(codes, dtype=np.uint8)
        self.names, self.starts, self.lengths = [name], np.zeros(1, np.int64), np.array([len(self.codes)], np.int64)

    def contig_of(self, g):
        return 0


def _kmer_level(table, codes, g, reverse, k=5):
    h = k // 2
    window = [g + h - j for j in range(k)] if reverse else [g - h + j for j in range(k)]
    if min(window) < 0 or max(window) >= len(codes):
        return float(table.mean())
    code = 0
    for p in window:
        code = code * 4 + (3 - int(codes[p]) if reverse else int(codes[p]))
    return float(table[code])


def planted_sample(rng, codes, table, n_reads, shifted):
    """[read dict with raw, logits, seq_lens and the planted `true_starts`] of one sample."""
    reads = []
    for k in range(n_reads):
        n = int(rng.integers(150, 301))
        pos = int(rng.integers(0, len(codes) - n + 1))
        if k < 12:                                       # enough reads over the planted site on either strand
            pos = int(rng.integers(max(0, 305 - n), min(295, len(codes) - n) + 1))
        reverse = k % 2 == 1
        piece = codes[pos:pos + n]
        called = _COMPLEMENT[piece[::-1]] if reverse else piece.copy()
        gs = (pos + n - 1 - np.arange(n)) if reverse else (pos + np.arange(n))           # genome position of every base, signal order
        dwell = rng.geometric(1.0 / 9.0, n)
        head = int(rng.integers(0, 51))
        starts = head + np.concatenate([[0], np.cumsum(dwell)])
        x = np.empty(int(starts[-1]), dtype=np.float64)
        x[:head] = table.mean() + rng.normal(0, 3.0, head)
        for i in range(n):
            lv = _kmer_level(table, codes, int(gs[i]), reverse)
            if shifted and not reverse and 298 <= gs[i] <= 302:
                lv += 1.5 * TABLE_SD
            x[starts[i]:starts[i + 1]] = lv + rng.normal(0, 3.0, int(dwell[i]))
        raw = (x * rng.uniform(0.8, 1.2) + rng.uniform(-20, 20)).astype(np.float32)
        windows = (len(raw) + SEGMENT_LEN - 1) // SEGMENT_LEN
        seq_lens = np.minimum(len(raw) - SEGMENT_LEN * np.arange(windows), SEGMENT_LEN).astype(np.int64)
        reads.append({"name": "read%d" % k, "pos": pos, "ops": np.zeros(n, np.uint8), "reverse": reverse, "lead": 0, "called": called.astype(np.uint8),
                      "raw": raw, "logits": np.zeros((len(raw), 5), np.float32), "seq_lens": seq_lens, "true_starts": starts[:-1].astype(np.int32)})
    return reads


def planted(seed=PLANTED_SEED):
    """dict(genome, table, a, b): sample a carries the shift, b is the control."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 4, 600).astype(np.uint8)
    table = 100.0 + TABLE_SD * rng.standard_normal(4 ** 5)
    return {"genome": PlainGenome(codes), "table": table, "a": planted_sample(rng, codes, table, 30, True),
            "b": planted_sample(rng, codes, table, 30, False)}


def frame_aligner_of(reads):
    """The forced alignment the case knows, in the place of label.align: a frame is a sample, so a base's first frame is its first
    sample.  The reads are found by their logits arrays, which polish.align_frames hands through as they are."""
    known = {id(r["logits"]): r["true_starts"] for r in reads}

    def aligner(scores, labels, band0, max_band):
        n = len(scores)
        return {"start": [known[id(x)] for x in scores], "score": np.zeros(n), "band": np.zeros(n, np.int32), "status": np.zeros(n, np.int32)}
    return aligner
