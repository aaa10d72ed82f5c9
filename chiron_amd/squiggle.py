"""Squiggle: the reads' current levels on the genome, and two samples compared position by position.

Everything else here works in base space.  This module puts the signal itself on the reference: per read, the samples of every called
base are reduced to one level (their mean, rounded), and the levels are summed per genome position and strand -- or per k-mer, which
gives a pore model of the run.  From the sums a native sample is compared with a control by Welch's t per position (`compare`):
sample-compare detection of modified bases, in the family of Tombo's sample compare and Nanocompore.

What ties a sample to a position is already in the tree: label.align ties frames to called bases, label.frames_to_samples frames to
samples (base_starts), and a `map --cigar` alignment called bases to genome positions with strand and leading clip
(polish.reads_from_sam; genome_bins uses polish.read_window's index mapping).  The stage that joins them is the library's
chiron_signal_levels (csrc/signal.hip): a segmented reduction over the samples of every base and a scatter-add into four int64
planes per bin -- events, dwell, sum of levels, sum of squared levels.  It is defined on integers, so it is exact and reproducible.

A read here is polish.py's dict(name, pos, ops, reverse, called, lead) plus `signal` (int16, normalise) and `starts` (int32
[bases + 1], base_starts), both in signal order.  The strands are separate planes: a reverse-strand read's signal saw the
complementary k-mers.

The reduction is the library's; everything else is plain numpy.  There is no CPU fallback: the hooks reducer= and frame_aligner= exist
for the tests' reference.

With a level table (`squiggle --refine`, the kmer_levels.tsv of an earlier run) the borders are first moved to where the samples
change level: expected_levels gives every base the level of its k-mer, refine_items cuts a read into the runs of bases that have
one, and the library's chiron_signal_refine (csrc/refine.hip) runs an exact banded DTW of each run's samples against its levels,
64 candidates a border around the frame alignment's.  refiner= replaces that stage in the tests."""
import json
import os

import numpy as np

from . import _lib, label, polish

PLANES, EMPTY = _lib.SIGNAL_PLANES, _lib.SIGNAL_EMPTY
MAX_SAMPLES, MAX_BINS = _lib.SIGNAL_MAX_SAMPLES, _lib.SIGNAL_MAX_BINS
THREADS, MAX_GROUPS = _lib.SIGNAL_THREADS, _lib.SIGNAL_MAX_GROUPS
EVENTS, DWELL, SUM, SQ = 0, 1, 2, 3
SCALE = 256                              # int16 units of one MAD-scaled unit of current
MAD_FACTOR = 0.6744897501960817
MODES = ("mad", "none")
MAX_K = 10
READ_DROPS = ("no_signal", "no_frames", "outside_acgt", "flat_signal", "infeasible", "band_exhausted")
LEVEL_COLUMNS = ("contig", "pos", "strand", "ref", "events", "mean_dwell", "mean", "sd")
COMPARE_COLUMNS = ("contig", "pos", "strand", "ref", "events_a", "mean_a", "sd_a", "events_b", "mean_b", "sd_b", "t", "df", "effect")
KMER_COLUMNS = ("kmer", "events", "mean_dwell", "mean", "sd")
EVENT_COLUMNS = ("start", "length", "level", "contig", "pos")
REFINE_HALF, INFEASIBLE = _lib.REFINE_HALF, _lib.REFINE_INFEASIBLE
UNKNOWN = EMPTY                          # a base without an expected level, a k-mer without a table entry
REFINE_COUNTS = ("items", "bases", "infeasible", "borders", "moved", "mean_move", "cost")


# ----------------------------------------------------------------------------------------------------------------------------
# samples, starts, bins
# ----------------------------------------------------------------------------------------------------------------------------
def normalise(signal, mode="mad"):
    """The read's samples as int16.  mad: m = median, d = median|x - m| / 0.6744897501960817, both in float64, and the result is
    clip(rint((x - m) / d * SCALE), -32767, 32767); None when d = 0 (a flat signal: the caller drops the read).  none:
    clip(rint(x))."""
    if mode not in MODES:
        raise ValueError("normalise mode %r is neither of %s" % (mode, "/".join(MODES)))
    x = np.asarray(signal, dtype=np.float64).reshape(-1)
    if mode == "mad":
        if x.size == 0:
            return None
        m = np.median(x)
        d = np.median(np.abs(x - m)) / MAD_FACTOR
        if d == 0:
            return None
        x = (x - m) / d * SCALE
    return np.clip(np.rint(x), -32767, 32767).astype(np.int16)


def base_starts(start_frames, seq_lens, segment_len, ratio, signal_len):
    """int32 [bases + 1]: the first sample of every base (label.frames_to_samples of its first frame) and, last, signal_len, as
    label.spans ends the last base.  Two bases may start in one sample: an empty span is legal here, unlike in label."""
    s = label.frames_to_samples(start_frames, seq_lens, segment_len, ratio, signal_len)
    return np.concatenate([s, [int(signal_len)]]).astype(np.int32)


def _columns(read):
    """Per '=' / 'X' column of the read's alignment: (genome position, index of its base in read["called"], signal orientation)."""
    ops = np.asarray(read["ops"], dtype=np.uint8)
    n, lead = len(read["called"]), int(read["lead"])
    consumes_read, consumes_ref = ops != 3, ops != 2
    aligned = int(consumes_read.sum())
    if lead < 0 or lead + aligned > n:
        raise ValueError("read %s: %d clipped and %d aligned bases, the called sequence has %d" % (read.get("name", "?"), lead, aligned, n))
    i = np.cumsum(consumes_read) - consumes_read          # read-consuming columns before each column
    q = np.cumsum(consumes_ref) - consumes_ref
    keep = ops <= 1
    g = int(read["pos"]) + q[keep].astype(np.int64)
    idx = i[keep].astype(np.int64) + lead
    return g, (n - 1 - idx if read["reverse"] else idx)


def genome_bins(read, g0, g1):
    """int32 [bases of read["called"]], signal order: strand * (g1 - g0) + (g - g0) for the base of every '=' and 'X' column at a
    position g of the tile [g0, g1) -- miscalls are where modifications show, so 'X' counts, as in the pileup -- and -1 for every
    other base (inserted, clipped, outside the tile).  strand is 1 for a reverse-strand read."""
    out = np.full(len(read["called"]), -1, dtype=np.int32)
    g, idx = _columns(read)
    inside = (g >= g0) & (g < g1)
    out[idx[inside]] = (int(bool(read["reverse"])) * (g1 - g0) + (g[inside] - g0)).astype(np.int32)
    return out


def kmer_bins(read, genome, k):
    """int32 [bases], signal order: for the base of every '=' and 'X' column at g, the code (2 bits a base, first base highest) of
    the genome k-mer around g in the read's strand orientation, the base itself at index k // 2 of it: genome[g - k // 2 ..) for a
    forward read, the reverse complement of genome[g - (k - 1 - k // 2) ..) for a reverse one.  -1 where the window leaves the genome
    or holds a code above 3 (N, and the separators between contigs), and for every other base."""
    if not 1 <= k <= MAX_K:
        raise ValueError("k = %d outside 1 .. %d" % (k, MAX_K))
    codes = np.asarray(genome.codes, dtype=np.int64)
    out = np.full(len(read["called"]), -1, dtype=np.int32)
    g, idx = _columns(read)
    h = k // 2
    lo = g - (k - 1 - h if read["reverse"] else h)
    ok = (lo >= 0) & (lo + k <= len(codes))
    lo, idx = lo[ok], idx[ok]
    if len(lo) == 0:
        return out
    win = codes[lo[:, None] + np.arange(k)[None, :]]
    good = (win <= 3).all(axis=1)
    if read["reverse"]:
        win = 3 - win[:, ::-1]
    code = (win * (4 ** np.arange(k - 1, -1, -1, dtype=np.int64))[None, :]).sum(axis=1)
    out[idx[good]] = code[good].astype(np.int32)
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# the kernel
# ----------------------------------------------------------------------------------------------------------------------------
def workspace_size(reads, samples, bases, bins, want_levels=True):
    """chiron_signal_workspace_size (host-only)."""
    return _lib.sized("chiron_signal_workspace_size", int(reads), int(samples), int(bases), int(bins), int(bool(want_levels)))


def reduce_call(signals, starts, bins, n_bins, want_levels=True, device_id=0):
    """One chiron_signal_levels call.  signals: int16 arrays; starts: int32 [bases + 1] per read; bins: int32 [bases] per read.
    -> (planes int64 [PLANES, n_bins], [int32 levels per read] or None)."""
    if not len(signals) == len(starts) == len(bins):
        raise ValueError("%d signals, %d start arrays, %d bin arrays" % (len(signals), len(starts), len(bins)))
    reads = len(signals)
    sig = [np.ascontiguousarray(s, dtype=np.int16).reshape(-1) for s in signals]
    st = [np.ascontiguousarray(s, dtype=np.int32).reshape(-1) for s in starts]
    bn = [np.ascontiguousarray(b, dtype=np.int32).reshape(-1) for b in bins]
    for r in range(reads):
        if len(st[r]) != len(bn[r]) + 1:
            raise ValueError("read %d: %d start entries for %d bases, one more is needed" % (r, len(st[r]), len(bn[r])))
    sample_off, base_off = label._offsets([len(s) for s in sig]), label._offsets([len(b) for b in bn])
    n_bases = int(base_off[-1])
    samples = np.ascontiguousarray(np.concatenate(sig + [np.zeros(1, np.int16)]))
    start = np.ascontiguousarray(np.concatenate(st + [np.zeros(1, np.int32)]))
    bin_flat = np.ascontiguousarray(np.concatenate(bn + [np.zeros(1, np.int32)]))
    planes = np.zeros((PLANES, int(n_bins)), dtype=np.int64)
    level = np.zeros(max(n_bases, 1), dtype=np.int32)

    def split():
        return [level[base_off[r]:base_off[r + 1]].copy() for r in range(reads)] if want_levels else None
    if n_bases == 0 and n_bins == 0:
        return planes, split()
    lib, ws, stream = _lib.device_workspace(lambda: workspace_size(reads, int(sample_off[-1]), n_bases, n_bins, want_levels), device_id,
                                            "squiggle.reduce", "level kernel")
    _lib.check(lib.chiron_signal_levels(device_id, samples.ctypes.data, sample_off.ctypes.data, start.ctypes.data, base_off.ctypes.data,
                                        bin_flat.ctypes.data, reads, int(n_bins), 0, planes.ctypes.data if n_bins else None,
                                        level.ctypes.data if want_levels else None, ws.data_ptr(), stream))
    del ws
    return planes, split()


def _read_span(read):
    """(first genome position, one past the last) of the read's alignment."""
    ops = np.asarray(read["ops"], dtype=np.uint8)
    return int(read["pos"]), int(read["pos"]) + int((ops != 2).sum())


def plan_tiles(reads, total, budget_bytes, max_tile=MAX_BINS // 2):
    """Cut [0, total) into consecutive tiles so that one call's workspace -- the tile's 2 * (g1 - g0) bins and the reads handed to
    it -- stays within the budget; a tile of one position is always allowed.  A tile is handed every read that has a position in it:
    one that straddles an edge goes to both tiles, with a second copy of its samples.  The size is monotone in g1, so the largest
    tile that fits is found by bisection over the host-only size function, as pileup.plan_tiles does.
    -> [(g0, g1, indices of its reads, workspace bytes)]."""
    spans = np.array([_read_span(r) for r in reads], dtype=np.int64).reshape(-1, 2)
    n_samples = np.array([len(r["signal"]) for r in reads], dtype=np.int64)
    n_bases = np.array([len(r["called"]) for r in reads], dtype=np.int64)
    live = spans[:, 1] > spans[:, 0]

    def need(g0, g1):
        sel = live & (spans[:, 0] < g1) & (spans[:, 1] > g0)
        return workspace_size(int(sel.sum()), int(n_samples[sel].sum()), int(n_bases[sel].sum()), 2 * (g1 - g0)), sel

    tiles, g0 = [], 0
    while g0 < total:
        lo, hi = g0 + 1, min(total, g0 + max_tile)
        nbytes, sel = need(g0, hi)
        if nbytes > budget_bytes:
            while lo < hi:
                mid = (lo + hi + 1) // 2
                if need(g0, mid)[0] <= budget_bytes:
                    lo = mid
                else:
                    hi = mid - 1
            nbytes, sel = need(g0, lo)
            hi = lo
        tiles.append((g0, hi, np.nonzero(sel)[0].tolist(), nbytes))
        g0 = hi
    return tiles


def plan_read_batches(reads, n_bins, budget_bytes):
    """Consecutive runs of reads [(first, last + 1)] whose call with n_bins bins fits the budget, each the longest that does (the
    size grows with every read: bisection); a read that alone exceeds it gets a run of its own."""
    samples = label._offsets([len(r["signal"]) for r in reads])
    bases = label._offsets([len(r["called"]) for r in reads])
    n, runs, first = len(reads), [], 0
    while first < n:
        lo, hi = first + 1, n
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if workspace_size(mid - first, int(samples[mid] - samples[first]), int(bases[mid] - bases[first]), n_bins, False) <= budget_bytes:
                lo = mid
            else:
                hi = mid - 1
        runs.append((first, lo))
        first = lo
    return runs


def _reducer_of(reducer, device_id):
    if reducer is not None:
        return reducer
    import torch  # noqa: F401  before the planners load the library: torch's ROCm runtime has to come up first (_lib.py)

    def on_gpu(signals, starts, bins, n_bins):
        return reduce_call(signals, starts, bins, n_bins, True, device_id)
    return on_gpu


def levels(reads, genome, workspace_mb=4096, device_id=0, reducer=None, max_tile=MAX_BINS // 2):
    """The levels of the reads on the whole concatenated genome, tile by tile (plan_tiles; workspace_mb may be a fraction).
    reducer(signals, starts, bins, n_bins) -> (planes, levels per read) replaces the library call (the tests' reference).
    -> dict(planes int64 [2, PLANES, G], strand 0 forward and 1 reverse; levels [int32 [bases] per read, EMPTY for a base without a
    sample, None for a read that touches no position]; tiles)."""
    reducer = _reducer_of(reducer, device_id)
    reads = list(reads)
    total = len(genome.codes)
    planes = np.zeros((2, PLANES, total), dtype=np.int64)
    per_read = [None] * len(reads)
    tiles = plan_tiles(reads, total, int(workspace_mb * (1 << 20)), max_tile)
    for g0, g1, idx, _ in tiles:
        if not idx:
            continue
        got, lv = reducer([reads[i]["signal"] for i in idx], [reads[i]["starts"] for i in idx],
                          [genome_bins(reads[i], g0, g1) for i in idx], 2 * (g1 - g0))
        planes[:, :, g0:g1] = np.asarray(got, dtype=np.int64).reshape(PLANES, 2, g1 - g0).transpose(1, 0, 2)
        for k, i in enumerate(idx):
            if per_read[i] is None:                      # a read's levels do not depend on the tile
                per_read[i] = np.asarray(lv[k], dtype=np.int32)
    return {"planes": planes, "levels": per_read, "tiles": len(tiles)}


def kmer_levels(reads, genome, k, workspace_mb=4096, device_id=0, reducer=None):
    """The four planes per k-mer, int64 [PLANES, 4^k]: the same reduction with kmer_bins, in runs of reads planned against
    workspace_mb and summed."""
    reducer = _reducer_of(reducer, device_id)
    reads = list(reads)
    n_bins = 4 ** k
    planes = np.zeros((PLANES, n_bins), dtype=np.int64)
    for first, last in plan_read_batches(reads, n_bins, int(workspace_mb * (1 << 20))):
        part = reads[first:last]
        planes += np.asarray(reducer([r["signal"] for r in part], [r["starts"] for r in part], [kmer_bins(r, genome, k) for r in part], n_bins)[0],
                             dtype=np.int64)
    return planes


# ----------------------------------------------------------------------------------------------------------------------------
# refinement of the borders against a level table
# ----------------------------------------------------------------------------------------------------------------------------
def load_level_table(path, min_events=5):
    """The kmer_levels.tsv that `squiggle --kmer K` writes -> (K, int32 [4^K]): rint(mean * SCALE) for a k-mer with at least
    min_events events, UNKNOWN for every other."""
    with open(path) as f:
        rows = [ln.rstrip("\n").split("\t") for ln in f if ln.strip()]
    if not rows or tuple(rows[0]) != KMER_COLUMNS:
        raise ValueError("%s is not a kmer_levels.tsv: its first line is not %s" % (path, " ".join(KMER_COLUMNS)))
    if len(rows) < 2:
        raise ValueError("%s holds no k-mer" % path)
    k = len(rows[1][0])
    if not 1 <= k <= MAX_K:
        raise ValueError("%s: k-mers of %d bases, outside 1 .. %d" % (path, k, MAX_K))
    table = np.full(4 ** k, UNKNOWN, dtype=np.int32)
    for row in rows[1:]:
        if len(row) != len(KMER_COLUMNS) or len(row[0]) != k or set(row[0]) - set("ACGT"):
            raise ValueError("%s: a row of %d fields with the k-mer %r among %d-mers" % (path, len(row), row[0], k))
        if int(row[1]) >= min_events:
            code = 0
            for c in row[0]:
                code = code * 4 + "ACGT".index(c)
            table[code] = int(np.clip(np.rint(float(row[3]) * SCALE), -32767, 32767))
    return k, table


def table_of(kmer_planes, min_events=5):
    """The table load_level_table would read from kmer_lines(kmer_planes): without the file in between, and so without the
    rounding of its five decimals."""
    n, mean, _ = moments(kmer_planes)
    with np.errstate(invalid="ignore"):
        level = np.clip(np.rint(np.where(n > 0, mean, 0.0)), -32767, 32767).astype(np.int32)
    return np.where(n >= max(int(min_events), 1), level, UNKNOWN).astype(np.int32)


def expected_levels(read, genome, table, k):
    """int32 [bases], signal order: the table's level of every base's k-mer, the base itself at index k // 2 of it.  For the base of
    an '=' or 'X' column that is the genome k-mer of kmer_bins; for an inserted or clipped base it is the k-mer of the read's own
    called bases around it, in signal order.  UNKNOWN where the k-mer leaves the genome or the read, holds a code above 3, or has no
    entry in the table."""
    table = np.asarray(table, dtype=np.int32)
    if table.shape != (4 ** k,):
        raise ValueError("a table of %s entries for k = %d" % (table.shape, k))
    called = np.asarray(read["called"], dtype=np.int64)
    n, h = len(called), k // 2
    code = np.full(n, -1, dtype=np.int64)
    if n >= k:
        win = called[np.arange(n - k + 1)[:, None] + np.arange(k)[None, :]]
        own = (win * (4 ** np.arange(k - 1, -1, -1, dtype=np.int64))[None, :]).sum(axis=1)
        code[h:h + n - k + 1] = np.where((win <= 3).all(axis=1), own, -1)
    _, idx = _columns(read)
    code[idx] = kmer_bins(read, genome, k)[idx]
    return np.where(code >= 0, table[np.maximum(code, 0)], UNKNOWN).astype(np.int32)


def refine_items(levels):
    """[(first base, one past the last)] of the maximal runs of bases whose level is not UNKNOWN."""
    known = np.concatenate([[False], np.asarray(levels) != UNKNOWN, [False]])
    edges = np.flatnonzero(known[1:] != known[:-1])
    return [(int(a), int(b)) for a, b in zip(edges[0::2], edges[1::2])]


def refine_workspace_size(items, samples, bases):
    """chiron_signal_refine_workspace_size (host-only)."""
    return _lib.sized("chiron_signal_refine_workspace_size", int(items), int(samples), int(bases))


def refine_call(signals, levels, starts, device_id=0):
    """One chiron_signal_refine call.  Per item: its int16 samples, its int32 levels [L] and its int32 starts [L + 1], relative to
    its first sample.  -> ([int32 refined starts per item], int64 costs [items], INFEASIBLE for an item that keeps its starts)."""
    if not len(signals) == len(levels) == len(starts):
        raise ValueError("%d signals, %d level arrays, %d start arrays" % (len(signals), len(levels), len(starts)))
    items = len(signals)
    sig = [np.ascontiguousarray(s, dtype=np.int16).reshape(-1) for s in signals]
    lv = [np.ascontiguousarray(e, dtype=np.int32).reshape(-1) for e in levels]
    st = [np.ascontiguousarray(s, dtype=np.int32).reshape(-1) for s in starts]
    for i in range(items):
        if len(st[i]) != len(lv[i]) + 1:
            raise ValueError("item %d: %d start entries for %d bases, one more is needed" % (i, len(st[i]), len(lv[i])))
    sample_off, base_off = label._offsets([len(s) for s in sig]), label._offsets([len(e) for e in lv])
    n_bases = int(base_off[-1])
    samples = np.ascontiguousarray(np.concatenate(sig + [np.zeros(1, np.int16)]))
    level = np.ascontiguousarray(np.concatenate(lv + [np.zeros(1, np.int32)]))
    start = np.ascontiguousarray(np.concatenate(st + [np.zeros(1, np.int32)]))
    out = np.zeros(n_bases + items + 1, dtype=np.int32)
    cost = np.zeros(max(items, 1), dtype=np.int64)

    def split():
        return [out[base_off[i] + i:base_off[i + 1] + i + 1].copy() for i in range(items)], cost[:items].copy()
    args = (samples.ctypes.data, sample_off.ctypes.data, level.ctypes.data, start.ctypes.data, base_off.ctypes.data, items, 0, out.ctypes.data,
            cost.ctypes.data)
    if n_bases == 0:                                    # nothing to move: the library touches no device
        _lib.check(_lib.load().chiron_signal_refine(device_id, *args, None, None))
        return split()
    lib, ws, stream = _lib.device_workspace(lambda: refine_workspace_size(items, int(sample_off[-1]), n_bases), device_id, "squiggle.refine",
                                            "refine kernel")
    _lib.check(lib.chiron_signal_refine(device_id, *args, ws.data_ptr(), stream))
    del ws
    return split()


def plan_refine_batches(counts, budget_bytes):
    """counts: (items, samples, bases) per read.  Consecutive runs of reads [(first, last + 1)] whose call fits the budget, each the
    longest that does (the size grows with every read: bisection); a read that alone exceeds it gets a run of its own."""
    c = np.concatenate([np.zeros((1, 3), np.int64), np.cumsum(np.asarray(counts, dtype=np.int64).reshape(-1, 3), axis=0)])
    n, runs, first = len(c) - 1, [], 0
    while first < n:
        lo, hi = first + 1, n
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if refine_workspace_size(*(c[mid] - c[first]).tolist()) <= budget_bytes:
                lo = mid
            else:
                hi = mid - 1
        runs.append((first, lo))
        first = lo
    return runs


def refine(reads, genome, table, k, workspace_mb=4096, device_id=0, refiner=None):
    """Moves the borders of every read to where its samples meet the table's levels and replaces its `starts`.  Per read the items
    are the runs of refine_items(expected_levels(...)); a border outside them, and an item the DP finds infeasible, stays.  The
    calls are planned against workspace_mb with the host-only size function.  refiner(signals, levels, starts) -> (starts, costs)
    replaces the library call (the tests' reference).
    -> dict(items, bases in them, infeasible items, borders inside items, moved of them, mean_move = mean |move| in samples over
    those borders, cost of the feasible items, calls)."""
    if refiner is None:
        import torch  # noqa: F401  before the planner loads the library: torch's ROCm runtime has to come up first (_lib.py)

        def refiner(signals, levels, starts):
            return refine_call(signals, levels, starts, device_id)
    reads = list(reads)
    per_read = []
    for r in reads:
        lv = expected_levels(r, genome, table, k)
        st = np.asarray(r["starts"], dtype=np.int32)
        runs = refine_items(lv)
        per_read.append((lv, runs, (len(runs), sum(int(st[b] - st[a]) for a, b in runs), sum(b - a for a, b in runs))))
    out = dict.fromkeys(REFINE_COUNTS, 0)
    moved_by = 0
    batches = plan_refine_batches([c for _, _, c in per_read], int(workspace_mb * (1 << 20))) if reads else []
    for first, last in batches:
        signals, levels_, starts, where = [], [], [], []
        for i in range(first, last):
            lv, runs, _ = per_read[i]
            st = np.asarray(reads[i]["starts"], dtype=np.int32)
            for a, b in runs:
                signals.append(reads[i]["signal"][st[a]:st[b]])
                levels_.append(lv[a:b])
                starts.append(st[a:b + 1] - st[a])
                where.append((i, a, b))
        if not where:
            continue
        got, cost = refiner(signals, levels_, starts)
        new = {}
        for (i, a, b), s_in, s, c in zip(where, starts, got, cost):
            out["items"] += 1
            out["bases"] += b - a
            if int(c) == INFEASIBLE:
                out["infeasible"] += 1
                continue
            st = new.setdefault(i, np.array(reads[i]["starts"], dtype=np.int32))
            st[a:b + 1] = st[a] + np.asarray(s, dtype=np.int32)
            move = np.abs(np.asarray(s, dtype=np.int64) - s_in)[1:-1]
            out["borders"] += len(move)
            out["moved"] += int((move > 0).sum())
            moved_by += int(move.sum())
            out["cost"] += int(c)
        for i, st in new.items():
            reads[i]["starts"] = st
    out["mean_move"] = moved_by / out["borders"] if out["borders"] else 0.0
    out["calls"] = len(batches)
    return out


_refine_reads = refine                   # sample() has an argument of that name


# ----------------------------------------------------------------------------------------------------------------------------
# statistics
# ----------------------------------------------------------------------------------------------------------------------------
def moments(planes):
    """(events, mean, sample variance) per bin of planes [PLANES, ...], float64: mean = sum / n and variance = (sq - sum^2 / n) /
    (n - 1), nan where n is too small for them."""
    p = np.asarray(planes)
    n, s, q = (p[k].astype(np.float64) for k in (EVENTS, SUM, SQ))
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(n > 0, s / n, np.nan)
        var = np.where(n > 1, (q - s * s / n) / (n - 1), np.nan)
    return n, mean, var


def compare(a, b, min_events=5):
    """Two samples' planes [PLANES, ...] of one shape, bin by bin, in float64.  -> dict of arrays of that shape: keep (at least
    max(min_events, 2) events in both), events_a, mean_a, var_a, events_b, mean_b, var_b, t = (mean_a - mean_b) / sqrt(var_a / n_a +
    var_b / n_b) (Welch), df = (var_a / n_a + var_b / n_b)^2 / ((var_a / n_a)^2 / (n_a - 1) + (var_b / n_b)^2 / (n_b - 1))
    (Welch-Satterthwaite) and effect = (mean_a - mean_b) / SCALE, in MAD units.  Where keep is false the statistics are nan.  Two
    bins without any spread give t = +-inf, or 0 when their means agree, and df = nan.  No p-values: no dependency is added."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.shape[0] != PLANES:
        raise ValueError("planes of shapes %s and %s" % (a.shape, b.shape))
    na, ma, va = moments(a)
    nb, mb, vb = moments(b)
    floor = max(int(min_events), 2)
    keep = (na >= floor) & (nb >= floor)
    with np.errstate(divide="ignore", invalid="ignore"):
        ea, eb = va / na, vb / nb
        diff = ma - mb
        t = np.where(diff == 0, 0.0, diff / np.sqrt(ea + eb))
        df = (ea + eb) ** 2 / (ea * ea / (na - 1) + eb * eb / (nb - 1))
    out = {"events_a": na, "mean_a": ma, "var_a": va, "events_b": nb, "mean_b": mb, "var_b": vb, "t": t, "df": df, "effect": diff / SCALE}
    for key in ("mean_a", "var_a", "mean_b", "var_b", "t", "df", "effect"):
        out[key] = np.where(keep, out[key], np.nan)
    out["keep"] = keep
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# the pipeline
# ----------------------------------------------------------------------------------------------------------------------------
def prepare(reads, segment_len, ratio, mode="mad", band=label.BAND0, max_band=label.MAX_BAND, workspace_mb=4096, device_id=0,
            frame_aligner=None):
    """reads: polish.py's dicts with `logits`, `seq_lens` (label.read_frames) and `raw` (the samples as read).  Aligns every usable
    read's frames to its called bases (polish.align_frames) and gives it `signal` and `starts`.  -> (the reads kept, drops by
    reason)."""
    drops = {reason: 0 for reason in READ_DROPS}
    usable = []
    for r in reads:
        if r.get("logits") is None:
            drops["no_signal"] += 1
        elif r["logits"].shape[0] == 0 or len(r["called"]) == 0:
            drops["no_frames"] += 1
        elif np.any(np.asarray(r["called"]) > 3):
            drops["outside_acgt"] += 1
        else:
            sig = normalise(r["raw"], mode)
            if sig is None:
                drops["flat_signal"] += 1
            else:
                usable.append(dict(r, signal=sig))
    starts, status = polish.align_frames(usable, band, max_band, workspace_mb, device_id, frame_aligner)
    kept = []
    for r, st, s in zip(usable, status, starts):
        if st != 0:
            drops[label.STATUS_NAMES[int(st)]] += 1
        else:
            r["starts"] = base_starts(s[:-1], r["seq_lens"], segment_len, ratio, len(r["signal"]))
            kept.append(r)
    return kept, drops


def sample(reads, genome, segment_len, ratio, mode="mad", band=label.BAND0, max_band=label.MAX_BAND, workspace_mb=4096, device_id=0,
           frame_aligner=None, reducer=None, kmer=0, refine=None, refiner=None):
    """One sample from loaded reads to planes: prepare, with refine = (table, k) the refinement of the borders (`refine` above;
    refiner= is its hook), levels and, with kmer > 0, kmer_levels.
    -> dict(reads kept, planes, levels, tiles, kmer_planes or None, report); the report has a `refine` section when refined."""
    kept, drops = prepare(reads, segment_len, ratio, mode, band, max_band, workspace_mb, device_id, frame_aligner)
    refined = _refine_reads(kept, genome, refine[0], refine[1], workspace_mb, device_id, refiner) if refine is not None else None
    got = levels(kept, genome, workspace_mb, device_id, reducer)
    report = {"reads": {"total": len(reads), "used": len(kept), "dropped": drops}, "tiles": got["tiles"],
              "bases": int(sum(len(r["called"]) for r in kept)), "samples": int(sum(len(r["signal"]) for r in kept)),
              "events": int(got["planes"][:, EVENTS].sum())}
    if refined is not None:
        report["refine"] = refined
    return {"reads": kept, "planes": got["planes"], "levels": got["levels"], "tiles": got["tiles"], "report": report,
            "kmer_planes": kmer_levels(kept, genome, kmer, workspace_mb, device_id, reducer) if kmer else None}


# ----------------------------------------------------------------------------------------------------------------------------
# files and the command
# ----------------------------------------------------------------------------------------------------------------------------
def _positions(genome, mask):
    """(g, contig name, 1-based position, genome base) of the concatenated positions where mask holds, separators left out."""
    for g in np.flatnonzero(mask):
        c = genome.contig_of(int(g))
        at = int(g) - int(genome.starts[c])
        if at < int(genome.lengths[c]):
            yield int(g), genome.names[c], at + 1, "ACGTN"[int(genome.codes[g])]


def _stats(planes, at):
    """events, mean dwell, mean and sd of the level at one bin, the levels in MAD units."""
    n = int(planes[EVENTS][at])
    _, mean, var = moments(planes[:, at:at + 1])
    return n, float(planes[DWELL][at]) / n, float(mean[0]) / SCALE, (float(np.sqrt(max(var[0], 0.0))) / SCALE if n > 1 else float("nan"))


def level_lines(planes, genome):
    """levels.tsv: one row per position and strand with an event; `ref` is the genome's base there, on either strand."""
    lines = ["\t".join(LEVEL_COLUMNS) + "\n"]
    for g, contig, pos, ref in _positions(genome, (planes[:, EVENTS] > 0).any(axis=0)):
        for strand in (0, 1):
            if planes[strand, EVENTS, g] > 0:
                n, dwell, mean, sd = _stats(planes[strand], g)
                lines.append("%s\t%d\t%s\t%s\t%d\t%.3f\t%.5f\t%.5f\n" % (contig, pos, "+-"[strand], ref, n, dwell, mean, sd))
    return lines


def compare_lines(result, genome):
    """compare.tsv: one row per position and strand that `compare` kept; sample a is the input, b the control."""
    lines = ["\t".join(COMPARE_COLUMNS) + "\n"]
    for g, contig, pos, ref in _positions(genome, result["keep"].any(axis=0)):
        for strand in (0, 1):
            if result["keep"][strand, g]:
                v = {k: result[k][strand, g] for k in result}
                lines.append("%s\t%d\t%s\t%s\t%d\t%.5f\t%.5f\t%d\t%.5f\t%.5f\t%.5f\t%.3f\t%.5f\n" % (
                    contig, pos, "+-"[strand], ref, v["events_a"], v["mean_a"] / SCALE, np.sqrt(v["var_a"]) / SCALE, v["events_b"],
                    v["mean_b"] / SCALE, np.sqrt(v["var_b"]) / SCALE, v["t"], v["df"], v["effect"]))
    return lines


def kmer_lines(planes, k):
    """kmer_levels.tsv: one row per k-mer with an event."""
    lines = ["\t".join(KMER_COLUMNS) + "\n"]
    for code in np.flatnonzero(planes[EVENTS] > 0):
        n, dwell, mean, sd = _stats(planes, int(code))
        lines.append("%s\t%d\t%.3f\t%.5f\t%.5f\n" % ("".join("ACGT"[(int(code) >> (2 * (k - 1 - j))) & 3] for j in range(k)), n, dwell, mean, sd))
    return lines


def event_lines(read, level, genome):
    """events/<read>.tsv: one row per base in signal order: start, length, level ('.' without a sample), contig and 1-based pos, or
    '.' for a base that is on no position."""
    g, idx = _columns(read)
    where = np.full(len(read["called"]), -1, dtype=np.int64)
    where[idx] = g
    lines = ["\t".join(EVENT_COLUMNS) + "\n"]
    for n in range(len(read["called"])):
        contig, pos = ".", "."
        if where[n] >= 0:
            c = genome.contig_of(int(where[n]))
            contig, pos = genome.names[c], str(int(where[n]) - int(genome.starts[c]) + 1)
        s, e = int(read["starts"][n]), int(read["starts"][n + 1])
        lines.append("%d\t%d\t%s\t%s\t%s\n" % (s, e - s, "." if level is None or level[n] == EMPTY else str(int(level[n])), contig, pos))
    return lines


def _sam_of(path):
    if os.path.isdir(path):
        sam = os.path.join(path, "mapped.sam")
        if not os.path.exists(sam):
            raise ValueError("%s has no mapped.sam: run `chiron map` with --cigar, which writes it" % path)
        return sam
    return path


def load_sample(sam, signal_dir, genome, engine, batch_size, min_mapq=0, dropped=None):
    """The reads of one sample as `prepare` takes them: polish.reads_from_sam, and for every read with a .signal file its samples
    (`raw`, as `call` reads them), its frame logits and the windows' frame counts (label.read_frames).  min_mapq: as for
    pileup.read_sam; the number of records it drops is appended to `dropped`."""
    from . import signal_io
    source, reads = polish.reads_from_sam(sam, genome, min_mapq)
    if dropped is not None:
        dropped.append(source["low_mapq"])
    signals = dict(label.find_signals(signal_dir))
    for r in reads:
        if r["name"] in signals:
            r["raw"] = np.asarray(signal_io.read_signal(signals[r["name"]], normalize=signal_io.SIG_NORM))
            r["logits"], r["seq_lens"] = label.read_frames(engine, r["raw"], batch_size)
    return reads


def squiggle_command(args):
    """The `squiggle` command: mapped.sam + the reads' signals + the genome + a model -> levels.tsv, squiggle_report.json and, as
    asked, compare.tsv, kmer_levels.tsv and events/<read>.tsv; returns the report."""
    import torch  # noqa: F401  the later stages take their workspaces from torch: its runtime has to be up before the engine loads the library (_lib.py)
    from . import map as map_mod, model as model_mod
    from .engine import Engine
    if args.kmer and not 1 <= args.kmer <= MAX_K:
        raise ValueError("--kmer %d outside 1 .. %d" % (args.kmer, MAX_K))
    if bool(args.control) != bool(args.control_signal):
        raise ValueError("--control and --control-signal go together")
    refine_path = getattr(args, "refine", None)
    table = None
    if refine_path:
        table = load_level_table(refine_path, getattr(args, "refine_min_events", 5))[::-1]            # (table, k): read before the engine starts
    sam = _sam_of(args.input)
    control_sam = _sam_of(args.control) if args.control else None
    genome = map_mod.load_genome(args.genome)
    spec, weights, _ = model_mod.load_model(args.model, allow_synthetic=args.synthetic_weights)
    with Engine(spec, weights, max_batch=args.batch_size, segment_len=args.segment_len, device_id=args.device, dtype=args.dtype) as eng:
        ratio = eng.ratio
        min_mapq, low = getattr(args, "min_mapq", 0), []
        loaded = load_sample(sam, args.signal, genome, eng, args.batch_size, min_mapq, low)
        control = load_sample(control_sam, args.control_signal, genome, eng, args.batch_size, min_mapq, low) if control_sam else None
    kw = dict(segment_len=args.segment_len, ratio=ratio, mode=args.normalize, band=args.band, max_band=args.max_band,
              workspace_mb=args.workspace_mb, device_id=args.device, refine=table)
    a = sample(loaded, genome, kmer=args.kmer or 0, **kw)
    os.makedirs(args.output, exist_ok=True)
    files = ["levels.tsv"]
    with open(os.path.join(args.output, "levels.tsv"), "w") as f:
        f.write("".join(level_lines(a["planes"], genome)))
    report = {"input": args.input, "sam": sam, "signal": args.signal, "genome": args.genome, "model": args.model, "segment_len": args.segment_len,
              "dtype": args.dtype, "normalize": args.normalize, "scale": SCALE, "min_events": args.min_events, "kmer": args.kmer or 0,
              "band": args.band, "max_band": args.max_band, "workspace_mb": args.workspace_mb, "ratio": ratio}
    report.update(a["report"])
    if table is not None:                                     # sample() put the counts there; the table's own facts join them
        report["refine"] = dict(report["refine"], table=refine_path, k=table[1], min_events=getattr(args, "refine_min_events", 5),
                                kmers_known=int((table[0] != UNKNOWN).sum()))
    if min_mapq > 0:
        report.update({"min_mapq": min_mapq, "low_mapq": low[0]})
    if control is not None:
        b = sample(control, genome, **kw)
        result = compare(a["planes"].transpose(1, 0, 2), b["planes"].transpose(1, 0, 2), args.min_events)
        with open(os.path.join(args.output, "compare.tsv"), "w") as f:
            f.write("".join(compare_lines(result, genome)))
        files.append("compare.tsv")
        report["control"] = dict(b["report"], sam=control_sam, signal=args.control_signal, **({"low_mapq": low[1]} if min_mapq > 0 else {}))
        report["compared"] = int(result["keep"].sum())
    if args.kmer:
        with open(os.path.join(args.output, "kmer_levels.tsv"), "w") as f:
            f.write("".join(kmer_lines(a["kmer_planes"], args.kmer)))
        files.append("kmer_levels.tsv")
        report["kmers_seen"] = int((a["kmer_planes"][EVENTS] > 0).sum())
    if args.events:
        os.makedirs(os.path.join(args.output, "events"), exist_ok=True)
        for r, lv in zip(a["reads"], a["levels"]):
            with open(os.path.join(args.output, "events", r["name"] + ".tsv"), "w") as f:
                f.write("".join(event_lines(r, lv, genome)))
        report["event_files"] = len(a["reads"])
    report["files"] = files
    with open(os.path.join(args.output, "squiggle_report.json"), "w") as f:
        json.dump(report, f, indent=1)
    return report
