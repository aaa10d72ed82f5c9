"""The definition of chiron_signal_levels (include/chiron_amd.h) restated twice, sharing no code with the library or with each
other: `reduce` in plain Python integers, one base at a time, and `reduce_numpy` / `reduce_flat` with np.add.reduceat and np.add.at.
Both have the signature of chiron_amd.squiggle's reducer= hook.  Also the brute-force walks of the alignment columns that
genome_bins and kmer_bins are held to, and Welch's statistics from explicit lists of levels."""
import math

import numpy as np

PLANES = 4
EMPTY = -(1 << 31)


def level_of(samples):
    """floor((2 s + c) / (2 c)) in Python integers, whose // is floor division."""
    c = len(samples)
    s = sum(int(v) for v in samples)
    return (2 * s + c) // (2 * c)


def reduce(signals, starts, bins, n_bins):
    """-> (planes int64 [4, n_bins], [int32 levels per read]), one base at a time."""
    planes = [[0] * n_bins for _ in range(PLANES)]
    levels = []
    for sig, st, bn in zip(signals, starts, bins):
        assert len(st) == len(bn) + 1
        out = []
        for n in range(len(bn)):
            a, z = int(st[n]), int(st[n + 1])
            assert 0 <= a <= z <= len(sig)
            if z == a:
                out.append(EMPTY)
                continue
            lv = level_of(sig[a:z])
            out.append(lv)
            b = int(bn[n])
            assert -1 <= b < n_bins
            if b >= 0:
                planes[0][b] += 1
                planes[1][b] += z - a
                planes[2][b] += lv
                planes[3][b] += lv * lv
        levels.append(np.array(out, dtype=np.int32))
    return np.array(planes, dtype=np.int64).reshape(PLANES, n_bins), levels


def reduce_flat(samples, sample_off, start, base_off, bins, n_bins):
    """The library's own flat arrays (sample_off[0] = base_off[0] = 0) -> (planes, levels int32 [bases]) with np.add.reduceat over the
    interleaved span borders and np.add.at into the planes.  The even results of reduceat are the spans' sums; a border pair (end of
    one span, start of the next) sums the samples nobody owns, or repeats an element when the two coincide: the odd results are
    dropped either way."""
    sample_off, base_off = np.asarray(sample_off, dtype=np.int64), np.asarray(base_off, dtype=np.int64)
    reads = len(base_off) - 1
    n_bases = int(base_off[-1])
    start = np.asarray(start, dtype=np.int64)[:n_bases + reads]
    lens = np.diff(base_off)
    read_of = np.repeat(np.arange(reads), lens)
    at = np.arange(n_bases) + read_of                            # the base's entry of start; the next entry is its end
    first = start[at] + sample_off[read_of]
    end = start[at + 1] + sample_off[read_of]
    count = end - first
    level = np.full(n_bases, EMPTY, dtype=np.int64)
    some = count > 0
    if some.any():
        borders = np.stack([first[some], end[some]], axis=1).reshape(-1)
        padded = np.concatenate([np.asarray(samples, dtype=np.int16)[:int(sample_off[-1])], np.zeros(1, np.int16)])   # an end may be the length
        s = np.add.reduceat(padded, borders, dtype=np.int64)[0::2]
        level[some] = np.floor_divide(2 * s + count[some], 2 * count[some])
    planes = np.zeros((PLANES, n_bins), dtype=np.int64)
    b = np.asarray(bins, dtype=np.int64)[:n_bases]
    hit = some & (b >= 0)
    np.add.at(planes[0], b[hit], 1)
    np.add.at(planes[1], b[hit], count[hit])
    np.add.at(planes[2], b[hit], level[hit])
    np.add.at(planes[3], b[hit], level[hit] * level[hit])
    return planes, level.astype(np.int32)


def flatten(signals, starts, bins):
    """The arrays chiron_signal_levels takes, each with one pad element: (samples, sample_off, start, base_off, bin)."""
    off = lambda lens: np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.int64)
    cat = lambda parts, dtype: np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=dtype).reshape(-1) for p in parts] + [np.zeros(1, dtype)]))
    return (cat(signals, np.int16), off([len(s) for s in signals]), cat(starts, np.int32), off([len(b) for b in bins]), cat(bins, np.int32))


def reduce_numpy(signals, starts, bins, n_bins):
    samples, sample_off, start, base_off, bin_flat = flatten(signals, starts, bins)
    planes, level = reduce_flat(samples, sample_off, start, base_off, bin_flat, n_bins)
    return planes, [level[base_off[r]:base_off[r + 1]].copy() for r in range(len(signals))]


# ----------------------------------------------------------------------------------------------------------------------------
# the columns of an alignment, one at a time
# ----------------------------------------------------------------------------------------------------------------------------
def walk_columns(read):
    """[(genome position, index into read["called"] in signal order)] of the '=' and 'X' columns."""
    n = len(read["called"])
    g, i, out = int(read["pos"]), int(read["lead"]), []
    for op in read["ops"]:
        if op in (0, 1):
            out.append((g, n - 1 - i if read["reverse"] else i))
        if op != 3:
            i += 1
        if op != 2:
            g += 1
    return out


def genome_bins(read, g0, g1):
    out = [-1] * len(read["called"])
    for g, idx in walk_columns(read):
        if g0 <= g < g1:
            out[idx] = (1 if read["reverse"] else 0) * (g1 - g0) + g - g0
    return np.array(out, dtype=np.int32)


def kmer_bins(read, codes, k):
    out = [-1] * len(read["called"])
    h = k // 2
    for g, idx in walk_columns(read):
        if read["reverse"]:                 # the read saw the complement strand, backwards: the base at g stays at index h
            window = [g + h - j for j in range(k)]
            letters = [3 - int(codes[p]) if 0 <= p < len(codes) and codes[p] <= 3 else None for p in window]
        else:
            window = [g - h + j for j in range(k)]
            letters = [int(codes[p]) if 0 <= p < len(codes) and codes[p] <= 3 else None for p in window]
        if None not in letters:
            code = 0
            for c in letters:
                code = code * 4 + c
            out[idx] = code
    return np.array(out, dtype=np.int32)


# ----------------------------------------------------------------------------------------------------------------------------
# Welch from the levels themselves
# ----------------------------------------------------------------------------------------------------------------------------
def welch(xa, xb, scale):
    """(mean_a, var_a, mean_b, var_b, t, df, effect) of two lists of levels, each of at least two."""
    na, nb = len(xa), len(xb)
    ma, mb = math.fsum(xa) / na, math.fsum(xb) / nb
    va = math.fsum((x - ma) ** 2 for x in xa) / (na - 1)
    vb = math.fsum((x - mb) ** 2 for x in xb) / (nb - 1)
    ea, eb = va / na, vb / nb
    t = (ma - mb) / math.sqrt(ea + eb)
    df = (ea + eb) ** 2 / (ea * ea / (na - 1) + eb * eb / (nb - 1))
    return ma, va, mb, vb, t, df, (ma - mb) / scale
