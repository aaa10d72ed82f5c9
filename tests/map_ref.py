"""Reference for the read mapper's alignment (chiron_align_infix / chiron_amd.map): what (E, M, s, e) of a read and a window IS,
computed the slow and obvious way.  Shares no code with the package.

Semantics: over every substring win[s:e) and every unit-cost global alignment of the read against it, the smallest tuple in the
order: smallest E, then largest M, then smallest s, then smallest e.  Bases compare as in assess_ref (case-insensitive, U is T,
anything else matches nothing).

brute_force: every (s, e), the global (E, M) of assess_ref.full_table, picked by the stated order.
full_table: a full-table numpy DP of one key per cell, key = E * 2^40 - M * 2^20 + s (row 0 is free: cell (0, j) = j), row by row
    as assess_ref.full_table sweeps; the horizontal dependency of a row is a running minimum of A[j] - j * 2^40, which is exact
    because a step to the right adds 2^40 and leaves M and s alone.
banded / doubling: the kernel's band scheme in plain Python, anti-diagonal by anti-diagonal in one array indexed by the diagonal.
"""
import numpy as np

import assess_ref

G = 1 << 40
MT = 1 << 20
INF = 1 << 62


def unpack(key):
    E = (key + (G >> 1)) >> 40
    rem = E * G - key
    M = (rem + MT - 1) >> 20
    return int(E), int(M), int(M * MT - rem)


def brute_force(read, win):
    best = None
    for s in range(len(win) + 1):
        for e in range(s, len(win) + 1):
            E, M = assess_ref.full_table(read, win[s:e])
            cand = (E, -M, s, e)
            if best is None or cand < best:
                best = cand
    return best[0], -best[1], best[2], best[3]


def full_table(read, win):
    """(E, M, s, e) of str read against the best substring of str win."""
    a, b = assess_ref.canon(read), assess_ref.canon(win)
    n, m = len(a), len(b)
    j = np.arange(m + 1, dtype=np.int64)
    row = j.copy()
    for i in range(1, n + 1):
        diag = row[:-1] + np.where(assess_ref._match_row(a[i - 1], b), -MT, G)
        up = row[1:] + G
        A = np.empty(m + 1, np.int64)
        A[0] = i * G
        A[1:] = np.minimum(diag, up)
        row = np.minimum.accumulate(A - j * G) + j * G
    e = int(np.argmin(row))                       # the first minimum: the smallest e
    return unpack(int(row[e])) + (e,)


def band_edges(n, m, w):
    return max(min(0, m - n) - w, -n), min(max(0, m - n) + w, m)


def banded(read, win, w):
    """-> (E, M, s, e, certified): certified when E <= w or the band is the whole table."""
    n, m = len(read), len(win)
    dlo, dhi = band_edges(n, m, w)
    row = [INF] * (dhi - dlo + 1)
    for k in range(n + m + 1):
        lo = max(dlo, -k, k - 2 * n)
        hi = min(dhi, k, 2 * m - k)
        lo += (lo + k) & 1
        for d in range(lo, hi + 1, 2):
            i, j = (k - d) // 2, (k + d) // 2
            s = d - dlo
            if i == 0:
                best = j
            else:
                best = INF
                if j > 0:
                    best = row[s] + (-MT if assess_ref.is_match(read[i - 1], win[j - 1]) else G)
                if d < dhi:
                    best = min(best, row[s + 1] + G)
                if j > 0 and d > dlo:
                    best = min(best, row[s - 1] + G)
            row[s] = best
    key, e = min((row[d - dlo], n + d) for d in range(dlo, m - n + 1))
    E, M, s = unpack(key)
    return E, M, s, e, (dlo == -n and dhi == m) or E <= w


def doubling(read, win, band0):
    """The kernel's loop: w = band0, doubled until the result is certified.  band0 = 0: the full table, band 0.
    -> (E, M, s, e, accepted w)."""
    if band0 == 0:
        return banded(read, win, len(read) + len(win))[:4] + (0,)
    w = band0
    while True:
        E, M, s, e, ok = banded(read, win, w)
        if ok:
            return E, M, s, e, w
        w *= 2


def expected_band(n, m, E, band0):
    """The half-width the kernel stops at, from the true E: the banded E is never below the true one and equals it once
    E <= w, so the loop stops at the first w of band0 * 2^k with E <= w or with the whole table inside the band."""
    if band0 == 0:
        return 0
    w = band0
    while not (E <= w or band_edges(n, m, w) == (-n, m)):
        w *= 2
    return w


def as_str(seq):
    """Codes 0..4 (what the package hands its aligner) back to letters; a str passes through."""
    return seq if isinstance(seq, str) else "".join("ACGTN"[c] for c in seq)


def infix_rows(reads, wins, band0, dtype):
    """The package's aligner interface on the reference: rows of `dtype` (edit, match, start, end, band)."""
    out = np.zeros(len(reads), dtype=dtype)
    for k, (a, b) in enumerate(zip(reads, wins)):
        a, b = as_str(a), as_str(b)
        E, M, s, e = full_table(a, b)
        out[k] = (E, M, s, e, expected_band(len(a), len(b), E, band0))
    return out


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTN", "TGCAN"))


def planted_case(seed, genome_len=200000, reads=24, unrelated=2, rate=0.10):
    """The end-to-end case: a two-contig genome, reads cut from it and mutated (every other one reverse-complemented), and
    unrelated reads.  -> (contigs [(name, seq)], reads {name: seq}, truth {name: (contig, start, end, strand, edits applied)})."""
    rng = np.random.default_rng(seed)
    cut = genome_len * 2 // 5
    g = assess_ref.random_seq(genome_len, rng)
    contigs = [("ctgA", g[:cut]), ("ctgB", g[cut:])]
    out, truth = {}, {}
    for k in range(reads):
        name, seq = contigs[k % 2]
        n = int(rng.integers(400, 1501))
        start = int(rng.integers(0, len(seq) - n))
        piece, edits = mutate_counted(seq[start:start + n], rate, rng)
        strand = "reverse" if k % 2 == (k // 2) % 2 else "forward"
        out["read%02d" % k] = revcomp(piece) if strand == "reverse" else piece
        truth["read%02d" % k] = (name, start, start + n, strand, edits)
    for k in range(unrelated):
        out["noise%d" % k] = assess_ref.random_seq(int(rng.integers(400, 1501)), rng)
    return contigs, out, truth


def mutate_counted(seq, rate, rng):
    """assess_ref.mutate that also counts the edits it applied."""
    out, edits = [], 0
    for ch in seq:
        r = rng.random()
        if r < rate / 3:
            edits += 1
            continue
        if r < 2 * rate / 3:
            out.append("ACGT"[rng.integers(4)])
            edits += 1
            continue
        out.append(ch)
        if r < rate:
            out.append("ACGT"[rng.integers(4)])
            edits += 1
    return "".join(out), edits
