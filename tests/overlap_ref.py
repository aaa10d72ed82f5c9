"""Reference for the read-to-read overlap alignment (chiron_align_overlap / chiron_amd.overlap): what (cost, M, s, e) of two reads
and a band of diagonals IS, stated three times.  Shares no code with the package.

Semantics: read a (n codes) and read b (m codes), codes 0..3 bases and 4 matching nothing.  A path through the (n+1) x (m+1) table
takes diagonal, down and right moves, starts on row 0 or column 0, ends on row n or column m, and every cell of it lies on a
diagonal d = j - i of [dlo, dhi] (clipped to [-n, m]).  cost = 2 E - M, M the diagonal moves on equal codes below 4 and E every
other move.  A start (0, j) is s = j + n and a start (i, 0) is s = n - i; an end (n, j) is e = j and an end (i, m) is e = m - i + n.
The result is the smallest (cost, -M, s, e) over all paths in the band.

recurrence: the table of the lexicographic minimum of (cost, -M, s) per cell, as tuples, cell by cell in plain Python.
brute_force_all: every path of an (n, m) table enumerated once with its start, end, gap count, diagonal cells and diagonal range;
    every pair of strings and every band is then a masked minimum over the paths.  Nothing of a recurrence is in it.
rows: numpy, many pairs at once, row by row on arrays indexed by the diagonal, one int64 key a cell
    (cost * 2^40 - M * 2^20 + start diagonal + 2^17); the dependency along a row is a running minimum, which is exact because a
    step to the right adds 2^41 and leaves M and the start alone.  Fast enough for the planted case.
"""
import numpy as np

G = 1 << 40
MT = 1 << 20
INF = 1 << 62
BIAS = 1 << 17
CHUNK = 48
DTYPE = np.dtype([("cost", np.int32), ("match", np.int32), ("start", np.int32), ("end", np.int32)])


def codes_of(seq):
    """A str over ACGTN (any case, anything else N) or an array of codes -> a list of codes 0..4."""
    if isinstance(seq, str):
        return [{"A": 0, "C": 1, "G": 2, "T": 3, "U": 3}.get(ch, 4) for ch in seq.upper()]
    return [int(c) for c in seq]


def clip(n, m, dlo, dhi):
    return max(dlo, -n), min(dhi, m)


def recurrence(a, b, dlo, dhi):
    """-> (cost, M, s, e), or None for a band that is empty after clipping."""
    a, b = codes_of(a), codes_of(b)
    n, m = len(a), len(b)
    dlo, dhi = clip(n, m, dlo, dhi)
    if dlo > dhi:
        return None
    cell = {}
    for i in range(n + 1):
        for j in range(m + 1):
            if not dlo <= j - i <= dhi:
                continue
            cands = []
            if i == 0:
                cands.append((0, 0, j + n))
            if j == 0:
                cands.append((0, 0, n - i))
            if i > 0 and j > 0 and (i - 1, j - 1) in cell:
                c, negm, s = cell[i - 1, j - 1]
                cands.append((c - 1, negm - 1, s) if a[i - 1] == b[j - 1] and a[i - 1] < 4 else (c + 2, negm, s))
            for prev in ((i - 1, j), (i, j - 1)):
                if prev in cell:
                    c, negm, s = cell[prev]
                    cands.append((c + 2, negm, s))
            cell[i, j] = min(cands)
    ends = []
    for (i, j), (c, negm, s) in cell.items():
        if i == n:
            ends.append((c, negm, s, j))
        if j == m:
            ends.append((c, negm, s, m - i + n))
    c, negm, s, e = min(ends)
    return c, -negm, s, e


def _paths(n, m):
    """Every path of the (n, m) table from a boundary start to a boundary end: (s, e, gaps, [diagonal cells], dmin, dmax)."""
    out = []

    def walk(i, j, s, gaps, diag, dmin, dmax):
        d = j - i
        dmin, dmax = min(dmin, d), max(dmax, d)
        if i == n:
            out.append((s, j, gaps, tuple(diag), dmin, dmax))
        if j == m and i != n:
            out.append((s, m - i + n, gaps, tuple(diag), dmin, dmax))
        if i < n and j < m:
            walk(i + 1, j + 1, s, gaps, diag + [i * m + j], dmin, dmax)
        if i < n:
            walk(i + 1, j, s, gaps + 1, diag, dmin, dmax)
        if j < m:
            walk(i, j + 1, s, gaps + 1, diag, dmin, dmax)

    starts = [(0, j, j + n) for j in range(m + 1)] + [(i, 0, n - i) for i in range(1, n + 1)]
    for i, j, s in starts:
        walk(i, j, s, 0, [], j - i, j - i)
    return out


def brute_force_all(n, m, letters=2):
    """{(a, b, dlo, dhi): (cost, M, s, e)} for every a of n and b of m codes below `letters` and every band inside [-n, m]."""
    paths = _paths(n, m)
    P = len(paths)
    s = np.array([p[0] for p in paths])
    e = np.array([p[1] for p in paths])
    gaps = np.array([p[2] for p in paths])
    dmin = np.array([p[4] for p in paths])
    dmax = np.array([p[5] for p in paths])
    inc = np.zeros((P, max(n * m, 1)), dtype=np.int64)
    for k, p in enumerate(paths):
        for c in p[3]:
            inc[k, c] = 1
    seqs_a = [tuple((v // letters ** t) % letters for t in range(n)) for v in range(letters ** n)]
    seqs_b = [tuple((v // letters ** t) % letters for t in range(m)) for v in range(letters ** m)]
    out = {}
    for a in seqs_a:
        for b in seqs_b:
            eq = np.array([1 if a[i] == b[j] else 0 for i in range(n) for j in range(m)] or [0], dtype=np.int64)
            M = inc @ eq
            E = gaps + inc.sum(axis=1) - M
            cost = 2 * E - M
            key = (((cost + 64) * 64 + (32 - M)) * 64 + s) * 64 + e          # every field within 0 .. 63 at n <= 4, m <= 5
            for dlo in range(-n, m + 1):
                for dhi in range(dlo, m + 1):
                    ok = (dmin >= dlo) & (dmax <= dhi)
                    k = int(np.argmin(np.where(ok, key, 1 << 40)))
                    assert ok[k]
                    out[a, b, dlo, dhi] = (int(cost[k]), int(M[k]), int(s[k]), int(e[k]))
    return out


def unpack(key, n):
    cost = (key + (G >> 1)) >> 40
    rem = cost * G - key
    M = (rem + MT - 1) >> 20
    return int(cost), int(M), int(M * MT - rem) - BIAS + n


def rows(reads, pairs):
    """reads: code sequences; pairs: rows of (a index, b index, dlo, dhi).  -> DTYPE rows.  A band that is empty after clipping
    raises ValueError."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 4)
    out = np.zeros(len(pairs), dtype=DTYPE)
    if len(pairs) == 0:
        return out
    if len(pairs) > CHUNK:                           # pairs of like length together, few enough that a row's arrays stay in cache
        order = np.argsort(np.array([len(reads[p[0]]) for p in pairs]), kind="stable")
        for lo in range(0, len(pairs), CHUNK):
            out[order[lo:lo + CHUNK]] = rows(reads, pairs[order[lo:lo + CHUNK]])
        return out
    reads = {int(k): np.asarray(codes_of(reads[k]) if isinstance(reads[k], str) else reads[k], dtype=np.int64) for k in np.unique(pairs[:, :2])}
    n = np.array([len(reads[p[0]]) for p in pairs], dtype=np.int64)
    m = np.array([len(reads[p[1]]) for p in pairs], dtype=np.int64)
    dlo = np.maximum(pairs[:, 2], -n)
    dhi = np.minimum(pairs[:, 3], m)
    if (dlo > dhi).any():
        raise ValueError("pair %d: an empty band" % int(np.nonzero(dlo > dhi)[0][0]))
    P, W, N = len(pairs), int((dhi - dlo).max()) + 1, int(n.max())
    # A[p, i] = a_p[i] (5 where a has no base or a code 4); B[p, x] = b_p[x + dlo_p] (6 likewise): row i's cells j = i + d read
    # b[j - 1] = B[p, i - 1 + slot]
    A = np.full((P, N + 1), 5, dtype=np.int8)
    B = np.full((P, N + W + 1), 6, dtype=np.int8)
    for p, (ia, ib) in enumerate(pairs[:, :2]):
        a, b = reads[ia], reads[ib]
        A[p, :len(a)] = np.where(a < 4, a, 5)
        x0 = int(dlo[p])                                              # B[p, x] = b[x + x0]
        lo, hi = max(0, -x0), min(N + W + 1, len(b) - x0)
        if hi > lo:
            B[p, lo:hi] = np.where(b[lo + x0:hi + x0] < 4, b[lo + x0:hi + x0], 6)
    # Stored as R = key - slot * 2^41, so that the move along a row -- (i, j-1), the diagonal below, at 2^41 -- is a running minimum.
    # Cells outside the table are not masked: left of column 0 they stay at INF or above (the pads match nothing), right of column
    # m and below row n they hold values no cell of the table reads.  A diagonal's last cell is copied out when it is computed.
    slot = np.arange(W, dtype=np.int64)
    ramp = slot * (2 * G)
    width = dhi - dlo + 1
    out_band = slot[None, :] >= width[:, None]
    d0 = dlo[:, None] + slot[None, :]
    R = np.where((d0 >= 0) & (d0 <= m[:, None]) & ~out_band, d0 + BIAS, INF) - ramp
    key = np.full((P, W), INF, dtype=np.int64)
    every = np.arange(P)
    for i in range(N + 1):
        if i > 0:
            best = R + np.where(B[:, i - 1:i - 1 + W] == A[:, i - 1:i], -G - MT, 2 * G)       # (i-1, j-1): the same diagonal
            np.minimum(best[:, :-1], R[:, 1:] + 4 * G, out=best[:, :-1])                      # (i-1, j): the diagonal above
            x0 = -dlo - i                                                                   # column 0: a start
            at0 = (x0 >= 0) & (x0 < width)
            best[every[at0], x0[at0]] = BIAS - i - x0[at0] * (2 * G)
            R = np.minimum.accumulate(best, axis=1)
            if out_band.any():
                np.putmask(R, out_band, INF)
        xm = m - dlo - i                                                                    # column m: the end of its diagonal
        atm = (xm >= 0) & (xm < width) & (i <= n)
        key[every[atm], xm[atm]] = R[every[atm], xm[atm]] + xm[atm] * (2 * G)
        for p in np.nonzero(n == i)[0]:                                                     # row n: the ends of the others
            hi = int(min(width[p] - 1, m[p] - dlo[p] - n[p]))
            if hi >= 0:
                key[p, :hi + 1] = R[p, :hi + 1] + ramp[:hi + 1]
    at = np.argmin(key, axis=1)                                                             # the first minimum: the smallest e
    for p in range(P):
        c, M, s = unpack(int(key[p, at[p]]), int(n[p]))
        out[p] = (c, M, s, int(dlo[p] + at[p] + n[p]))
    return out
