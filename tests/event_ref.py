"""The definitions of chiron_signal_events and chiron_event_locate (include/chiron_amd.h) restated, independent of the code under test.

The detector, twice:
segment_plain   T[i] from the windows' sums taken anew at every i, the borders by the first-index-of-the-maximum rule, the levels by
                floor division, all in Python integers.
segment_numpy   the same from prefix sums and shifted comparisons.
Each gives (levels int16 [count], borders int32 [count + 1], truncated).

The DP, three times:
columns_plain   the recurrence in plain Python, cell by cell, over pairs (cost, start) ordered lexicographically.
columns_brute   every path enumerated -- a first column and, per further event, stay, move on or skip a column -- for tiny Q and R.
columns_numpy   the recurrence a row at a time in numpy, cost and start packed into one int64 so that the lexmin is a minimum.
Each gives, per end column, (D[j], S[j]) with NONE in both for a column without a path.  The block triples are locate_ref's
blocks_of; locator(penalty) has the signature of chiron_amd.locate's locator= hook: (queries, ref) -> int32 [items][blocks][3]."""
import itertools

import numpy as np

from locate_ref import BLOCK, BREAK, NONE, blocks_of  # noqa: F401  the same output as chiron_signal_locate

_INF = 1 << 31                                  # above every real cost (below 2^30) with a penalty on top
_SHIFT, _MASK = 28, (1 << 28) - 1               # a start is a column, below CHIRON_LOCATE_MAX_REF = 2^28


# ----------------------------------------------------------------------------------------------------------------------------
# the detector
# ----------------------------------------------------------------------------------------------------------------------------
def statistic_plain(x, w):
    """T[0 .. n] as Python integers."""
    x = [int(v) for v in x]
    n = len(x)
    T = [0] * (n + 1)
    for i in range(w, n - w + 1):
        a, b = x[i - w:i], x[i:i + w]
        s1, q1, s2, q2 = sum(a), sum(v * v for v in a), sum(b), sum(v * v for v in b)
        d = s1 - s2
        V = (w * q1 - s1 * s1) + (w * q2 - s2 * s2)
        T[i] = (w * d * d * 256) // max(V, 1)
    return T


def _cut(x, borders, max_events):
    """Borders (0 and n among them, increasing) -> (levels, kept borders, truncated)."""
    x = [int(v) for v in x]
    truncated = len(borders) - 1 > max_events
    borders = borders[:max_events + 1]
    levels = []
    for a, b in zip(borders[:-1], borders[1:]):
        s, c = sum(x[a:b]), b - a
        levels.append((2 * s + c) // (2 * c))
    return np.asarray(levels, dtype=np.int16), np.asarray(borders, dtype=np.int32), truncated


def segment_plain(x, w, r, thr, max_events=1 << 17):
    n = len(x)
    T = statistic_plain(x, w)
    borders = [0]
    for i in range(1, n):
        if T[i] >= thr:
            lo, hi = max(i - r, 0), min(i + r, n)
            top = max(T[lo:hi + 1])
            if T[i] == top and T[lo:hi + 1].index(top) + lo == i:
                borders.append(i)
    return _cut(x, borders + [n], max_events)


def statistic_numpy(x, w):
    x = np.asarray(x, dtype=np.int64)
    n = len(x)
    T = np.zeros(n + 1, dtype=np.int64)
    if n < 2 * w:
        return T
    p1, p2 = np.concatenate([[0], np.cumsum(x)]), np.concatenate([[0], np.cumsum(x * x)])
    i = np.arange(w, n - w + 1)
    s1, q1 = p1[i] - p1[i - w], p2[i] - p2[i - w]
    s2, q2 = p1[i + w] - p1[i], p2[i + w] - p2[i]
    d = s1 - s2
    V = (w * q1 - s1 * s1) + (w * q2 - s2 * s2)
    T[i] = (w * d * d * 256) // np.maximum(V, 1)
    return T


def segment_numpy(x, w, r, thr, max_events=1 << 17):
    n = len(x)
    T = statistic_numpy(x, w)
    ok = T >= thr
    for k in range(1, r + 1):                          # strictly above what lies left, at or above what lies right
        ok[k:] &= T[k:] > T[:-k]
        ok[:-k] &= T[:-k] >= T[k:]
    ok[0] = ok[n] = True
    borders = np.flatnonzero(ok)
    truncated = len(borders) - 1 > max_events
    borders = borders[:max_events + 1]
    sums = np.concatenate([[0], np.cumsum(np.asarray(x, dtype=np.int64))])
    s, c = sums[borders[1:]] - sums[borders[:-1]], borders[1:] - borders[:-1]
    return ((2 * s + c) // (2 * c)).astype(np.int16), borders.astype(np.int32), truncated


# ----------------------------------------------------------------------------------------------------------------------------
# the DP
# ----------------------------------------------------------------------------------------------------------------------------
def columns_plain(x, e, P):
    """-> [(D[j], S[j]) or (NONE, NONE) per column]."""
    x, e = [int(v) for v in x], [int(v) for v in e]
    R = len(e)
    row = [None if e[j] == BREAK else (abs(x[0] - e[j]), j) for j in range(R)]
    for t in range(1, len(x)):
        new = []
        for j in range(R):
            best = None
            if e[j] != BREAK:
                cands = [row[j]]
                if j >= 1:
                    cands.append(row[j - 1])
                if j >= 2 and e[j - 1] != BREAK and row[j - 2] is not None:
                    cands.append((row[j - 2][0] + P, row[j - 2][1]))
                for cand in cands:
                    if cand is not None and (best is None or cand < best):      # tuples: cost, then start
                        best = cand
                if best is not None:
                    best = (best[0] + abs(x[t] - e[j]), best[1])
            new.append(best)
        row = new
    return [(NONE, NONE) if v is None else v for v in row]


def columns_brute(x, e, P):
    """Every path: a first column and len(x) - 1 moves of 0, 1 or 2 columns.  Only for tiny inputs."""
    x, e = [int(v) for v in x], [int(v) for v in e]
    R, Q = len(e), len(x)
    best = [None] * R
    for first in range(R):
        for moves in itertools.product((0, 1, 2), repeat=Q - 1):
            j, cost, ok = first, 0, True
            for t in range(Q):
                if t:
                    if moves[t - 1] == 2:
                        if j + 1 >= R or e[j + 1] == BREAK:
                            ok = False
                            break
                        cost += P
                    j += moves[t - 1]
                if j >= R or e[j] == BREAK:
                    ok = False
                    break
                cost += abs(x[t] - e[j])
            if ok and (best[j] is None or (cost, first) < best[j]):
                best[j] = (cost, first)
    return [(NONE, NONE) if v is None else v for v in best]


def _rows_numpy(x, e, P):
    """The last row as packed int64: cost << 28 | start; a cost of _INF or more is a column without a path.  Such a column is set
    back to _INF every row, so nothing grows past 2^33 << 28."""
    x = np.asarray(x, dtype=np.int64)
    e = np.asarray(e, dtype=np.int64)
    brk = e == BREAK
    lv = np.where(brk, 0, e)
    none = _INF << _SHIFT
    over = np.concatenate([[True], brk[:-1]]) if len(e) else brk        # whether the column to the left is a break
    row = (np.where(brk, _INF, np.abs(x[0] - lv)) << _SHIFT) | np.arange(len(e), dtype=np.int64)
    for t in range(1, len(x)):
        left = np.concatenate([[none], row[:-1]])
        skip = np.concatenate([[none, none], row[:-2]])[:len(e)] + (int(P) << _SHIFT)
        skip[over] = none
        row = np.minimum(np.minimum(row, left), skip) + (np.abs(x[t] - lv) << _SHIFT)
        row[brk | (row >= none)] = none
    return row


def columns_numpy(x, e, P):
    row = _rows_numpy(x, e, P)
    cost, start = row >> _SHIFT, row & _MASK
    return [(int(c), int(s)) if c < _INF else (NONE, NONE) for c, s in zip(cost, start)]


def blocks_numpy(x, e, P, block=BLOCK):
    """blocks_of(columns_numpy(x, e, P)) without the Python loop over columns."""
    row = _rows_numpy(x, e, P)
    R = len(row)
    n = (R + block - 1) // block
    out = np.full((n, 3), NONE, dtype=np.int32)
    if R == 0:
        return out
    cost = np.concatenate([row >> _SHIFT, np.full(n * block - R, _INF, np.int64)]).reshape(n, block)
    j = cost.argmin(axis=1)                                                      # the first of the smallest
    best = cost[np.arange(n), j]
    col = np.arange(n) * block + j
    ok = best < _INF
    out[ok, 0], out[ok, 1], out[ok, 2] = best[ok], col[ok], (row[col[ok]] & _MASK)
    return out


def locate(queries, ref, P):
    n = (len(ref) + BLOCK - 1) // BLOCK
    return np.stack([blocks_numpy(q, ref, P) for q in queries]).astype(np.int32) if len(queries) else np.zeros((0, n, 3), np.int32)


def locate_plain(queries, ref, P):
    n = (len(ref) + BLOCK - 1) // BLOCK
    return np.stack([blocks_of(columns_plain(q, ref, P)) for q in queries]).astype(np.int32) if len(queries) else np.zeros((0, n, 3), np.int32)


def locator(P):
    """The locator= hook on the numpy rows at penalty P."""
    return lambda queries, ref: locate(queries, ref, P)
