"""The definition of chiron_signal_locate (include/chiron_amd.h) restated three times, independent of the code under test.

columns_plain   the recurrence in plain Python, cell by cell, over pairs (cost, start) ordered lexicographically.
columns_brute   every path enumerated -- a first column and, per further sample, stay or move on -- for tiny Q and R; per end column
                the least cost and the smallest first column among the paths that attain it.
columns_numpy   the same recurrence a row at a time in numpy, cost and start packed into one int64 so that the lexmin is a minimum.

Each gives, per end column, (D[j], S[j]) with NONE in both for a column without a path.  blocks_of reduces them to the block
triples of the output; locate / locate_plain have the signature of chiron_amd.locate's locator= hook: (queries, ref) -> int32
[items][blocks][3]."""
import itertools

import numpy as np

BREAK = -(1 << 31)
NONE = (1 << 31) - 1
BLOCK = 1024
_INF = 1 << 31                                  # above every real cost (below 2^30), and with 2^30 on top still below 2^32
_SHIFT, _MASK = 28, (1 << 28) - 1               # a start is a column, below CHIRON_LOCATE_MAX_REF = 2^28


def columns_plain(x, e):
    """-> [(D[j], S[j]) or (NONE, NONE) per column]."""
    x, e = [int(v) for v in x], [int(v) for v in e]
    R = len(e)
    row = [None if e[j] == BREAK else (abs(x[0] - e[j]), j) for j in range(R)]
    for t in range(1, len(x)):
        new = []
        for j in range(R):
            best = None
            if e[j] != BREAK:
                for cand in ([row[j]] + ([row[j - 1]] if j > 0 else [])):
                    if cand is not None and (best is None or cand < best):      # tuples: cost, then start
                        best = cand
                if best is not None:
                    best = (best[0] + abs(x[t] - e[j]), best[1])
            new.append(best)
        row = new
    return [(NONE, NONE) if v is None else v for v in row]


def columns_brute(x, e):
    """Every path: a first column and len(x) - 1 choices of stay / move.  Only for tiny inputs."""
    x, e = [int(v) for v in x], [int(v) for v in e]
    R, Q = len(e), len(x)
    best = [None] * R
    for first in range(R):
        for moves in itertools.product((0, 1), repeat=Q - 1):
            j, cost, ok = first, 0, True
            for t in range(Q):
                if t:
                    j += moves[t - 1]
                if j >= R or e[j] == BREAK:
                    ok = False
                    break
                cost += abs(x[t] - e[j])
            if ok and (best[j] is None or (cost, first) < best[j]):
                best[j] = (cost, first)
    return [(NONE, NONE) if v is None else v for v in best]


def _rows_numpy(x, e):
    """The last row as packed int64: cost << 28 | start (a start is below 2^28); a cost of _INF or more is a column without a
    path.  Such a column is set back to _INF every row, so nothing grows past 2^32 << 28."""
    x = np.asarray(x, dtype=np.int64)
    e = np.asarray(e, dtype=np.int64)
    brk = e == BREAK
    lv = np.where(brk, 0, e)
    row = (np.where(brk, _INF, np.abs(x[0] - lv)) << _SHIFT) | np.arange(len(e), dtype=np.int64)
    for t in range(1, len(x)):
        left = np.concatenate([[_INF << _SHIFT], row[:-1]])
        row = np.minimum(row, left) + (np.abs(x[t] - lv) << _SHIFT)
        row[brk] = _INF << _SHIFT
    return row


def columns_numpy(x, e):
    row = _rows_numpy(x, e)
    cost, start = row >> _SHIFT, row & _MASK
    return [(int(c), int(s)) if c < _INF else (NONE, NONE) for c, s in zip(cost, start)]


def blocks_of(columns, block=BLOCK):
    """[(D, S) per column] -> int32 [blocks][3]: per block the least D, the smallest column that attains it, and its S."""
    n = (len(columns) + block - 1) // block
    out = np.full((n, 3), NONE, dtype=np.int32)
    for b in range(n):
        best = None
        for j in range(b * block, min(len(columns), (b + 1) * block)):
            d, s = columns[j]
            if d != NONE and (best is None or d < best[0]):
                best = (d, j, s)
        if best is not None:
            out[b] = best
    return out


def blocks_numpy(x, e, block=BLOCK):
    """blocks_of(columns_numpy(x, e)) without the Python loop over columns."""
    row = _rows_numpy(x, e)
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


def locate(queries, ref):
    """The locator= hook on the numpy rows."""
    n = (len(ref) + BLOCK - 1) // BLOCK
    return np.stack([blocks_numpy(q, ref) for q in queries]).astype(np.int32) if len(queries) else np.zeros((0, n, 3), np.int32)


def locate_plain(queries, ref):
    """The locator= hook on the plain-Python recurrence."""
    n = (len(ref) + BLOCK - 1) // BLOCK
    return np.stack([blocks_of(columns_plain(q, ref)) for q in queries]).astype(np.int32) if len(queries) else np.zeros((0, n, 3), np.int32)
