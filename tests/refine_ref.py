"""The definition of chiron_signal_refine (include/chiron_amd.h) restated three times, independent of the code under test.

refine_item        the recurrence in plain Python, cell by cell: F[n][s] = P(s) + min over candidates s' < s of (F[n-1][s'] - P(s')),
                   the predecessor the smallest s' that attains the minimum.
brute_item         every strictly increasing assignment inside the windows, enumerated; the tie rule applied as the header words it
                   (smallest s[L-1], then smallest s[L-2], ...).  Only for small half-widths.
refine_item_numpy  the same recurrence a row at a time in numpy (cumsum, minimum.accumulate), fast enough for the planted case and
                   for the GPU tests' long items.

`half` is the half-width of a border's window, HALF = 32 in the library; other values exist for the brute force only.
refine / refine_plain have the signature of chiron_amd.squiggle's refiner= hook: (signals, levels, starts) per item ->
([int32 starts per item], int64 costs)."""
import itertools

import numpy as np

HALF = 32
INFEASIBLE = (1 << 63) - 1


def cost_of(x, e, s):
    """sum over n of sum over t in s[n] .. s[n+1]) of |x[t] - e[n]|, in Python integers."""
    return sum(abs(int(x[t]) - int(e[n])) for n in range(len(e)) for t in range(int(s[n]), int(s[n + 1])))


def _candidates(a, n, L, half):
    if n == 0 or n == L:
        return [a[n]]
    return [s for s in range(a[n] - half, a[n] + half) if a[0] <= s <= a[L]]


def refine_item(x, e, a, half=HALF):
    """-> ([s[0 .. L]], cost), or (a copy of a, INFEASIBLE)."""
    a = [int(v) for v in a]
    L = len(e)
    assert len(a) == L + 1
    F = {a[0]: 0}
    back = []
    for n in range(1, L + 1):
        lv = int(e[n - 1])
        new, pred = {}, {}
        for s in _candidates(a, n, L, half):
            best = arg = None
            for sp in sorted(F):
                if sp >= s:
                    break
                c = F[sp] + sum(abs(int(x[t]) - lv) for t in range(sp, s))
                if best is None or c < best:                      # strictly: the smallest s' that attains the minimum stays
                    best, arg = c, sp
            if best is not None:
                new[s], pred[s] = best, arg
        F = new
        back.append(pred)
    if a[L] not in F:
        return list(a), INFEASIBLE
    s = [a[L]]
    for pred in reversed(back):
        s.append(pred[s[-1]])
    return s[::-1], F[a[L]]


def brute_item(x, e, a, half):
    a = [int(v) for v in a]
    L = len(e)
    if L == 0:
        return list(a), 0
    best = None
    for mid in itertools.product(*[_candidates(a, n, L, half) for n in range(1, L)]):
        s = [a[0]] + list(mid) + [a[L]]
        if any(s[n + 1] <= s[n] for n in range(L)):
            continue
        key = (cost_of(x, e, s), s[::-1])                          # the cost, then s[L-1], then s[L-2], ...
        if best is None or key < best:
            best = key
    if best is None:
        return list(a), INFEASIBLE
    return best[1][::-1], best[0]


def refine_item_numpy(x, e, a, half=HALF):
    x = np.asarray(x, dtype=np.int64)
    a = np.asarray(a, dtype=np.int64)
    L, W = len(e), 2 * half
    a0, aL = int(a[0]), int(a[L])
    none = np.int64(1 << 62)
    lanes = np.arange(W, dtype=np.int64)
    F = np.where(lanes == half, 0, none).astype(np.int64)
    masks = np.zeros((L, W), dtype=bool)
    for n in range(1, L + 1):
        w, d = int(a[n - 1]) - half, int(a[n] - a[n - 1])
        lo, hi = max(w, a0), min(w + d + W, aL)
        v = np.zeros(d + W, dtype=np.int64)
        if hi > lo:
            v[lo - w:hi - w] = np.abs(x[lo:hi] - int(e[n - 1]))
        P = np.concatenate([[0], np.cumsum(v)])
        G = np.where(F == none, none, F - P[:W])
        M = np.minimum.accumulate(G)
        masks[n - 1] = G < np.concatenate([[none], M[:-1]])
        reach = np.minimum(lanes + min(d, W) - 1, W - 1)
        m = np.where(reach >= 0, M[np.maximum(reach, 0)], none)
        s = int(a[n]) - half + lanes
        live = (m != none) & (s >= a0) & (s <= aL) & ((n < L) | (lanes == half))
        F = np.where(live, m + P[d:d + W], none)
    if F[half] == none:
        return [int(v) for v in a], INFEASIBLE
    out, j = [aL], half
    for n in range(L, 0, -1):
        reach = min(j + min(int(a[n] - a[n - 1]), W) - 1, W - 1)
        j = int(np.flatnonzero(masks[n - 1][:reach + 1])[-1])
        out.append(int(a[n - 1]) - half + j)
    return out[::-1], int(F[half])


def _over(fn, signals, levels, starts):
    got = [fn(x, e, a) for x, e, a in zip(signals, levels, starts)]
    return [np.asarray(s, dtype=np.int32) for s, _ in got], np.array([c for _, c in got], dtype=np.int64)


def flatten(signals, levels, starts):
    """The arrays chiron_signal_refine takes, each with one pad element: (samples, sample_off, level, start_in, base_off)."""
    off = lambda lens: np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.int64)
    cat = lambda parts, dtype: np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=dtype).reshape(-1) for p in parts] + [np.zeros(1, dtype)]))
    return (cat(signals, np.int16), off([len(s) for s in signals]), cat(levels, np.int32), cat(starts, np.int32), off([len(e) for e in levels]))


def refine(signals, levels, starts):
    return _over(refine_item_numpy, signals, levels, starts)


def refine_plain(signals, levels, starts):
    return _over(refine_item, signals, levels, starts)


def expected_levels(read, codes, table, k, unknown):
    """chiron_amd.squiggle.expected_levels as a walk in plain Python: the genome k-mer around the position of every '=' and 'X'
    column (in the read's orientation, squiggle_ref.kmer_bins), the read's own k-mer around every other base."""
    import squiggle_ref
    called = [int(c) for c in read["called"]]
    n, h = len(called), k // 2
    bins = squiggle_ref.kmer_bins(read, codes, k)
    on_column = set(idx for _, idx in squiggle_ref.walk_columns(read))
    out = []
    for i in range(n):
        code = -1
        if i in on_column:
            code = int(bins[i])
        elif i - h >= 0 and i - h + k <= n and all(c <= 3 for c in called[i - h:i - h + k]):
            code = 0
            for c in called[i - h:i - h + k]:
                code = code * 4 + c
        out.append(int(table[code]) if code >= 0 else unknown)
    return np.array(out, dtype=np.int32)
