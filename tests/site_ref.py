"""The definition of chiron_signal_score (include/chiron_amd.h) restated, independent of the code under test.

A candidate is a row of L levels e, 1 <= L <= 16, against the S samples x of the segment it names.  A path gives sample t a column
j_t with j_0 = 0, j_{S-1} = L - 1 and j_{t+1} in {j_t, j_t + 1}; cost = min over the paths of sum_t |x[t] - e[j_t]|, INFEASIBLE
when there is no path (S < L, S = 0 included).

Three restatements: score_item, the recurrence in plain Python integers; brute_item, every path enumerated (S <= 7, L <= 5);
score, the recurrence in numpy rows over all candidates of a call at once, which is what the GPU tests and tools/bench_modcall.py
compare with.  tests/test_modcall_cpu.py holds the three to each other."""
import itertools

import numpy as np

INFEASIBLE = (1 << 31) - 1
MAX_SAMPLES, MAX_COLUMNS = 4096, 16


def score_item(x, e):
    """D[0][0] = |x[0] - e[0]|, D[t][n] = min(D[t-1][n], D[t-1][n-1]) + |x[t] - e[n]| over the terms that exist; D[S-1][L-1]."""
    x, e = [int(v) for v in x], [int(v) for v in e]
    S, L = len(x), len(e)
    if S < L or S == 0:
        return INFEASIBLE
    row = [None] * L
    row[0] = abs(x[0] - e[0])
    for t in range(1, S):
        new = [None] * L
        for n in range(L):
            before = [v for v in (row[n], row[n - 1] if n > 0 else None) if v is not None]
            if before:
                new[n] = min(before) + abs(x[t] - e[n])
        row = new
    return INFEASIBLE if row[L - 1] is None else row[L - 1]


def brute_paths(x, e):
    """Every path: the L - 1 samples at which the column goes up, chosen among samples 1 .. S - 1.  -> [cost of every path]."""
    x, e = [int(v) for v in x], [int(v) for v in e]
    S, L = len(x), len(e)
    assert S <= 7 and L <= 5
    costs = []
    for ups in (itertools.combinations(range(1, S), L - 1) if S >= L else ()):
        col = cost = 0
        for t in range(S):
            col += t in ups
            cost += abs(x[t] - e[col])
        costs.append(cost)
    return costs


def brute_item(x, e):
    """The least cost over every path, INFEASIBLE when there is none."""
    costs = brute_paths(x, e)
    return min(costs) if costs else INFEASIBLE


def flatten(segments, candidates):
    """The arrays chiron_signal_score takes: (samples int16, sample_off int64, level int32, level_off int64, seg int32); the flat
    arrays end with one entry nobody owns, so that none is empty."""
    sig = [np.ascontiguousarray(s, dtype=np.int16).reshape(-1) for s in segments]
    lv = [np.ascontiguousarray(e, dtype=np.int32).reshape(-1) for _, e in candidates]
    off = lambda lens: np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.int64)
    return (np.ascontiguousarray(np.concatenate(sig + [np.zeros(1, np.int16)])), off([len(s) for s in sig]),
            np.ascontiguousarray(np.concatenate(lv + [np.zeros(1, np.int32)])), off([len(e) for e in lv]),
            np.asarray([g for g, _ in candidates], dtype=np.int32).reshape(-1))


def score_flat(samples, sample_off, level, level_off, seg):
    """The recurrence in numpy rows, every candidate of the call at once: row t of all candidates that still have a sample t, over
    int64 with NONE for a cell without a value."""
    NONE = 1 << 60
    n = len(seg)
    out = np.full(n, INFEASIBLE, dtype=np.int32)
    if n == 0:
        return out
    seg = np.asarray(seg, dtype=np.int64)
    first = np.asarray(sample_off, dtype=np.int64)[seg]
    S = np.asarray(sample_off, dtype=np.int64)[seg + 1] - first
    l0 = np.asarray(level_off, dtype=np.int64)[:-1]
    L = np.asarray(level_off, dtype=np.int64)[1:] - l0
    width = int(L.max())
    cols = np.arange(width)[None, :]
    real = cols < L[:, None]
    E = np.where(real, np.asarray(level, dtype=np.int64)[np.minimum(l0[:, None] + cols, len(level) - 1)], 0)
    x = np.asarray(samples, dtype=np.int64)
    D = np.full((n, width), NONE, dtype=np.int64)
    live = np.flatnonzero(S > 0)
    D[live, 0] = np.abs(x[first[live]] - E[live, 0])
    for t in range(1, int(S.max(initial=0))):
        live = live[S[live] > t]
        d = D[live]
        left = np.concatenate([np.full((len(live), 1), NONE, np.int64), d[:, :-1]], axis=1)
        best = np.minimum(d, left)
        D[live] = np.where((best < NONE) & real[live], best + np.abs(x[first[live] + t][:, None] - E[live]), NONE)
    last = D[np.arange(n), L - 1]
    ok = last < NONE
    out[ok] = last[ok].astype(np.int32)
    return out


def score(segments, candidates):
    """segments: int16 arrays; candidates: (segment index, int32 levels) pairs -> int32 costs [candidates]."""
    return score_flat(*flatten(segments, candidates))


def score_item_numpy(x, e):
    return int(score([x], [(0, e)])[0])


def score_plain(segments, candidates):
    return np.asarray([score_item(segments[g], e) for g, e in candidates], dtype=np.int32).reshape(-1)
