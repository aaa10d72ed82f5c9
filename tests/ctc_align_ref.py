"""The semantics of chiron_ctc_align (include/chiron_amd.h) restated in numpy float64: the max-plus recursion over the S = 2L+1
states of the extended label, the tie order, the band passes with their edge rule and doubling, and the statuses.  Vectorised
over states, one frame per step; every step is one float64 add of a float32 widened to float64, as in the kernel, so the results
compare with == and not with a tolerance.  `brute_force` enumerates every step sequence of a tiny case."""
import itertools

import numpy as np

BLANK = 4
NEG = -np.inf


def _c(t, S, F):
    return (int(t) * (S - 1)) // max(F - 1, 1)


def band_pass(x, lab, w, full):
    """One pass of half-width w (full: the whole table).  -> (accepted, score, start) or (False, -inf, None) when the end is
    not reachable."""
    F, L = x.shape[0], len(lab)
    S = 2 * L + 1
    cls = np.full(S, BLANK, dtype=np.int64)
    cls[1::2] = lab
    allow2 = np.zeros(S, dtype=bool)
    if L > 1:
        allow2[3::2] = lab[1:] != lab[:-1]
    xd = x.astype(np.float64)
    lo_of = (lambda c: 0) if full else (lambda c: max(0, c - w))
    hi_of = (lambda c: S - 1) if full else (lambda c: min(S - 1, c + w))
    # prev / cur are padded by two -inf cells on the left, so that s-1 and s-2 of state 0 read -inf
    prev = np.full(S + 2, NEG)
    cur = np.full(S + 2, NEG)
    bp = np.zeros((F, S), dtype=np.uint8)
    h0 = hi_of(0)
    prev[2] = xd[0, BLANK]
    if h0 >= 1:
        prev[3] = xd[0, lab[0]]
    plo, phi = 0, h0
    for t in range(1, F):
        c = _c(t, S, F)
        lo, hi = lo_of(c), hi_of(c)
        stay = prev[lo + 2:hi + 3]
        d1 = prev[lo + 1:hi + 2]
        d2 = np.where(allow2[lo:hi + 1], prev[lo:hi + 1], NEG)
        best = stay.copy()
        m = np.zeros(hi - lo + 1, dtype=np.uint8)
        g = d1 > best
        best[g] = d1[g]
        m[g] = 1
        g = d2 > best
        best[g] = d2[g]
        m[g] = 2
        cur[lo + 2:hi + 3] = best + xd[t, cls[lo:hi + 1]]
        bp[t, lo:hi + 1] = m
        prev[plo + 2:phi + 3] = NEG          # the row before last: cleared, it becomes the next frame's target
        prev, cur = cur, prev
        plo, phi = lo, hi
    s = S - 1
    best = prev[S + 1]
    if S >= 2 and prev[S] > best:
        best = prev[S]
        s = S - 2
    if not best > NEG:
        return False, NEG, None
    start = np.full(L, -1, dtype=np.int32)
    ok = True
    for t in range(F - 1, -1, -1):
        c = _c(t, S, F)
        if not full and ((s == c - w and s > 0) or (s == c + w and s < S - 1)):
            ok = False
        m = int(bp[t, s]) if t > 0 else 0
        if (s & 1) and (m != 0 or t == 0):
            start[s >> 1] = t
        s -= m
    assert s in (0, 1)
    return ok, float(best), start


def align_one(x, lab, band0=0, max_band=0):
    """-> (start int32 [L], score float64, band, status) of one read: x float32 [F, 5], lab codes 0..3."""
    x = np.asarray(x, dtype=np.float32).reshape(-1, 5)
    lab = np.asarray(lab, dtype=np.uint8)
    F, L = x.shape[0], len(lab)
    S = 2 * L + 1
    fail = np.full(L, -1, dtype=np.int32)
    rep = int(np.count_nonzero(lab[1:] == lab[:-1])) if L > 1 else 0
    if F < L + rep:
        return fail, NEG, band0, 1
    if F == 0:
        return fail, 0.0, band0, 0
    w = band0
    while True:
        full = band0 == 0 or w >= S - 1
        ok, score, start = band_pass(x, lab, w, full)
        if ok or full:
            return start, score, w, 0
        nxt = 2 * w
        if max_band > 0 and nxt > max_band and nxt < S - 1:
            return fail, NEG, w, 2
        w = nxt


def align(scores_list, labels_list, band0=0, max_band=0):
    """The batch form of chiron_amd.label.align: a dict of start (list), score, band, status."""
    out = [align_one(x, l, band0, max_band) for x, l in zip(scores_list, labels_list)]
    return {"start": [o[0] for o in out], "score": np.array([o[1] for o in out], dtype=np.float64),
            "band": np.array([o[2] for o in out], dtype=np.int32), "status": np.array([o[3] for o in out], dtype=np.int32)}


def brute_force(x, lab):
    """The best score over EVERY valid state sequence (F <= 7, L <= 3), or None when there is none."""
    x = np.asarray(x, dtype=np.float32).reshape(-1, 5)
    F, L = x.shape[0], len(lab)
    S = 2 * L + 1
    assert F <= 7 and L <= 3
    if F == 0:
        return 0.0 if L == 0 else None
    cls = [BLANK if s % 2 == 0 else int(lab[s >> 1]) for s in range(S)]
    best = None
    for first in (0, 1):
        if first >= S:
            continue
        for steps in itertools.product((0, 1, 2), repeat=F - 1):
            s, total, valid = first, float(x[0, cls[first]]), True
            for t, d in enumerate(steps, 1):
                n = s + d
                if n >= S or (d == 2 and not (n % 2 == 1 and lab[n >> 1] != lab[(n >> 1) - 1])):
                    valid = False
                    break
                s = n
                total = total + float(x[t, cls[s]])
            if valid and s >= S - 2 and (best is None or total > best):
                best = total
    return best

