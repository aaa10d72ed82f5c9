"""The definition of chiron_demux_windows (include/chiron_amd.h) restated three times in plain Python / numpy, sharing no code
with the package:

  pair_dp        a column DP over uint8 codes, one window base at a time: the reference
  pair_bitvector the kernel's automaton (Myers / Hyyro, the first row free) in Python ints held to 64 bits
  pairs_batch    pair_dp with a leading axis over windows of one length, for the large GPU cases

and the per-window reduction (reduce_window, match) the kernel does with shuffles.  Codes 0..3; 4 and above match nothing."""
import numpy as np

NONE = 0x7FFFFFFF
MASK64 = (1 << 64) - 1


def pair_dp(pat, win):
    """(E, e) of pattern codes `pat` (n >= 1) against window codes `win`: D(e) = the last cell of the column after e window bases,
    row 0 free; the smallest D, then the smallest e."""
    pat = np.asarray(pat, dtype=np.int64)
    n = len(pat)
    col = np.arange(n + 1, dtype=np.int64)          # before any window base: cell i costs i deletions of pattern bases
    best, end = int(col[n]), 0
    for j, c in enumerate(np.asarray(win, dtype=np.int64)):
        sub = col[:-1] + np.where((pat == c) & (c < 4), 0, 1)
        new = np.empty_like(col)
        new[0] = 0
        new[1:] = np.minimum(sub, col[1:] + 1)
        for i in range(1, n + 1):                   # the vertical move, in order
            if new[i - 1] + 1 < new[i]:
                new[i] = new[i - 1] + 1
        col = new
        if col[n] < best:
            best, end = int(col[n]), j + 1
    return best, end


def masks_of(pat):
    """The four match masks of a pattern as Python ints: bit i of mask c set when base i is c."""
    m = [0, 0, 0, 0]
    for i, c in enumerate(pat):
        if c < 4:
            m[int(c)] |= 1 << i
    return m


def pair_bitvector(pat, win):
    """(E, e) by the kernel's arithmetic: every word is cut to 64 bits after each operation that can pass them, so a 64-base
    pattern sees the wrap of the add exactly as uint64_t does."""
    n = len(pat)
    peq = masks_of(pat)
    top = 1 << (n - 1)
    pv, mv = MASK64, 0
    score = best = n
    end = 0
    for j, c in enumerate(win):
        eq = peq[int(c)] if c < 4 else 0
        xv = eq | mv
        xh = ((((eq & pv) + pv) & MASK64) ^ pv) | eq
        ph = mv | (~(xh | pv) & MASK64)
        mh = pv & xh
        score += 1 if ph & top else 0
        score -= 1 if mh & top else 0
        ph = (ph << 1) & MASK64
        mh = (mh << 1) & MASK64
        pv = mh | (~(xv | ph) & MASK64)
        mv = ph & xv
        if score < best:
            best, end = score, j + 1
    return best, end


def pairs_batch(pat, wins):
    """pair_dp of one pattern against W windows of one length m at once: wins uint8 [W, m] -> (E int64 [W], e int64 [W])."""
    pat = np.asarray(pat, dtype=np.int64)
    wins = np.asarray(wins, dtype=np.int64)
    W, m = wins.shape
    n = len(pat)
    rows = np.arange(n + 1, dtype=np.int64)[None, :]
    col = np.tile(rows, (W, 1))
    best = col[:, n].copy()
    end = np.zeros(W, dtype=np.int64)
    for j in range(m):
        c = wins[:, j:j + 1]
        sub = col[:, :-1] + np.where((pat[None, :] == c) & (c < 4), 0, 1)
        new = np.empty_like(col)
        new[:, 0] = 0
        new[:, 1:] = np.minimum(sub, col[:, 1:] + 1)
        col = np.minimum.accumulate(new - rows, axis=1) + rows      # the vertical move: cell i = min over k <= i of cell k + (i - k)
        better = col[:, n] < best
        best = np.where(better, col[:, n], best)
        end = np.where(better, j + 1, end)
    return best, end


def reduce_window(E, e, groups):
    """(best, dist, end, second) of one window from its pairs' E and e."""
    E = [int(v) for v in E]
    best = min(range(len(E)), key=lambda q: (E[q], q))
    others = [E[q] for q in range(len(E)) if groups[q] != groups[best]]
    return best, E[best], int(e[best]), (min(others) if others else NONE)


def matrix(windows, patterns):
    """(E, e), int64 [windows, patterns]; windows of equal length go through pairs_batch together."""
    W, P = len(windows), len(patterns)
    E = np.zeros((W, P), dtype=np.int64)
    e = np.zeros((W, P), dtype=np.int64)
    by_len = {}
    for w, t in enumerate(windows):
        by_len.setdefault(len(t), []).append(w)
    for m, ws in by_len.items():
        block = np.array([np.asarray(windows[w], dtype=np.uint8) for w in ws], dtype=np.uint8).reshape(len(ws), m)
        for q, p in enumerate(patterns):
            E[ws, q], e[ws, q] = pairs_batch(p, block)
    return E, e


def reduce_windows(E, e, groups):
    """reduce_window of every row of E, e [windows, patterns] at once -> (best, dist, end, second) arrays."""
    groups = np.asarray(groups, dtype=np.int64)
    rows = np.arange(E.shape[0])
    best = np.argmin(E, axis=1) if E.shape[0] else np.zeros(0, np.int64)          # the first of equal minima: the smaller index
    other = groups[None, :] != groups[best][:, None]
    second = np.where(other, E, NONE).min(axis=1) if E.shape[0] else np.zeros(0, np.int64)
    return best, E[rows, best], e[rows, best], second


def match(windows, patterns, groups, want_matrix=False):
    """The package's matcher interface on the reference: the dict of demux.match_windows."""
    E, e = matrix(windows, patterns)
    out = {name: np.asarray(v, dtype=np.int32) for name, v in zip(("best", "dist", "end", "second"), reduce_windows(E, e, groups))}
    if want_matrix:
        out["pair_dist"], out["pair_end"] = E.astype(np.int16), e.astype(np.int16)
    return out
