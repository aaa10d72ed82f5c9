"""Reference for the alignment traceback (chiron_align_trace / chiron_amd.assess.align_ops, cigar, error_profile): what the
canonical alignment of a pair IS, computed the slow and obvious way.  Shares no code with the package.

Semantics: global alignment, unit costs, the match rule of assess_ref (case-insensitive, U is T, anything but A, C, G, T matches
nothing).  Among the alignments with the smallest E and then the largest M, the canonical one is the one whose column string
over = X I D, read from the last column to the first, is smallest under the order diagonal (= or X) < I < D.  Columns are
numbered 0 '=', 1 'X', 2 'I' (a read base alone), 3 'D' (a reference base alone).

full_trace   a full-table numpy DP (assess_ref's keys E * 2^32 - M, row by row) that also records, per cell, the first admissible
             predecessor in the order diagonal, up, left, and then walks the pointers from (n, m).
banded_trace the same in plain Python on the diagonals [min(0, m-n) - w, max(0, m-n) + w] only.
brute        every alignment of a small pair enumerated; the (E, M)-optimal ones kept; the smallest reversed string returned.
error_profile, cigar   restated from their definitions in plain Python.
"""
import numpy as np

import assess_ref

G = assess_ref.G
LETTERS = "=XID"


def full_trace(read, ref):
    """-> (E, M, ops) of str read against str ref; ops a uint8 array, first column first."""
    a, b = assess_ref.canon(read), assess_ref.canon(ref)
    n, m = len(a), len(b)
    j = np.arange(m + 1, dtype=np.int64)
    okb = np.isin(b, (65, 67, 71, 84))
    ptr = np.zeros((n + 1, m + 1), dtype=np.uint8)
    ptr[0, 1:] = 2
    row = j * G
    for i in range(1, n + 1):
        diag = row[:-1] + np.where((b == a[i - 1]) & okb, -1, G)
        up = row[1:] + G
        A = np.empty(m + 1, np.int64)
        A[0] = i * G
        A[1:] = np.minimum(diag, up)
        new = np.minimum.accumulate(A - j * G) + j * G
        p = np.full(m + 1, 2, dtype=np.uint8)          # left, unless an earlier predecessor in the order is admissible
        p[1:][up == new[1:]] = 1
        p[1:][diag == new[1:]] = 0
        p[0] = 1
        ptr[i] = p
        row = new
    k = int(row[-1])
    E = (k + (G >> 1)) >> 32
    M = E * G - k
    ops = []
    i, jj = n, m
    while i or jj:
        q = ptr[i, jj]
        if q == 0:
            ops.append(0 if assess_ref.is_match(read[i - 1], ref[jj - 1]) else 1)
            i, jj = i - 1, jj - 1
        elif q == 1:
            ops.append(2)
            i -= 1
        else:
            ops.append(3)
            jj -= 1
    return E, M, np.array(ops[::-1], dtype=np.uint8)


def trace(read, ref):
    return full_trace(read, ref)[2]


def tight_band(n, m, E):
    """w*: every alignment of cost E lies on the diagonals [min(0, m-n) - w*, max(0, m-n) + w*]."""
    return (E - abs(m - n)) // 2


def banded_trace(read, ref, w):
    """(E, M, ops) of the DP restricted to the band of half-width w (cells outside it do not exist), with the same pointer rule
    and walk; E, M and ops are whatever the band yields, which is the truth only when the band holds every optimal alignment."""
    n, m = len(read), len(ref)
    dlo, dhi = min(0, m - n) - w, max(0, m - n) + w
    INF = 1 << 60
    K, P = {}, {}
    for i in range(n + 1):
        for j in range(max(0, i + dlo), min(m, i + dhi) + 1):
            if i == 0 and j == 0:
                K[0, 0] = 0
                continue
            cands = []
            if i and j:
                cands.append(K.get((i - 1, j - 1), INF) + (-1 if assess_ref.is_match(read[i - 1], ref[j - 1]) else G))
            else:
                cands.append(INF)
            cands.append(K.get((i - 1, j), INF) + G if i else INF)
            cands.append(K.get((i, j - 1), INF) + G if j else INF)
            best = min(cands)
            K[i, j] = best
            P[i, j] = cands.index(best)
    k = K[n, m]
    E = (k + (G >> 1)) >> 32
    M = E * G - k
    ops = []
    i, j = n, m
    while i or j:
        q = P[i, j]
        if q == 0:
            ops.append(0 if assess_ref.is_match(read[i - 1], ref[j - 1]) else 1)
            i, j = i - 1, j - 1
        elif q == 1:
            ops.append(2)
            i -= 1
        else:
            ops.append(3)
            j -= 1
    return E, M, np.array(ops[::-1], dtype=np.uint8)


_PATHS = {}


def _paths(n, m):
    """Every monotone path of an n x m table as a string over d (diagonal), i (up: a read base alone), l (left: a reference base
    alone), first column first; sorted by the reversed string under d < i < l.  Per path the (read, reference) indices of its
    diagonal columns, padded with (n, m)."""
    if (n, m) not in _PATHS:
        found = []

        def walk(i, j, sofar):
            if i == n and j == m:
                found.append(sofar)
                return
            if i < n and j < m:
                walk(i + 1, j + 1, sofar + "d")
            if i < n:
                walk(i + 1, j, sofar + "i")
            if j < m:
                walk(i, j + 1, sofar + "l")

        walk(0, 0, "")
        found.sort(key=lambda s: ["dil".index(ch) for ch in reversed(s)])
        width = max(1, min(n, m))
        ri = np.full((len(found), width), n, dtype=np.int64)
        rj = np.full((len(found), width), m, dtype=np.int64)
        gaps = np.zeros(len(found), dtype=np.int64)
        for p, s in enumerate(found):
            i = j = t = 0
            for ch in s:
                if ch == "d":
                    ri[p, t], rj[p, t] = i, j
                    i, j, t = i + 1, j + 1, t + 1
                elif ch == "i":
                    i += 1
                else:
                    j += 1
            gaps[p] = len(s) - t
        _PATHS[n, m] = (found, ri, rj, gaps, (ri < n).sum(axis=1))
    return _PATHS[n, m]


def brute(read, ref):
    """(E, M, ops) by enumerating EVERY alignment: each path's cost and matches, the paths of the smallest cost and then the most
    matches, and of those the one whose reversed string is smallest.  Lengths up to 5 or so."""
    n, m = len(read), len(ref)
    found, ri, rj, gaps, diags = _paths(n, m)
    eq = np.zeros((n + 1, m + 1), dtype=np.int64)       # the extra row and column: the padding matches nothing
    for i in range(n):
        for j in range(m):
            eq[i, j] = assess_ref.is_match(read[i], ref[j])
    matches = eq[ri, rj].sum(axis=1)
    cost = gaps + diags - matches
    E = int(cost.min())
    M = int(matches[cost == E].max())
    best = int(np.nonzero((cost == E) & (matches == M))[0][0])      # the paths are in the order of their reversed strings
    ops, i, j = [], 0, 0
    for ch in found[best]:
        if ch == "d":
            ops.append(0 if eq[i, j] else 1)
            i, j = i + 1, j + 1
        elif ch == "i":
            ops.append(2)
            i += 1
        else:
            ops.append(3)
            j += 1
    return E, M, np.array(ops, dtype=np.uint8)


def cigar(ops):
    if len(ops) == 0:
        return "*"
    out, run, cur = [], 0, ops[0]
    for o in list(ops) + [None]:
        if o == cur:
            run += 1
        else:
            out.append("%d%s" % (run, LETTERS[cur]))
            run, cur = 1, o
    return "".join(out)


def replay(cigar_text, seq, ref):
    """Walk a CIGAR over =XID along seq and ref (both from their first aligned base): -> (read bases used, reference bases used,
    edits); asserts that '=' columns hold equal bases and 'X' columns do not match."""
    import re
    i = j = edits = 0
    for count, op in re.findall(r"(\d+)([=XID])", cigar_text):
        for _ in range(int(count)):
            if op in "=X":
                assert assess_ref.is_match(seq[i], ref[j]) == (op == "="), (i, j, op)
                i, j = i + 1, j + 1
            elif op == "I":
                i += 1
            else:
                j += 1
            edits += op != "="
    assert "".join("%s%s" % pair for pair in re.findall(r"(\d+)([=XID])", cigar_text)) == cigar_text
    return i, j, edits


def code(ch):
    ch = ch.upper().replace("U", "T")
    return "ACGT".index(ch) if ch in "ACGT" else 4


def error_profile(read, ref, ops):
    """The tables of chiron_amd.assess.error_profile, column by column and run by run."""
    sub = [[0] * 4 for _ in range(4)]
    ins, dele, other = [0] * 5, [0] * 5, 0
    hp = [[0] * 21 for _ in range(11)]
    cols = []                                   # per column: (read code or None, reference index or None)
    i = j = 0
    for o in ops:
        if o in (0, 1):
            ca, cb = code(read[i]), code(ref[j])
            if ca < 4 and cb < 4:
                sub[cb][ca] += 1
            else:
                assert o == 1
                other += 1
            cols.append((ca, j))
            i, j = i + 1, j + 1
        elif o == 2:
            ins[code(read[i])] += 1
            cols.append((code(read[i]), None))
            i += 1
        else:
            dele[code(ref[j])] += 1
            cols.append((None, j))
            j += 1
    assert i == len(read) and j == len(ref)
    col_of = {rj: c for c, (_, rj) in enumerate(cols) if rj is not None}
    j = 0
    while j < len(ref):
        e = j
        while e + 1 < len(ref) and code(ref[e + 1]) == code(ref[j]):
            e += 1
        base = code(ref[j])
        if base < 4:
            start = col_of[j - 1] + 1 if j else 0
            called = sum(1 for ca, _ in cols[start:col_of[e] + 1] if ca == base)
            hp[min(e - j + 1, 10)][min(called, 20)] += 1
        j = e + 1
    return {"substitution": sub, "other_mismatch": other, "insertion": ins, "deletion": dele, "homopolymer": hp}


def merge(profiles):
    out = error_profile("", "", [])
    for p in profiles:
        for key, val in p.items():
            if isinstance(val, int):
                out[key] += val
            elif isinstance(val[0], list):
                out[key] = [[x + y for x, y in zip(r0, r1)] for r0, r1 in zip(out[key], val)]
            else:
                out[key] = [x + y for x, y in zip(out[key], val)]
    return out


def check_ops(read, ref, ops, E, M):
    """What every op array must satisfy whatever the tie rule: its counts are those (E, M) give, and it consumes both sequences."""
    n, m = len(read), len(ref)
    X, I, D = assess_ref.counts(n, m, E, M)
    got = np.bincount(np.asarray(ops, dtype=np.int64), minlength=4)
    assert tuple(int(v) for v in got) == (M, X, I, D), (n, m, tuple(got), (M, X, I, D))
    assert got[0] + got[1] + got[2] == n and got[0] + got[1] + got[3] == m
