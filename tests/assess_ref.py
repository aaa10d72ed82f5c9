"""Reference for the read-level assessment (chiron_align_pairs / chiron_amd.assess): what (E, M) of a pair IS, computed the slow
and obvious way.  Shares no code with the package.

Semantics: global alignment, unit costs.  E is the Levenshtein distance, M the largest number of matching columns over all
alignments of cost E.  Bases compare case-insensitively, U is T, every other character matches nothing (not even itself).

full_table: a full-table numpy DP of one 64-bit key per cell, key = E * 2^32 - M (a match adds -1, a mismatch or a gap 2^32),
row by row; the horizontal dependency of a row, row[j] = min(A[j], row[j-1] + 2^32), is a running minimum of A[j] - j * 2^32.
"""
import numpy as np

G = 1 << 32


def canon(seq):
    """str -> character codes, upper case, U as T; _match_row lets only A, C, G and T match."""
    return np.frombuffer(seq.upper().replace("U", "T").encode("latin-1"), dtype=np.uint8).astype(np.int64)


def _match_row(a_i, b):
    return (b == a_i) & np.isin(b, (65, 67, 71, 84))


def full_table(read, ref):
    """(E, M) of str read against str ref."""
    a, b = canon(read), canon(ref)
    n, m = len(a), len(b)
    j = np.arange(m + 1, dtype=np.int64)
    row = j * G
    for i in range(1, n + 1):
        diag = row[:-1] + np.where(_match_row(a[i - 1], b), -1, G)
        up = row[1:] + G
        A = np.empty(m + 1, np.int64)
        A[0] = i * G
        A[1:] = np.minimum(diag, up)
        row = np.minimum.accumulate(A - j * G) + j * G
    k = int(row[-1])
    E = (k + (G >> 1)) >> 32
    return E, E * G - k


def full_table_batch(reads, refs):
    """[(E, M)] of many short pairs at once: the same recurrence with a leading pair axis.  Sequences are padded with a
    character that matches nothing; pair p's answer is cell (n_p, m_p), taken when row n_p is complete."""
    P = len(reads)
    N, Mx = max(len(r) for r in reads), max(len(r) for r in refs)
    A_ = np.zeros((P, N), np.int64)
    B_ = np.zeros((P, Mx), np.int64)
    for p in range(P):
        A_[p, :len(reads[p])] = canon(reads[p])
        B_[p, :len(refs[p])] = canon(refs[p])
    n = np.array([len(r) for r in reads])
    m = np.array([len(r) for r in refs])
    okb = np.isin(B_, (65, 67, 71, 84))
    j = np.arange(Mx + 1, dtype=np.int64)[None, :]
    row = np.repeat(j * G, P, axis=0)
    key = np.zeros(P, np.int64)
    rows = np.arange(P)
    done = n == 0
    key[done] = row[rows[done], m[done]]
    for i in range(1, N + 1):
        diag = row[:, :-1] + np.where((B_ == A_[:, i - 1:i]) & okb, -1, G)
        up = row[:, 1:] + G
        A = np.empty((P, Mx + 1), np.int64)
        A[:, 0] = i * G
        A[:, 1:] = np.minimum(diag, up)
        row = np.minimum.accumulate(A - j * G, axis=1) + j * G
        done = n == i
        key[done] = row[rows[done], m[done]]
    E = (key + (G >> 1)) >> 32
    return [(int(e), int(e * G - k)) for e, k in zip(E, key)]


def counts(n, m, E, M):
    X = n + m - 2 * M - E
    return X, n - M - X, m - M - X


def is_match(x, y):
    x, y = x.upper().replace("U", "T"), y.upper().replace("U", "T")
    return x == y and x in "ACGT"


def exhaustive(read, ref):
    """(E, M) by enumerating every alignment (every monotone path of diagonal / down / right steps): minimum cost, then
    the maximum number of matches among the paths of that cost.  Lengths up to 5 or so."""
    n, m = len(read), len(ref)
    best = [None]

    def walk(i, j, cost, matches):
        if i == n and j == m:
            cand = (cost, -matches)
            if best[0] is None or cand < best[0]:
                best[0] = cand
            return
        if i < n and j < m:
            hit = is_match(read[i], ref[j])
            walk(i + 1, j + 1, cost + (0 if hit else 1), matches + (1 if hit else 0))
        if i < n:
            walk(i + 1, j, cost + 1, matches)
        if j < m:
            walk(i, j + 1, cost + 1, matches)

    walk(0, 0, 0, 0)
    return best[0][0], -best[0][1]


def traceback_counts(read, ref):
    """(M, X, I, D) of ONE optimal alignment under the lexicographic rule, by an explicit table and traceback in plain Python."""
    n, m = len(read), len(ref)
    T = [[None] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        for j in range(m + 1):
            if i == 0 and j == 0:
                T[i][j] = (0, 0, None)
                continue
            c = []
            if i and j:
                hit = is_match(read[i - 1], ref[j - 1])
                c.append((T[i - 1][j - 1][0] + (0 if hit else 1), T[i - 1][j - 1][1] - (1 if hit else 0), "M" if hit else "X"))
            if i:
                c.append((T[i - 1][j][0] + 1, T[i - 1][j][1], "I"))
            if j:
                c.append((T[i][j - 1][0] + 1, T[i][j - 1][1], "D"))
            T[i][j] = min(c)
    ops = {"M": 0, "X": 0, "I": 0, "D": 0}
    i, j = n, m
    while i or j:
        op = T[i][j][2]
        ops[op] += 1
        if op in "MX":
            i, j = i - 1, j - 1
        elif op == "I":
            i -= 1
        else:
            j -= 1
    return ops["M"], ops["X"], ops["I"], ops["D"]


def banded(read, ref, w):
    """The banded DP in plain Python: diagonals d = j - i in [min(0, m-n) - w, max(0, m-n) + w] only, anti-diagonal by
    anti-diagonal in ONE array indexed by d (step k rewrites the slots of k's parity in place and reads the other parity's
    neighbours).  -> (E, M, certified): certified when E <= 2w + 1 + |m-n| or the band is the whole table."""
    n, m = len(read), len(ref)
    dlo = max(min(0, m - n) - w, -n)
    dhi = min(max(0, m - n) + w, m)
    INF = 1 << 60
    row = [INF] * (dhi - dlo + 1)
    for k in range(n + m + 1):
        lo = max(dlo, -k, k - 2 * n)
        hi = min(dhi, k, 2 * m - k)
        lo += (lo + k) & 1
        for d in range(lo, hi + 1, 2):
            i, j = (k - d) // 2, (k + d) // 2
            s = d - dlo
            best = 0 if k == 0 else INF
            if i > 0 and j > 0:
                best = row[s] + (-1 if is_match(read[i - 1], ref[j - 1]) else G)
            if i > 0 and d < dhi:
                best = min(best, row[s + 1] + G)
            if j > 0 and d > dlo:
                best = min(best, row[s - 1] + G)
            row[s] = best
    key = row[(m - n) - dlo]
    E = (key + (G >> 1)) >> 32
    M = E * G - key
    full = dlo == -n and dhi == m
    return E, M, full or E <= 2 * w + 1 + abs(m - n)


def mutate(seq, rate, rng):
    """Seeded substitutions, insertions and deletions, a third of `rate` each per base."""
    out = []
    for ch in seq:
        r = rng.random()
        if r < rate / 3:
            continue
        if r < 2 * rate / 3:
            out.append("ACGT"[rng.integers(4)])
            continue
        out.append(ch)
        if r < rate:
            out.append("ACGT"[rng.integers(4)])
    return "".join(out)


def random_seq(n, rng, alphabet="ACGT"):
    return "".join(np.asarray(list(alphabet))[rng.integers(0, len(alphabet), n)]) if n else ""


def golden_read(root, k):
    with open("%s/tests/golden/example_dna/result/read%d.fastq" % (root, k)) as f:
        return f.read().split("\n")[1].strip()
