"""The definition of chiron_ctc_score (include/chiron_amd.h) restated in numpy float64: the per-frame log-softmax, the CTC forward
recurrence over the S = 2L+1 states with the repeat rule of chiron_ctc_align, lse with the maximum subtracted, the statuses.
`score_one` is the plain transcription, one candidate and one frame at a time; `score` is the batch form of
chiron_amd.polish.score (the scorer= hook), the same steps vectorised over candidates; `brute_force` sums over every path of a
tiny case.  The kernel is held to these within 1e-9 * max(1, |ref|): both sides round exp and log, a few ulp per frame."""
import itertools

import numpy as np

BLANK = 4
NEG = -np.inf
MAX_FRAMES, MAX_LABEL = 4096, 127


def log_softmax(x):
    """float32 [F, 5] -> float64 [F, 5]: (x_k - m) - log(sum_k exp(x_k - m)), the sum in class order."""
    d = np.asarray(x, dtype=np.float32).reshape(-1, 5).astype(np.float64)
    d = d - d.max(axis=1, keepdims=True)
    e = np.exp(d)
    s = (((e[:, 0] + e[:, 1]) + e[:, 2]) + e[:, 3]) + e[:, 4]
    return d - np.log(s)[:, None]


def lse(*v):
    """m + log(sum exp(v_i - m)) in the order given, elementwise; -inf where every operand is."""
    v = [np.asarray(a, dtype=np.float64) for a in v]
    m = v[0]
    for a in v[1:]:
        m = np.maximum(m, a)
    mm = np.where(np.isneginf(m), 0.0, m)
    s = np.exp(v[0] - mm)
    for a in v[1:]:
        s = s + np.exp(a - mm)
    with np.errstate(divide="ignore"):
        return mm + np.log(s)


def _classes(lab):
    L = len(lab)
    S = 2 * L + 1
    cls = np.full(S, BLANK, dtype=np.int64)
    cls[1::2] = lab
    allow2 = np.zeros(S, dtype=bool)
    if L > 1:
        allow2[3::2] = lab[1:] != lab[:-1]
    return cls, allow2


def score_one(lp, lab):
    """(loglik, status) of one candidate: lp float64 [T, 5] log-probabilities, lab codes 0..3."""
    lab = np.asarray(lab, dtype=np.uint8)
    T, L = lp.shape[0], len(lab)
    S = 2 * L + 1
    rep = int(np.count_nonzero(lab[1:] == lab[:-1])) if L > 1 else 0
    if T < L + rep:
        return NEG, 1
    if T == 0:
        return 0.0, 0
    cls, allow2 = _classes(lab)
    alpha = np.full(S, NEG)
    alpha[0] = lp[0, BLANK]
    if L >= 1:
        alpha[1] = lp[0, lab[0]]
    for t in range(1, T):
        p1 = np.concatenate([[NEG], alpha[:-1]])
        p2 = np.where(allow2, np.concatenate([[NEG, NEG], alpha[:-2]]), NEG)
        alpha = lse(alpha, p1, p2) + lp[t, cls]
    return float(lse(alpha[S - 1], alpha[S - 2]) if S >= 2 else lse(alpha[S - 1])), 0


def score(scores, items, candidates):
    """The batch form: scores float32 [frames, 5], items [(begin, end)], candidates [[label codes] per item].
    -> {"loglik": [float64 array per item], "status": [int32 array per item]}.  Vectorised over all candidates of the call, one
    frame per step, padded to the longest item and label; the steps are those of score_one."""
    lp = log_softmax(scores)
    labs = [np.asarray(l, dtype=np.uint8) for ls in candidates for l in ls]
    owner = np.array([i for i, ls in enumerate(candidates) for _ in ls], dtype=np.int64)
    C = len(labs)
    loglik, status = np.full(C, NEG), np.zeros(C, dtype=np.int32)
    if C:
        begin = np.array([items[i][0] for i in owner], dtype=np.int64)
        T = np.array([items[i][1] - items[i][0] for i in owner], dtype=np.int64)
        L = np.array([len(l) for l in labs], dtype=np.int64)
        assert T.max() <= MAX_FRAMES and L.max() <= MAX_LABEL
        Smax = 2 * int(L.max()) + 1
        cls = np.full((C, Smax), BLANK, dtype=np.int64)
        allow2 = np.zeros((C, Smax), dtype=bool)
        valid = np.arange(Smax)[None, :] < (2 * L + 1)[:, None]
        rep = np.zeros(C, dtype=np.int64)
        for c, l in enumerate(labs):
            k, a = _classes(l)
            cls[c, :len(k)], allow2[c, :len(k)] = k, a
            rep[c] = np.count_nonzero(l[1:] == l[:-1]) if len(l) > 1 else 0
        status[:] = T < L + rep
        alpha = np.full((C, Smax), NEG)
        rows = np.arange(C)
        live = (status == 0) & (T > 0)
        f0 = np.where(live, begin, 0)
        if lp.shape[0]:
            alpha[live, 0] = lp[f0[live], BLANK]
            one = live & (L >= 1)
            alpha[one, 1] = lp[f0[one], cls[one, 1]]
        pad1, pad2 = np.full((C, 1), NEG), np.full((C, 2), NEG)
        for t in range(1, int(T[live].max()) if live.any() else 0):
            on = live & (t < T)
            p1 = np.concatenate([pad1, alpha[:, :-1]], axis=1)
            p2 = np.where(allow2, np.concatenate([pad2, alpha[:, :-2]], axis=1), NEG) if Smax >= 2 else np.full((C, Smax), NEG)
            ft = np.where(on, begin + t, 0)
            new = np.where(valid, lse(alpha, p1, p2) + lp[ft[:, None], cls], NEG)
            alpha = np.where(on[:, None], new, alpha)
        last = alpha[rows, 2 * L]
        prev = np.where(L >= 1, alpha[rows, np.maximum(2 * L - 1, 0)], NEG)
        loglik = np.where(live, lse(last, prev), np.where((status == 0), 0.0, NEG))
    out_l, out_s, at = [], [], 0
    for ls in candidates:
        out_l.append(np.asarray(loglik[at:at + len(ls)], dtype=np.float64))
        out_s.append(np.asarray(status[at:at + len(ls)], dtype=np.int32))
        at += len(ls)
    return {"loglik": out_l, "status": out_s}


def brute_force(lp, lab):
    """log of the summed probability of EVERY valid state sequence (T <= 6, L <= 3); -inf when there is none."""
    T, L = lp.shape[0], len(lab)
    S = 2 * L + 1
    assert T <= 6 and L <= 3
    if T == 0:
        return 0.0 if L == 0 else NEG
    cls = [BLANK if s % 2 == 0 else int(lab[s >> 1]) for s in range(S)]
    total = 0.0
    for first in (0, 1):
        if first >= S:
            continue
        for steps in itertools.product((0, 1, 2), repeat=T - 1):
            s, logp, ok = first, lp[0, cls[first]], True
            for t, d in enumerate(steps, 1):
                n = s + d
                if n >= S or (d == 2 and not (n % 2 == 1 and lab[n >> 1] != lab[(n >> 1) - 1])):
                    ok = False
                    break
                s = n
                logp = logp + lp[t, cls[s]]
            if ok and s >= S - 2:
                total += float(np.exp(logp))
    with np.errstate(divide="ignore"):
        return float(np.log(total))


def greedy_decode(x):
    """The called sequence of a score matrix: the best class of every frame, repeats merged, blanks dropped."""
    best = np.asarray(x).reshape(-1, 5).argmax(axis=1)
    keep = np.concatenate([[True], best[1:] != best[:-1]]) & (best != BLANK)
    return best[keep].astype(np.uint8)
