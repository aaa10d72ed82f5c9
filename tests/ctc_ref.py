"""float64 numpy restatement of CTC (blank = 4, no collapsing of repeats beforehand, log-softmax over the classes of a frame):
per-row loss -log p(label | logits) and its gradient with respect to the logits, softmax - posterior.  Skipped rows (label_len >
seq_len) give 0, infeasible rows (label_len + repeats > seq_len) +inf, both with a zero gradient; frames past seq_len get 0."""
import itertools

import numpy as np

BLANK = 4


def _log_softmax(x):
    m = x.max(axis=-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))


def _lse(*v):
    v = np.stack(v)
    m = v.max(axis=0)
    safe = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.where(np.isfinite(m), safe + np.log(np.exp(v - safe).sum(axis=0)), -np.inf)


def ctc_row(x, lab):
    """x float64 [t, K] logits of the row's valid frames, lab the labels -> (loss, grad [t, K])."""
    t, K = x.shape
    lab = list(lab)
    L = len(lab)
    rep = sum(1 for i in range(1, L) if lab[i] == lab[i - 1])
    if L > t:
        return 0.0, np.zeros_like(x)
    if L + rep > t:
        return np.inf, np.zeros_like(x)
    lp = _log_softmax(x)
    if t == 0:
        return 0.0, np.zeros_like(x)
    S = 2 * L + 1
    ext = [BLANK if s % 2 == 0 else lab[s // 2] for s in range(S)]
    skip = np.array([s % 2 == 1 and s >= 3 and ext[s] != ext[s - 2] for s in range(S)])
    e = np.array(ext)
    a = np.full((t, S), -np.inf)
    a[0, 0] = lp[0, e[0]]
    if S > 1:
        a[0, 1] = lp[0, e[1]]
    for i in range(1, t):
        p = a[i - 1]
        p1 = np.concatenate([[-np.inf], p])[:S]
        p2 = np.where(skip, np.concatenate([[-np.inf, -np.inf], p])[:S], -np.inf)
        a[i] = _lse(p, p1, p2) + lp[i, e]
    ll = _lse(a[-1, -1], a[-1, -2]) if S > 1 else a[-1, -1]
    bt = np.full((t, S), -np.inf)
    bt[-1, -1] = lp[-1, e[-1]]
    if S > 1:
        bt[-1, -2] = lp[-1, e[-2]]
    skip_next = np.concatenate([skip, [False, False]])[2:]
    for i in range(t - 2, -1, -1):
        n = bt[i + 1]
        n1 = np.concatenate([n, [-np.inf]])[1:]
        n2 = np.where(skip_next, np.concatenate([n, [-np.inf, -np.inf]])[2:], -np.inf)
        bt[i] = _lse(n, n1, n2) + lp[i, e]
    post = np.exp(a + bt - lp[:, e] - ll)
    g = np.exp(lp)
    for k in range(K):
        g[:, k] -= post[:, e == k].sum(axis=1)
    return float(-ll), g


def ctc_batch(logits, seq_len, labels, label_len):
    """logits [B, T, K] -> (loss float64 [B], grad float64 [B, T, K])."""
    logits = np.asarray(logits, dtype=np.float64)
    B, T, K = logits.shape
    loss = np.zeros(B)
    grad = np.zeros((B, T, K))
    for b in range(B):
        t = int(seq_len[b])
        loss[b], grad[b, :t] = ctc_row(logits[b, :t], np.asarray(labels[b])[:int(label_len[b])])
    return loss, grad


def brute_force_loss(x, lab):
    """-log of the summed probability of every frame path that collapses (merge repeats, drop blanks) to lab."""
    x = np.asarray(x, dtype=np.float64)
    t, K = x.shape
    p = np.exp(_log_softmax(x))
    total = 0.0
    for path in itertools.product(range(K), repeat=t):
        out, prev = [], None
        for c in path:
            if c != prev and c != BLANK:
                out.append(c)
            prev = c
        if out == list(lab):
            total += np.prod([p[i, c] for i, c in enumerate(path)])
    return -np.log(total) if total > 0 else np.inf


def ctc_loss_batched(logits, seq_len, labels, label_len):
    """Loss only, the forward recursion vectorised over the rows (float64): the same numbers as ctc_batch, faster for big batches."""
    x = np.asarray(logits, dtype=np.float64)
    B, T, K = x.shape
    lp = _log_softmax(x)
    seq_len = np.asarray(seq_len)
    label_len = np.asarray(label_len)
    labels = np.asarray(labels)
    Lmax = int(label_len.max()) if B else 0
    S = 2 * Lmax + 1
    ext = np.full((B, S), BLANK)
    ext[:, 1::2] = labels[:, :Lmax] if Lmax else ext[:, 1::2]
    s_idx = np.arange(S)
    valid = s_idx[None, :] < (2 * label_len[:, None] + 1)
    skip = (s_idx[None, :] % 2 == 1) & (s_idx[None, :] >= 3)
    skip = skip & np.concatenate([np.zeros((B, 2), dtype=bool), ext[:, 2:] != ext[:, :-2]], axis=1)
    a = np.full((B, S), -np.inf)
    em = np.take_along_axis(lp[:, 0, :], ext, axis=1)
    a[:, 0] = em[:, 0]
    a[:, 1:2] = np.where(label_len[:, None] > 0, em[:, 1:2], -np.inf)
    a = np.where(valid, a, -np.inf)
    final = a.copy()
    for t in range(1, T):
        p1 = np.concatenate([np.full((B, 1), -np.inf), a[:, :-1]], axis=1)
        p2 = np.where(skip, np.concatenate([np.full((B, 2), -np.inf), a[:, :-2]], axis=1), -np.inf)
        em = np.take_along_axis(lp[:, t, :], ext, axis=1)
        nxt = np.where(valid, _lse(a, p1, p2) + em, -np.inf)
        live = (t < seq_len)[:, None]
        a = np.where(live, nxt, a)
    rows = np.arange(B)
    last = a[rows, 2 * label_len]
    prev = np.where(label_len > 0, a[rows, np.maximum(2 * label_len - 1, 0)], -np.inf)
    loss = -_lse(last, prev)
    rep = np.array([int(np.count_nonzero(labels[b, 1:label_len[b]] == labels[b, :label_len[b] - 1])) if label_len[b] > 1 else 0
                    for b in range(B)])
    loss = np.where(label_len + rep > seq_len, np.inf, loss)
    loss = np.where(seq_len == 0, np.where(label_len == 0, 0.0, loss), loss)
    return np.where(label_len > seq_len, 0.0, loss)
