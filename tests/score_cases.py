"""Rows for the edit-distance kernel behind Engine.score (edit_kernel, csrc/ctc_loss.hip): Myers' bit-vector recursion in words of
64 truth positions, with a horizontal carry handed from word to word.  The rows put truths on and around every word boundary up
to five words, keep hypotheses one or two edits away from their truth (a small distance: every carry counts, none saturates),
and sit at the edges of the kernel's 64-row blocks.  tests/test_score_cases_cpu.py proves with plain dynamic programming that
every row is what its name says; tests/test_gpu_ctc.py runs them.

A row is (name, hyp, truth): two lists of labels 0..3.  claims() gives, per name, the closed interval the row's Levenshtein
distance lies in by construction -- one number wherever the construction decides it."""
import functools

import numpy as np

LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320)
LMAX = 320
# rows that hold a designed, non-empty hypothesis / an empty hypothesis, whatever the batch size (negative: from the end)
PINNED_DESIGNED = (0, 63, 64, 127, 128, -1)
PINNED_EMPTY_HYP = (1, -2)
N_FILLER = 8


def _other(rng, *avoid):
    """A label 0..3 that is none of `avoid` (at most three distinct values)."""
    free = [c for c in range(4) if c not in avoid]
    return int(free[int(rng.integers(0, len(free)))])


def _no_repeat(rng, n):
    """n labels, no two neighbours equal."""
    out = [int(rng.integers(0, 4))]
    while len(out) < n:
        out.append(_other(rng, out[-1]))
    return out[:n]


def _word_edges(m):
    """truth indices 63, 64, 127, 128, ... below m: the last position of a word and the first of the next"""
    return [i for w in range(64, m + 64, 64) for i in (w - 1, w) if i < m]


def _substituted(rng, seq, at, keep_no_repeat=False):
    out = list(seq)
    for i in at:
        avoid = [seq[i]]
        if keep_no_repeat:
            avoid += [out[i - 1]] if i > 0 else []
            avoid += [out[i + 1]] if i + 1 < len(out) else []
        out[i] = _other(rng, *avoid)
    return out


@functools.lru_cache(maxsize=None)
def _build(T):
    if T < 400:
        raise ValueError("the rows need 400 frames: a truth of %d labels, hypotheses of up to 200 bases with a blank between" % LMAX)
    half = T // 2
    rng = np.random.default_rng(20241)
    rows, claim = [], {}

    def add(name, hyp, truth, lo, hi=None):
        assert name not in claim
        rows.append((name, [int(v) for v in hyp], [int(v) for v in truth]))
        claim[name] = (int(lo), int(lo if hi is None else hi))

    for m in LENGTHS:
        truth = {1: [2], 2: [0, 1]}.get(m) or [int(v) for v in rng.integers(0, 4, m)]
        edges = _word_edges(m)
        if m <= half:
            add("exact_m%d" % m, truth, truth, 0)
            add("del_first_m%d" % m, truth[1:], truth, 1)
            add("ins_first_m%d" % m, [_other(rng, truth[0])] + truth, truth, 1)
            add("sub_word_edges_m%d" % m, _substituted(rng, truth, edges), truth, len(edges))
            # the truth moved by one position: two edits (one for the single base, whose replacement differs from it)
            add("del_first_ins_last_m%d" % m, truth[1:] + [_other(rng, truth[-1], truth[0])], truth, 1 if m == 1 else 2)
        else:
            # the hypothesis holds at most T / 2 bases: a contiguous piece of the truth costs exactly the bases it lacks, and
            # an edit on it costs at most one more
            add("exact_m%d" % m, truth[:half], truth, m - half)
            for tag, o in (("head", 0), ("tail", m - half)):
                w = truth[o:o + half]
                inside = [i - o for i in edges if o <= i < o + half]
                before = [truth[o - 1]] if o > 0 else []
                add("del_first_m%d_%s" % (m, tag), w[1:], truth, m - half + 1)
                add("ins_first_m%d_%s" % (m, tag), [_other(rng, w[0], *before)] + w[:half - 1], truth, m - half, m - half + 2)
                add("sub_word_edges_m%d_%s" % (m, tag), _substituted(rng, w, inside), truth, m - half, m - half + len(inside))
                add("del_first_ins_last_m%d_%s" % (m, tag), w[1:] + [_other(rng, w[-1])], truth, m - half, m - half + 2)
        n = min(m, half)
        add("unrelated_m%d" % m, rng.integers(0, 4, n), truth, m - n, m)
    # five words with a SMALL distance: a hypothesis of more than T / 2 bases has to be free of adjacent repeats (one frame each)
    for m in (257, 320):
        truth = _no_repeat(rng, m)
        add("norepeat_del_first_m%d" % m, truth[1:], truth, 1)
        at = [63, 64, m - 1]
        add("norepeat_sub_m%d" % m, _substituted(rng, truth, at, keep_no_repeat=True), truth, len(at))
    # one symbol against one or two: the distance is the length difference, plus every truth position of the other symbol
    for m, ns in ((128, (100, 135)), (192, (164, 199)), (256, (150, half))):
        for n in ns:
            add("homopolymer_m%d_n%d" % (m, n), [0] * n, [0] * m, abs(m - n))
            add("period2_m%d_n%d" % (m, n), [0] * n, [0, 1] * (m // 2), max(m // 2, abs(m - n)), max(m, n))
    # n much larger than m: T bases, one per frame, with the truth as an infix
    for m in (65, 129):
        hyp = _no_repeat(rng, T)
        o = (T - m) // 3
        add("infix_m%d_n%d" % (m, T), hyp, hyp[o:o + m], T - m)
    for m in (1, 64, 65, 320):
        add("empty_hyp_m%d" % m, [], rng.integers(0, 4, m), m)
    add("empty_truth", rng.integers(0, 4, 40), [], 40)          # the kernel's answer is +inf: tf.edit_distance divides by 0
    add("both_empty", [], [], 0)
    for k in range(N_FILLER):
        n, m = int(rng.integers(20, 61)), int(rng.integers(20, 61))
        add("filler%d" % k, rng.integers(0, 4, n), rng.integers(0, 4, m), abs(m - n), max(m, n))

    # ---- the order: designed rows at the corners of the 64-row blocks, empty hypotheses next to both ends
    by_name = {r[0]: r for r in rows}
    pinned = ["norepeat_del_first_m320", "del_first_m193", "ins_first_m129", "sub_word_edges_m192", "del_first_ins_last_m128",
              "norepeat_sub_m257"]
    pinned_empty = ["empty_hyp_m320", "empty_hyp_m65"]
    B = len(rows)
    assert B > 130
    order = [None] * B
    for at, name in list(zip(PINNED_DESIGNED, pinned)) + list(zip(PINNED_EMPTY_HYP, pinned_empty)):
        order[at % B] = by_name[name]
    rest = iter(r for r in rows if r[0] not in pinned + pinned_empty)
    order = [r if r is not None else next(rest) for r in order]
    return tuple(order), claim


def edit_cases(T=400):
    """The rows, in batch order."""
    return list(_build(T)[0])


def claims(T=400):
    """name -> (lo, hi): the distance the row has by construction."""
    return dict(_build(T)[1])


def dense_truths(rows, lmax=LMAX):
    """-> (labels int32 [B, lmax] zero padded, label_len int32 [B])"""
    labels = np.zeros((len(rows), lmax), dtype=np.int32)
    ll = np.zeros(len(rows), dtype=np.int32)
    for b, (_, _, truth) in enumerate(rows):
        labels[b, :len(truth)] = truth
        ll[b] = len(truth)
    return labels, ll


def levenshtein_rows(a, b):
    """ctc.levenshtein's recurrence with one row of the table per NumPy statement (the plain form takes seconds on a batch):
    vertical and diagonal steps elementwise, then the horizontal steps cur[j] = min(cur[j], cur[j - 1] + 1) as a running minimum
    of cur[j] - j.  tests/test_score_cases_cpu.py holds it to the plain form on every row."""
    b = np.asarray(b, dtype=np.int64)
    ramp = np.arange(len(b) + 1)
    prev = ramp.copy()
    for i, ai in enumerate(a, 1):
        cur = np.empty_like(prev)
        cur[0] = i
        cur[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (b != ai))
        prev = np.minimum.accumulate(cur - ramp) + ramp
    return int(prev[-1])


def normalized(hyps, labels, label_len):
    """tf.edit_distance(..., normalize=True) per row, as ctc.edit_distance computes it: float32(d) / float32(m); an empty truth
    gives 0 against an empty hypothesis and +inf otherwise."""
    out = np.empty(len(hyps), dtype=np.float32)
    for r, hyp in enumerate(hyps):
        m = int(label_len[r])
        d = levenshtein_rows(hyp, labels[r, :m])
        out[r] = np.float32(d) / np.float32(m) if m else (np.float32(0) if not hyp else np.float32(np.inf))
    return out


def greedy_logits(hyps, T):
    """Logits [len(hyps), T, 5] whose greedy decode is `hyps`: blank 4.0 and every base -4.0 in every frame, then 6.0 for base i of
    a hypothesis at frame 2i (a blank frame parts neighbours, so repeats survive).  A hypothesis of more than T / 2 bases takes
    one frame per base from frame 0 on and must hold no adjacent repeat: the decoder would merge it."""
    lg = np.full((len(hyps), T, 5), -4.0, dtype=np.float32)
    lg[:, :, 4] = 4.0
    for r, hyp in enumerate(hyps):
        n = len(hyp)
        if n > T:
            raise ValueError("a hypothesis of %d bases does not fit %d frames" % (n, T))
        step = 2 if 2 * n <= T else 1
        if step == 1 and any(a == b for a, b in zip(hyp, hyp[1:])):
            raise ValueError("a hypothesis of more than T / 2 bases must not repeat a base")
        for i, c in enumerate(hyp):
            lg[r, step * i, c] = 6.0
    return lg
