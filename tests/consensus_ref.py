"""Plain Python / NumPy restatement of the overlap consensus of one read, for the glue and stick kernels, written from the rules
and from nothing else:

  glue   the segment starts `prev_n - i*` after its predecessor's start, where i* is the overlap with the highest score
         2 * matches(i) - i among 1 <= i < min(floor(0.1 * prev_n), n); matches(i) counts the positions at which the segment's
         first i bases equal the predecessor's last i.  The first overlap that reaches the highest score wins, and a score has to
         be positive: otherwise i* = 0.
  stick  the segment starts `prev_n` after its predecessor's start.
  start  the running sum of these displacements; segment 0 starts at 0.
  length max(start + n) over segments 1 and later: segment 0 casts its votes but does not count, and a read of fewer than two
         segments has an empty consensus.  Votes beyond the length are dropped.
  votes  every segment, in order, adds 1 to the count of its base and its quality to that base's quality sum, column by column.
  column the base is the first of the largest counts; n1 that count; n2 the second largest count, a tie at the top counted as a
         second (so n2 == n1 there); q_top the quality sum of the LAST of the largest counts.
"""
import math

import numpy as np

_CODE = np.full(256, -1, dtype=np.int64)
_CODE[[ord(ch) for ch in "ACGT"]] = [0, 1, 2, 3]


def codes(segment):
    out = _CODE[np.frombuffer(segment.encode("ascii"), dtype=np.uint8)]
    if (out < 0).any():
        raise ValueError("a segment holds the bases A, C, G, T")
    return out


def max_overlap(prev_n, n):
    """the exclusive upper end of the overlaps glue tries"""
    return min(int(math.floor(0.1 * prev_n)), n)


def glue_scores(cur, prev):
    """-> {i: 2 * matches(i) - i} for every overlap glue tries (cur, prev: code arrays)"""
    pn = len(prev)
    return {i: 2 * int(np.count_nonzero(cur[:i] == prev[pn - i:])) - i for i in range(1, max_overlap(pn, len(cur)))}


def glue_overlap(cur, prev):
    best_i, best = 0, 0
    for i, sc in sorted(glue_scores(cur, prev).items()):
        if sc > best:
            best_i, best = i, sc
    return best_i


def displacements(segs, kernal):
    """segs: code arrays -> one displacement per segment (0 for segment 0)"""
    if kernal not in ("glue", "stick"):
        raise ValueError(kernal)
    disp = [0]
    for s in range(1, len(segs)):
        pn = len(segs[s - 1])
        disp.append(pn - (glue_overlap(segs[s], segs[s - 1]) if kernal == "glue" else 0))
    return disp


def consensus(segments, qs, kernal):
    """segments: 'ACGT' strings; qs: one float per segment, or None -> dict(start, length, counts [4, length], qsum [4, length],
    base, n1, n2 (int64 [length]), q_top (float64 [length]))."""
    segs = [codes(s) for s in segments]
    q = np.zeros(len(segs)) if qs is None else np.asarray(qs, dtype=np.float64).reshape(len(segs))
    disp = displacements(segs, kernal) if segs else []
    start = np.cumsum(disp).astype(np.int64) if segs else np.zeros(0, dtype=np.int64)
    length = max([int(start[s]) + len(segs[s]) for s in range(1, len(segs))], default=0)
    counts = np.zeros((4, length), dtype=np.int64)
    qsum = np.zeros((4, length), dtype=np.float64)
    if length:
        # one entry per base of the read, in segment order: np.add.at adds them one by one in that order
        n = np.asarray([len(seg) for seg in segs])
        owner = np.repeat(np.arange(len(segs)), n)
        col = start[owner] + (np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n))
        keep = col < length
        every = np.concatenate(segs)
        np.add.at(counts, (every[keep], col[keep]), 1)
        np.add.at(qsum, (every[keep], col[keep]), q[owner[keep]])
    ranked = np.sort(counts, axis=0)              # ascending per column
    n1, n2 = ranked[3], ranked[2]
    at_top = counts == n1[None, :]
    base = np.argmax(at_top, axis=0)              # the first base at the top
    last = 3 - np.argmax(at_top[::-1], axis=0)    # the last base at the top
    q_top = qsum[last, np.arange(length)]
    return dict(start=start, length=length, counts=counts, qsum=qsum, base=base, n1=n1, n2=n2, q_top=q_top)
