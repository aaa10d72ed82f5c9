"""Inputs for the refinement tests, seeded and independent of the code under test: random items, the small cases a brute force can
enumerate, and the planted case of squiggle_cases.py with jittered borders."""
import numpy as np

import squiggle_cases

JITTER = 6


def _samples(rng, n, wide):
    lo, hi = ((-32768, 32768) if wide else (-40, 41))                    # the two sample ranges of squiggle_cases.random_set
    return rng.integers(lo, hi, n).astype(np.int16)


def _levels(rng, n, wide):
    lo, hi = ((-32767, 32768) if wide else (-40, 41))
    return rng.integers(lo, hi, n).astype(np.int32)


def item_of(rng, spans, head=0, tail=0, wide=None):
    """(samples, levels, starts) of one item whose bases have the given initial sample counts, behind `head` samples in front of
    a[0] and with `tail` samples from a[L] on; nobody may read either."""
    wide = bool(rng.integers(0, 2)) if wide is None else wide
    a = head + np.concatenate([[0], np.cumsum(np.asarray(spans, dtype=np.int64))])
    return _samples(rng, int(a[-1]) + tail, wide), _levels(rng, len(spans), wide), a.astype(np.int32)


def random_items(rng, count, max_bases=40, max_span=12, empty=0.1):
    """Items of 1 .. max_bases bases with spans of 0 .. max_span samples (a share `empty` of them empty, and now and then a run of
    empty ones, which may leave no solution), heads and tails of 0 .. 4 samples."""
    signals, levels, starts = [], [], []
    for _ in range(count):
        bases = int(rng.integers(1, max_bases + 1))
        spans = rng.integers(1, max_span + 1, bases)
        spans[rng.random(bases) < empty] = 0
        if rng.random() < 0.15:
            at = int(rng.integers(0, bases))
            spans[at:at + int(rng.integers(1, 12))] = 0
        x, e, a = item_of(rng, spans, int(rng.integers(0, 5)), int(rng.integers(0, 5)))
        signals.append(x)
        levels.append(e)
        starts.append(a)
    return signals, levels, starts


def small_case(rng, infeasible=False):
    """(x, e, a, half) small enough to enumerate: 1 .. 5 bases, half-width 1 .. 3; values from few levels so that ties occur."""
    half = int(rng.integers(1, 4))
    bases = int(rng.integers(1, 6))
    spans = rng.integers(0, 2, bases) if infeasible else rng.integers(0, 5, bases)
    wide = bool(rng.integers(0, 2))
    x, e, a = item_of(rng, spans, int(rng.integers(0, 3)), int(rng.integers(0, 3)), wide)
    if not wide:
        x, e = (x // 20).astype(np.int16), (e // 20).astype(np.int32)      # -2 .. 2: many equal costs
    return x, e, a, half


def jittered(reads, rng, by=JITTER):
    """The reads of a planted sample with every base's first sample moved by -by .. by, clipped to the signal and sorted; the
    copies share their logits arrays with the originals, so frame_aligner_of finds them."""
    out = []
    for r in reads:
        t = np.asarray(r["true_starts"], dtype=np.int64)
        moved = np.sort(np.clip(t + rng.integers(-by, by + 1, len(t)), 0, len(r["raw"]) - 1))
        out.append(dict(r, true_starts=moved.astype(np.int32)))
    return out


def planted(seed):
    """squiggle_cases.planted(seed) plus `a_jit` and `b_jit`, both samples with jittered borders."""
    case = squiggle_cases.planted(seed)
    rng = np.random.default_rng(1000 + seed)
    case["a_jit"], case["b_jit"] = jittered(case["a"], rng), jittered(case["b"], rng)
    return case
