"""Inputs for the locate tests, seeded and independent of the code under test: random queries and references with breaks, and
the planted case.

The planted case (planted()).  squiggle_cases.planted(seed): its 600-base genome, its random 5-mer level table and its 30 control
reads (sample b: no planted shift), on both strands, with their own gain, offset and unlabelled head.  The table the reference is
built from is the planted one, brought to the queries' units the way a signal is: squiggle.normalise(table, "mad") -- its median
to 0 and its MAD to 256.  A read's samples are that table's levels plus noise, so the read's own normalisation of its first 1000
samples lands close to it, not on it.  truth() says where a read's sample t comes from."""
import numpy as np

import squiggle_cases
from chiron_amd import squiggle

PREFIX, SKIP, K = 1000, 0, 5
SEEDS = (1, 2, 3, 4, 5)


def random_reference(rng, R, breaks=0.0, wide=False):
    """int32 [R]: levels over all of -32767 .. 32767 (wide) or -300 .. 300, a share `breaks` of them the break value."""
    hi = 32767 if wide else 300
    e = rng.integers(-hi, hi + 1, R).astype(np.int32)
    e[rng.random(R) < breaks] = -(1 << 31)
    return e


def random_query(rng, Q, wide=False):
    hi = 32767 if wide else 300
    return rng.integers(-hi, hi + 1, Q).astype(np.int16)


def walk_query(rng, e, first, Q, noise=20, mean_dwell=3.0):
    """A query that walks the reference from column `first`: Q samples at the levels of consecutive columns with a geometric
    dwell, plus noise.  -> (int16 query, the column of its last sample).  The walk stops moving at the reference's end."""
    cols, j = [], first
    while len(cols) < Q:
        cols += [j] * int(rng.geometric(1.0 / mean_dwell))
        j = min(j + 1, len(e) - 1)
    cols = np.asarray(cols[:Q])
    x = np.clip(e[cols].astype(np.int64) + rng.integers(-noise, noise + 1, Q), -32767, 32767)
    return x.astype(np.int16), int(cols[-1])


def planted(seed=squiggle_cases.PLANTED_SEED):
    """dict(genome, table int32 [4^5] in the queries' units, k, reads [(name, raw samples)], truth [dict(reverse, pos of every base
    in signal order, true_starts)])."""
    case = squiggle_cases.planted(seed)
    table = squiggle.normalise(case["table"], "mad").astype(np.int32)
    reads, truth = [], []
    for r in case["b"]:
        n = len(r["called"])
        gs = (r["pos"] + n - 1 - np.arange(n)) if r["reverse"] else (r["pos"] + np.arange(n))
        reads.append((r["name"], r["raw"]))
        truth.append({"reverse": bool(r["reverse"]), "pos": gs, "true_starts": np.asarray(r["true_starts"], dtype=np.int64)})
    return {"genome": case["genome"], "table": table, "k": K, "reads": reads, "truth": truth}


def true_locus(truth, t):
    """(0-based genome position, strand) of the base that sample t of the read belongs to; the first base's for a sample of the
    head."""
    i = max(int(np.searchsorted(truth["true_starts"], t, side="right")) - 1, 0)
    return int(truth["pos"][i]), int(truth["reverse"])
