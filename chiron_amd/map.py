"""Read mapping: where in a genome does each called read lie, and which stretch of it does the read cover?

`assess` and `label` need a reference sequence per read.  A run that has reads and a genome gets them here: seed
(chiron_seed_reads, csrc/seed.hip) and align (chiron_align_infix, csrc/map.hip) on the GPU, cut the covered stretch out.  `chiron map` writes the cut-outs as
reference/<read>_ref.fasta, which `assess -r` and `label -r` take unchanged, a PAF file and a JSON report.  With `--cigar` every
mapped read is also traced against the stretch it covers (assess.align_ops, csrc/trace.hip), in genome orientation: the PAF lines
gain a cg:Z: tag and mapped.sam is written.

The seeding rule is host-side numpy (`vote`), deterministic and shared by the command and the tests; `vote_reads` is the same
rule on the GPU, equal to it field for field, and what the commands run unless they are told `seed="host"`:
  genome   the contigs (assess.read_records, assess.encode) concatenated with runs of code 4 between them; a k-mer that holds a
           code 4 is never indexed, so none spans two contigs.
  index    k = 15, 2 bits per base; a stable argsort of the k-mer codes and their positions.  K-mers that occur more than
           max_occ times are dropped.
  votes    each read as given and as its reverse complement: every read k-mer is looked up with searchsorted; a hit at genome
           position g and read position r votes for the diagonal delta = g - r (concatenated coordinates), binned by
           delta // 256 (floor).  The score of a bin beta that holds a hit is count(beta) + count(beta + 1); the best score wins,
           ties to forward before reverse, then to the smaller beta.  The candidate delta* is the lower median of the hits of the
           winning two bins, ordered by (delta, g); the contig is the one that holds that hit's g.  Below min_votes the read is
           unmapped.  votes_second is the best score of the other strand or of a bin more than n // 256 + 2 away: with one
           candidate a read it is reported, never acted on (it is no mapping quality -- the two scores count seeds, not
           alignments).
  top-K    `vote_top` (on the GPU `vote_reads_top`, chiron_seed_candidates) picks up to K (strand, bin) pairs a read, each
           suppressing its neighbourhood; map_reads(candidates=K) aligns those with enough votes in the same launches, keeps the
           best alignment and derives a mapping quality from the two best edit distances: an ordering, not a calibrated
           probability, with defaults that are not tuned on real reads.  K = 1, the default, is the single-candidate path.
  window   [delta* - slack, delta* + n + slack) clipped to the contig, slack = max(256, n // 8).
  edge     a match that touches a window edge which is not a contig edge (s = 0, or e = m while the contig goes on) may continue
           outside: the read's slack doubles and it is aligned again in a follow-up launch, at most three times; then `edge`.
There is no CPU fallback: without the library or a GPU, align_infix and vote_reads raise.
"""
import json
import os

import numpy as np

from . import _lib, assess

K = 15
BIN = 256
SEPARATOR = K                           # code-4 bases between two contigs
MAX_WIDENINGS = 3
MIN_VOTES, MAX_OCC = 4, 64
MAPQ_MAX = 60                           # the mapq of a read with one mapped candidate; 255 in a file is "not available"
THREADS = _lib.INFIX_THREADS
LDS_SLOTS = _lib.INFIX_LDS_SLOTS
BAND0 = _lib.INFIX_BAND0
MAX_READ, MAX_WINDOW = _lib.INFIX_MAX_READ, _lib.INFIX_MAX_WINDOW

INFIX_DTYPE = np.dtype([("edit", np.int32), ("match", np.int32), ("start", np.int32), ("end", np.int32), ("band", np.int32)])
_LETTERS = np.frombuffer(b"ACGTN", dtype=np.uint8)


def decode(codes):
    return _LETTERS[codes].tobytes().decode("ascii")


# ----------------------------------------------------------------------------------------------------------------------------
# the kernel
# ----------------------------------------------------------------------------------------------------------------------------
def workspace_size(pairs, max_read, max_window):
    return _lib.sized("chiron_align_infix_workspace_size", pairs, max_read, max_window)


def align_infix(reads, windows, band0=BAND0, device_id=0):
    """Align reads[p] against the best substring of windows[p] (str, bytes or uint8 code arrays) on the GPU, all pairs in one
    launch.  -> structured array (INFIX_DTYPE): edit, match, start, end (offsets into the window), band."""
    if len(reads) != len(windows):
        raise ValueError("%d reads against %d windows" % (len(reads), len(windows)))
    pairs = len(reads)
    out = np.zeros(pairs, dtype=INFIX_DTYPE)
    if pairs == 0:
        return out
    a = [assess.encode(s) for s in reads]
    b = [assess.encode(s) for s in windows]
    codes, lens_a, lens_b, read_off, win_off = _lib.pack_pairs(a, b)
    lib, ws, stream = _lib.device_workspace(lambda: workspace_size(pairs, int(lens_a.max()), int(lens_b.max())), device_id,
                                            "map.align_infix", "alignment")
    res = [np.zeros(pairs, dtype=np.int32) for _ in range(5)]
    _lib.check(lib.chiron_align_infix(device_id, codes.ctypes.data, read_off.ctypes.data, win_off.ctypes.data, pairs, band0, 0,
                                      res[0].ctypes.data, res[1].ctypes.data, res[2].ctypes.data, res[3].ctypes.data,
                                      res[4].ctypes.data, ws.data_ptr(), stream))
    del ws
    out["edit"], out["match"], out["start"], out["end"], out["band"] = res
    return out


def plan_batches(read_lens, win_lens, budget_bytes):
    """Consecutive pairs grouped so that each group's workspace stays within the budget (a single pair always forms a group)."""
    batches, cur, mr, mw = [], [], 0, 0
    for i, (n, m) in enumerate(zip(read_lens, win_lens)):
        nr, nw = max(mr, n), max(mw, m)
        if cur and workspace_size(len(cur) + 1, nr, nw) > budget_bytes:
            batches.append(cur)
            cur, nr, nw = [], n, m
        cur.append(i)
        mr, mw = nr, nw
    if cur:
        batches.append(cur)
    return batches


def align_in_batches(reads, windows, band0=BAND0, workspace_mb=4096, device_id=0):
    import torch  # noqa: F401  before plan_batches loads the library: torch's ROCm runtime has to come up first (_lib.py)
    out = np.zeros(len(reads), dtype=INFIX_DTYPE)
    for batch in plan_batches([len(r) for r in reads], [len(w) for w in windows], workspace_mb << 20):
        out[batch] = align_infix([reads[i] for i in batch], [windows[i] for i in batch], band0, device_id)
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# genome, index, votes
# ----------------------------------------------------------------------------------------------------------------------------
class Genome:
    """Contigs concatenated into one code array, SEPARATOR code-4 bases between neighbours."""

    def __init__(self, records):
        self.names = [name for name, _ in records]
        seqs = [assess.encode(seq) for _, seq in records]
        self.lengths = np.array([len(s) for s in seqs], dtype=np.int64)
        self.starts = np.zeros(len(seqs), dtype=np.int64)
        parts, at = [], 0
        for c, s in enumerate(seqs):
            if c:
                parts.append(np.full(SEPARATOR, 4, np.uint8))
                at += SEPARATOR
            self.starts[c] = at
            parts.append(s)
            at += len(s)
        self.codes = np.concatenate(parts) if parts else np.zeros(0, np.uint8)

    def contig_of(self, g):
        """The contig that holds concatenated position g (a separator position counts to the contig before it)."""
        return int(np.searchsorted(self.starts, g, side="right") - 1)


def load_genome(path):
    records = assess.read_records(path)
    if not records:
        raise ValueError("%s holds no sequence" % path)
    return Genome(records)


def kmers(codes, k=K):
    """(k-mer codes, positions) of every k-mer of `codes` that holds no code above 3: 2 bits per base, first base highest."""
    n = len(codes) - k + 1
    if n <= 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    bad = np.concatenate([[0], np.cumsum(codes > 3)])
    ok = (bad[k:] - bad[:-k]) == 0
    val = np.zeros(n, dtype=np.int64)
    c = codes.astype(np.int64) & 3
    for t in range(k):
        val = (val << 2) | c[t:t + n]
    pos = np.nonzero(ok)[0].astype(np.int64)
    return val[pos], pos


def build_index(codes, k=K, max_occ=MAX_OCC):
    """-> (sorted k-mer codes, their genome positions); equal k-mers keep their positions in rising order (stable sort)."""
    val, pos = kmers(codes, k)
    order = np.argsort(val, kind="stable")
    val, pos = val[order], pos[order]
    if len(val):
        first = np.searchsorted(val, val, side="left")
        last = np.searchsorted(val, val, side="right")
        keep = (last - first) <= max_occ
        val, pos = val[keep], pos[keep]
    return val, pos


def hits(index, read_codes, k=K):
    """(delta, g) of every seed hit of the read against the index."""
    idx_val, idx_pos = index
    rv, rp = kmers(read_codes, k)
    lo = np.searchsorted(idx_val, rv, side="left")
    cnt = np.searchsorted(idx_val, rv, side="right") - lo
    total = int(cnt.sum())
    if total == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    which = np.repeat(np.arange(len(rv)), cnt)
    within = np.arange(total) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    g = idx_pos[lo[which] + within]
    return g - rp[which], g


def bin_scores(delta):
    """-> (bins that hold a hit, rising; score of each = its count + the count of the next bin up)."""
    bins, cnt = np.unique(delta // BIN, return_counts=True)          # floor division: negative diagonals bin downwards
    score = cnt.copy()
    if len(bins) > 1:
        nxt = bins[1:] == bins[:-1] + 1
        score[:-1] += np.where(nxt, cnt[1:], 0)
    return bins, score


def vote(index, read_codes, k=K):
    """The seeding decision for one read.  -> dict(votes, votes_second, strand, delta, g) -- delta and g None without a hit."""
    n = len(read_codes)
    per = []
    for strand, codes in (("forward", read_codes), ("reverse", assess.reverse_complement(read_codes))):
        delta, g = hits(index, codes, k)
        bins, score = bin_scores(delta) if len(delta) else (np.zeros(0, np.int64), np.zeros(0, np.int64))
        per.append((strand, delta, g, bins, score))
    best = [int(p[4].max()) if len(p[4]) else 0 for p in per]
    w = 1 if best[1] > best[0] else 0                                   # forward wins a tie
    strand, delta, g, bins, score = per[w]
    out = {"votes": best[w], "votes_second": best[1 - w], "strand": strand, "delta": None, "g": None}
    if best[w] == 0:
        return out
    beta = int(bins[int(np.argmax(score))])                              # the first maximum: the smaller beta
    far = np.abs(bins - beta) > n // BIN + 2
    if far.any():
        out["votes_second"] = max(out["votes_second"], int(score[far].max()))
    b = delta // BIN
    sel = np.nonzero((b == beta) | (b == beta + 1))[0]
    order = np.lexsort((g[sel], delta[sel]))
    mid = sel[order[(len(sel) - 1) // 2]]
    out["delta"], out["g"] = int(delta[mid]), int(g[mid])
    return out


def vote_top(index, read_codes, max_cand, min_score=1, k=K):
    """Up to max_cand seeding candidates of one read, best first: the definition of chiron_seed_candidates.  Bins and scores are
    those of `vote` (bin_scores on both strands).  Greedily: among the (strand, bin) pairs that hold a hit and are not
    suppressed, the largest score, ties to forward, then to the smaller bin; stop when nothing is left, when that score is below
    min_score, or after max_cand picks.  A pick at bin beta suppresses the bins b of its own strand with |b - beta| <= n // BIN + 2
    (the complement of `vote`'s "far"), and its (delta, g) is `vote`'s lower median over the hits of bins beta and beta + 1; the
    radius is at least 2, so no two picks share a bin.  Pick 0 is `vote`'s candidate and pick 1's votes are its votes_second.
    -> [dict(votes, strand, delta, g)] in pick order."""
    n = len(read_codes)
    reach = n // BIN + 2
    per = []
    for strand, codes in (("forward", read_codes), ("reverse", assess.reverse_complement(read_codes))):
        delta, g = hits(index, codes, k)
        bins, score = bin_scores(delta) if len(delta) else (np.zeros(0, np.int64), np.zeros(0, np.int64))
        per.append((strand, delta, g, bins, score.astype(np.int64), np.ones(len(bins), bool)))
    picks = []
    while len(picks) < max_cand:
        best = [int(np.where(p[5], p[4], 0).max()) if len(p[4]) else 0 for p in per]     # a bin that holds a hit scores at least 1
        w = 1 if best[1] > best[0] else 0                                                 # forward wins a tie
        if best[w] < max(min_score, 1):
            break
        strand, delta, g, bins, score, free = per[w]
        beta = int(bins[int(np.argmax(np.where(free, score, 0)))])                        # the first maximum: the smaller beta
        free &= np.abs(bins - beta) > reach
        b = delta // BIN
        sel = np.nonzero((b == beta) | (b == beta + 1))[0]
        order = np.lexsort((g[sel], delta[sel]))
        mid = sel[order[(len(sel) - 1) // 2]]
        picks.append({"votes": best[w], "strand": strand, "delta": int(delta[mid]), "g": int(g[mid])})
    return picks


# ----------------------------------------------------------------------------------------------------------------------------
# the votes on the GPU
# ----------------------------------------------------------------------------------------------------------------------------
SEEDS = ("gpu", "host")
DEFAULT_SEED = "gpu"                    # what the commands run; "host" is the per-read numpy `vote`


def seed_workspace_size(n_index, genome_len, reads, max_read, total_bases):
    return _lib.sized("chiron_seed_workspace_size", n_index, genome_len, reads, max_read, total_bases)


def seed_candidates_workspace_size(n_index, genome_len, reads, max_read, total_bases, max_cand):
    return _lib.sized("chiron_seed_candidates_workspace_size", n_index, genome_len, reads, max_read, total_bases, max_cand)


def plan_seed_batches(read_lens, n_index, genome_len, budget_bytes, max_cand=None):
    """Consecutive reads grouped so that each group's workspace stays within the budget (a single read always forms a group).
    max_cand: plan for chiron_seed_candidates with that many candidates instead of chiron_seed_reads."""
    def size(*args):
        return seed_workspace_size(*args) if max_cand is None else seed_candidates_workspace_size(*args, max_cand)
    batches, cur, mr, total = [], [], 0, 0
    for i, n in enumerate(read_lens):
        nr, nt = max(mr, n), total + n
        if cur and size(n_index, genome_len, len(cur) + 1, nr, nt) > budget_bytes:
            batches.append(cur)
            cur, nr, nt = [], n, n
        cur.append(i)
        mr, total = nr, nt
    if cur:
        batches.append(cur)
    return batches


def seed_reads(idx_val, idx_pos, genome_len, reads, device_id=0):
    """One call of chiron_seed_reads: idx_val uint32 and idx_pos int32 (sorted by value), reads a list of uint8 code arrays.
    -> (votes, votes_second, strand as 0 / 1: int32 arrays; delta, g: int64 arrays)."""
    count = len(reads)
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    read_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    codes = np.ascontiguousarray(np.concatenate(list(reads) + [np.zeros(1, np.uint8)]))
    res = [np.zeros(count, dtype=np.int32) for _ in range(3)] + [np.zeros(count, dtype=np.int64) for _ in range(2)]
    if count == 0:
        return res
    lib, ws, stream = _lib.device_workspace(lambda: seed_workspace_size(len(idx_val), genome_len, count, int(lens.max()), int(lens.sum())),
                                            device_id, "map.vote_reads", "seeding")
    _lib.check(lib.chiron_seed_reads(device_id, idx_val.ctypes.data, idx_pos.ctypes.data, len(idx_val), genome_len, codes.ctypes.data,
                                     read_off.ctypes.data, count, 0, *[r.ctypes.data for r in res], ws.data_ptr(), stream))
    del ws
    return res


def vote_reads(index, reads, workspace_mb=4096, device_id=0):
    """`vote` of every read, on the GPU: [vote(index, r) for r in reads], field for field.  The index goes to the device as
    uint32 values and int32 positions; consecutive reads share a call while the call's workspace stays within workspace_mb."""
    import torch  # noqa: F401  before the library loads: torch's ROCm runtime has to come up first (_lib.py)
    idx_val, idx_pos = index
    genome_len = int(idx_pos.max()) + K if len(idx_pos) else 0             # the shortest genome that holds every indexed k-mer
    reads = [assess.encode(r) for r in reads]
    lens = [len(r) for r in reads]
    batches = plan_seed_batches(lens, len(idx_val), genome_len, int(workspace_mb * (1 << 20)))   # refuses an oversized genome first
    val32, pos32 = np.ascontiguousarray(idx_val, dtype=np.uint32), np.ascontiguousarray(idx_pos, dtype=np.int32)
    out = []
    for batch in batches:
        votes, second, strand, delta, g = seed_reads(val32, pos32, genome_len, [reads[i] for i in batch], device_id)
        for v, s, w, d, at in zip(votes.tolist(), second.tolist(), strand.tolist(), delta.tolist(), g.tolist()):
            out.append({"votes": v, "votes_second": s, "strand": "reverse" if w else "forward", "delta": d if v else None,
                        "g": at if v else None})
    return out


def seed_candidates(idx_val, idx_pos, genome_len, reads, max_cand, min_score=1, device_id=0):
    """One call of chiron_seed_candidates; operands as for seed_reads.  -> (count int32 [reads]; votes, strand int32 and delta, g
    int64, each [reads, max_cand], zeros from a read's count on)."""
    count = len(reads)
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    read_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    codes = np.ascontiguousarray(np.concatenate(list(reads) + [np.zeros(1, np.uint8)]))
    res = [np.zeros(count, dtype=np.int32)] + [np.zeros((count, max_cand), dtype=t) for t in (np.int32, np.int32, np.int64, np.int64)]
    if count == 0:
        return res
    lib, ws, stream = _lib.device_workspace(
        lambda: seed_candidates_workspace_size(len(idx_val), genome_len, count, int(lens.max()), int(lens.sum()), max_cand),
        device_id, "map.vote_reads_top", "seeding")
    _lib.check(lib.chiron_seed_candidates(device_id, idx_val.ctypes.data, idx_pos.ctypes.data, len(idx_val), genome_len, codes.ctypes.data,
                                          read_off.ctypes.data, count, max_cand, min_score, 0, *[r.ctypes.data for r in res],
                                          ws.data_ptr(), stream))
    del ws
    return res


def vote_reads_top(index, reads, max_cand, min_score=1, workspace_mb=4096, device_id=0):
    """`vote_top` of every read, on the GPU: [vote_top(index, r, max_cand, min_score) for r in reads], field for field; batches
    as in vote_reads, planned with chiron_seed_candidates_workspace_size."""
    import torch  # noqa: F401  before the library loads: torch's ROCm runtime has to come up first (_lib.py)
    idx_val, idx_pos = index
    genome_len = int(idx_pos.max()) + K if len(idx_pos) else 0
    reads = [assess.encode(r) for r in reads]
    batches = plan_seed_batches([len(r) for r in reads], len(idx_val), genome_len, int(workspace_mb * (1 << 20)), max_cand)
    val32, pos32 = np.ascontiguousarray(idx_val, dtype=np.uint32), np.ascontiguousarray(idx_pos, dtype=np.int32)
    out = []
    for batch in batches:
        count, votes, strand, delta, g = seed_candidates(val32, pos32, genome_len, [reads[i] for i in batch], max_cand, min_score, device_id)
        for c, v, w, d, at in zip(count.tolist(), votes.tolist(), strand.tolist(), delta.tolist(), g.tolist()):
            out.append([{"votes": v[k], "strand": "reverse" if w[k] else "forward", "delta": d[k], "g": at[k]} for k in range(c)])
    return out


def seeder_of(seed, workspace_mb=4096, device_id=0):
    """The `seeder` of map_reads for a command's --seed: None (the per-read host `vote`) for "host", vote_reads for "gpu"."""
    if seed not in SEEDS:
        raise ValueError("seed must be one of %s, not %r" % (", ".join(SEEDS), seed))
    if seed == "host":
        return None
    return lambda index, reads: vote_reads(index, reads, workspace_mb, device_id)


def top_seeder_of(seed, workspace_mb=4096, device_id=0):
    """The `top_seeder` of map_reads for a command's --seed: None (the per-read host `vote_top`) or vote_reads_top."""
    if seed not in SEEDS:
        raise ValueError("seed must be one of %s, not %r" % (", ".join(SEEDS), seed))
    if seed == "host":
        return None
    return lambda index, reads, max_cand, min_score: vote_reads_top(index, reads, max_cand, min_score, workspace_mb, device_id)


# ----------------------------------------------------------------------------------------------------------------------------
# the pipeline
# ----------------------------------------------------------------------------------------------------------------------------
def window_of(genome, contig, delta, n, slack):
    """[lo, hi) in concatenated coordinates: [delta - slack, delta + n + slack) clipped to the contig."""
    c0 = int(genome.starts[contig])
    c1 = c0 + int(genome.lengths[contig])
    lo = min(max(delta - slack, c0), c1)
    hi = max(min(delta + n + slack, c1), lo)
    return lo, hi


def mapq_of(edits):
    """The mapping quality of a read from the edit distances of its mapped candidates: 60 with one; with E1 <= E2 the two
    smallest, min(60, 600 * (E2 - E1) // max(E2, 1)); 0 with none.  An ordering, not a calibrated probability."""
    if not edits:
        return 0
    if len(edits) == 1:
        return MAPQ_MAX
    e1, e2 = sorted(edits)[:2]
    return min(MAPQ_MAX, 600 * (e2 - e1) // max(e2, 1))


def candidates_of(picks, min_votes, second_ratio):
    """The picks of a read (vote_top order) that are aligned: votes >= min_votes and >= ceil(second_ratio * votes of pick 0)."""
    if not picks:
        return []
    floor = int(np.ceil(second_ratio * picks[0]["votes"]))
    return [(rank, p) for rank, p in enumerate(picks) if p["votes"] >= min_votes and p["votes"] >= floor]


def choose(cands):
    """cands: a read's aligned candidates in rank order, dicts with rank, contig, strand, start, end, edit, match, status.  Drops
    as a duplicate every candidate whose interval overlaps that of an earlier-ranked kept one on the same contig and strand;
    -> (the primary: the mapped one with the smallest (edit, -match, rank), or None; mapq; the second-smallest edit among the
    mapped ones, or None)."""
    kept = []
    for c in cands:
        if not any(k["contig"] == c["contig"] and k["strand"] == c["strand"] and c["start"] < k["end"] and k["start"] < c["end"] for k in kept):
            kept.append(c)
    good = sorted((c for c in kept if c["status"] == "mapped"), key=lambda c: (c["edit"], -c["match"], c["rank"]))
    if not good:
        return None, 0, None
    return good[0], mapq_of([c["edit"] for c in good]), good[1]["edit"] if len(good) > 1 else None


def map_reads(reads, genome, min_votes=MIN_VOTES, max_occ=MAX_OCC, band=BAND0, workspace_mb=4096, device_id=0, aligner=None,
              seeds=None, index=None, seeder=None, candidates=1, second_ratio=0.5, top_seeder=None):
    """Map {name: sequence} against a Genome.  aligner(reads, windows, band0) -> INFIX_DTYPE rows replaces the GPU kernel
    (the tests' reference pipeline); seeds {name: dict(strand, delta, contig)} replaces the voting for those reads (a test
    hook); seeder(index, [codes]) -> [vote dicts] replaces the per-read host `vote` for the others (seeder_of).  -> dict(reads=[per-read records, name order], references={name: cut-out in the read's orientation}, totals,
    unmapped=[names]).

    candidates > 1: every read's picks of top_seeder(index, [codes], candidates, min_score) -> [pick lists] (top_seeder_of; None
    is the per-read host vote_top) that pass candidates_of go through the window and widening loop together, in the same
    launches, and `choose` names the primary.  The record is the primary's (pick 0's when none mapped) and gains mapq,
    candidates (the number aligned), edit_second and seed_rank; its votes are pick 0's and its votes_second pick 1's (0 below
    min_votes).  A read without a pick of min_votes gets the single-candidate record, from `seeder`.  The result gains
    `ambiguity`: the reads at mapq 0, 1 .. 59 and 60 and those won by a pick other than 0."""
    if candidates < 1 or candidates > _lib.SEED_MAX_CANDIDATES:
        raise ValueError("candidates must be 1 .. %d, not %r" % (_lib.SEED_MAX_CANDIDATES, candidates))
    if not 0.0 <= second_ratio <= 1.0:
        raise ValueError("second_ratio must be within 0 .. 1, not %r" % (second_ratio,))
    if aligner is None:
        def aligner(rs, ws, band0):
            return align_in_batches(rs, ws, band0, workspace_mb, device_id)
    if index is None:
        index = build_index(genome.codes, K, max_occ)
    recs, todo = {}, []
    coded = {name: assess.encode(reads[name]) for name in sorted(reads)}
    voting = [name for name in coded if seeds is None or name not in seeds]
    picked = {}
    if candidates > 1:
        min_score = max(1, min_votes)
        tops = (top_seeder(index, [coded[name] for name in voting], candidates, min_score) if top_seeder is not None else
                [vote_top(index, coded[name], candidates, min_score) for name in voting])
        picked = {name: picks for name, picks in zip(voting, tops) if picks}
        voting = [name for name in voting if name not in picked]
    voted = dict(zip(voting, seeder(index, [coded[name] for name in voting]) if seeder is not None else
                     (vote(index, coded[name]) for name in voting)))
    several = {}                                                              # name -> its candidates' records, rank order
    for name, codes in coded.items():
        n = len(codes)
        rec = {"name": name, "read_len": n, "contig": None, "start": None, "end": None, "strand": None, "edit": None, "match": None,
               "mismatch": None, "insertion": None, "deletion": None, "identity": None, "votes": 0, "votes_second": 0, "band": None,
               "widenings": 0, "status": "unmapped"}
        recs[name] = rec
        if name in picked:
            picks = picked[name]
            rec["votes"], rec["votes_second"] = picks[0]["votes"], picks[1]["votes"] if len(picks) > 1 else 0
            several[name] = []
            for rank, v in candidates_of(picks, min_votes, second_ratio):
                contig = genome.contig_of(v["g"])
                sub = dict(rec, strand=v["strand"], contig=genome.names[contig], rank=rank)
                several[name].append(sub)
                todo.append({"rec": sub, "key": (name, rank), "codes": codes if v["strand"] == "forward" else assess.reverse_complement(codes),
                             "delta": v["delta"], "contig": contig, "slack": max(BIN, n // 8)})
            continue
        if seeds is not None and name in seeds:
            sd = seeds[name]
            strand, delta, contig = sd["strand"], int(sd["delta"]), int(sd["contig"])
        else:
            v = voted[name]
            rec["votes"], rec["votes_second"] = v["votes"], v["votes_second"]
            if v["votes"] < min_votes or v["delta"] is None:
                continue
            strand, delta, contig = v["strand"], v["delta"], genome.contig_of(v["g"])
        rec["strand"], rec["contig"] = strand, genome.names[contig]
        todo.append({"rec": rec, "key": name, "codes": codes if strand == "forward" else assess.reverse_complement(codes), "delta": delta,
                     "contig": contig, "slack": max(BIN, n // 8)})
    references = {}
    while todo:
        spans = [window_of(genome, t["contig"], t["delta"], len(t["codes"]), t["slack"]) for t in todo]
        got = aligner([t["codes"] for t in todo], [genome.codes[lo:hi] for lo, hi in spans], band)
        again = []
        for t, (lo, hi), r in zip(todo, spans, got):
            rec = t["rec"]
            c0 = int(genome.starts[t["contig"]])
            c1 = c0 + int(genome.lengths[t["contig"]])
            s, e, n = int(r["start"]), int(r["end"]), len(t["codes"])
            touches = (s == 0 and lo > c0) or (e == hi - lo and hi < c1)
            if touches and rec["widenings"] < MAX_WIDENINGS:
                rec["widenings"] += 1
                t["slack"] *= 2
                again.append(t)
                continue
            E, M = int(r["edit"]), int(r["match"])
            x, i, d = assess.counts(n, e - s, E, M)
            rec.update({"start": lo + s - c0, "end": lo + e - c0, "edit": E, "match": M, "mismatch": x, "insertion": i, "deletion": d,
                        "band": int(r["band"]), "status": "edge" if touches else "mapped"})
            rec.update(assess.rates(M, x, i, d))
            if not touches:
                cut = genome.codes[lo + s:lo + e]
                references[t["key"]] = decode(cut if rec["strand"] == "forward" else assess.reverse_complement(cut))
        todo = again
    if candidates > 1:
        for name, rec in recs.items():
            cands = several.get(name)
            if cands is None:                                                 # a single-candidate record: given seeds, or no pick
                rec.update({"mapq": MAPQ_MAX if rec["status"] == "mapped" else 0, "candidates": int(rec["status"] != "unmapped"),
                            "edit_second": None, "seed_rank": 0 if rec["status"] != "unmapped" else None})
                continue
            primary, mapq, second = choose(cands)
            shown = primary if primary is not None else cands[0] if cands else None
            if shown is not None:
                rec.update({key: shown[key] for key in shown if key not in ("rank", "votes", "votes_second")})
            rec.update({"mapq": mapq, "candidates": len(cands), "edit_second": second, "seed_rank": shown["rank"] if shown is not None else None})
        chosen = {name: (name, rec["seed_rank"]) for name, rec in recs.items() if name in several}
        references = {key if not isinstance(key, tuple) else key[0]: seq for key, seq in references.items()
                      if not isinstance(key, tuple) or (chosen[key[0]] == key and recs[key[0]]["status"] == "mapped")}
    per_read = [recs[name] for name in sorted(recs)]
    totals = {st: sum(1 for r in per_read if r["status"] == st) for st in ("mapped", "unmapped", "edge")}
    totals["reads"] = len(per_read)
    for key in ("edit", "match", "mismatch", "insertion", "deletion"):
        totals[key] = int(sum(r[key] for r in per_read if r["status"] == "mapped"))
    totals.update(assess.rates(totals["match"], totals["mismatch"], totals["insertion"], totals["deletion"]))
    result = {"reads": per_read, "references": references, "totals": totals,
              "unmapped": [r["name"] for r in per_read if r["status"] == "unmapped"]}
    if candidates > 1:
        result["ambiguity"] = {"mapq0": sum(1 for r in per_read if r["mapq"] == 0),
                               "mapq1_59": sum(1 for r in per_read if 0 < r["mapq"] < MAPQ_MAX),
                               "mapq60": sum(1 for r in per_read if r["mapq"] == MAPQ_MAX),
                               "won_by_later_pick": sum(1 for r in per_read if r["seed_rank"])}
    return result


def add_cigars(result, reads, genome, workspace_mb=4096, device_id=0, tracer=None):
    """Trace every mapped read of a map_reads result against genome[start : end) of its contig on the forward genome strand -- a
    reverse-strand read as its reverse complement, the orientation map_reads aligned it in -- and record the CIGAR (over =XID, in
    genome coordinates, gaps left-aligned there) as the record's `cigar`.  tracer(reads, refs) -> op arrays replaces
    assess.align_ops (the tests' reference)."""
    if tracer is None:
        def tracer(rs, fs):
            return assess.align_ops(rs, fs, workspace_mb, device_id)
    contig = {name: c for c, name in enumerate(genome.names)}
    recs = [r for r in result["reads"] if r["status"] == "mapped"]
    seqs, cuts = [], []
    for r in recs:
        codes = assess.encode(reads[r["name"]])
        c0 = int(genome.starts[contig[r["contig"]]])
        seqs.append(codes if r["strand"] == "forward" else assess.reverse_complement(codes))
        cuts.append(genome.codes[c0 + r["start"]:c0 + r["end"]])
    for r, ops in zip(recs, tracer(seqs, cuts) if recs else []):
        r["cigar"] = assess.cigar(ops)
    return result


def sam_lines(result, reads, genome):
    """@HD, @SQ per contig, then one line per mapped read that carries a `cigar` (add_cigars): FLAG 0 or 16, POS 1-based, MAPQ the
    record's mapq (255, not available, without one: map_reads at candidates=1), the CIGAR over =XID, SEQ in genome orientation,
    QUAL *, NM:i:E and, when a second candidate was aligned, e2:i: with its edit distance."""
    lines = ["@HD\tVN:1.6\tSO:unknown"] + ["@SQ\tSN:%s\tLN:%d" % (name, int(n)) for name, n in zip(genome.names, genome.lengths)]
    for r in result["reads"]:
        if r["status"] != "mapped" or "cigar" not in r:
            continue
        codes = assess.encode(reads[r["name"]])
        seq = decode(codes if r["strand"] == "forward" else assess.reverse_complement(codes))
        lines.append("\t".join(str(v) for v in (r["name"], 0 if r["strand"] == "forward" else 16, r["contig"], r["start"] + 1, r.get("mapq", 255),
                                                 r["cigar"], "*", 0, 0, seq or "*", "*", "NM:i:%d" % r["edit"]) + _second_tag(r)))
    return lines


def _second_tag(r):
    return ("e2:i:%d" % r["edit_second"],) if r.get("edit_second") is not None else ()


def paf_lines(result, genome):
    """The twelve PAF columns of every mapped read: the whole read is aligned (query 0 .. n), the residue-match column is M, the
    block length M + X + I + D, the mapping quality the record's mapq (255, not available, without one).  After them e2:i: when a
    second candidate was aligned, and a cg:Z: tag for a record that carries a `cigar` (add_cigars)."""
    tlen = dict(zip(genome.names, (int(v) for v in genome.lengths)))
    lines = []
    for r in result["reads"]:
        if r["status"] != "mapped":
            continue
        block = r["match"] + r["mismatch"] + r["insertion"] + r["deletion"]
        cols = (r["name"], r["read_len"], 0, r["read_len"], "+" if r["strand"] == "forward" else "-", r["contig"], tlen[r["contig"]],
                r["start"], r["end"], r["match"], block, r.get("mapq", 255)) + _second_tag(r) + (("cg:Z:" + r["cigar"],) if "cigar" in r else ())
        lines.append("\t".join(str(v) for v in cols))
    return lines


def write_references(folder, references):
    os.makedirs(folder, exist_ok=True)
    for name, seq in references.items():
        with open(os.path.join(folder, name + "_ref.fasta"), "w") as f:
            f.write(">%s\n%s\n" % (name, seq))


def write_outputs(out_dir, result, genome, meta=None, reads=None):
    """reference/<read>_ref.fasta, mapped.paf and map_report.json under out_dir; with reads (a result that went through
    add_cigars) mapped.sam as well."""
    os.makedirs(out_dir, exist_ok=True)
    write_references(os.path.join(out_dir, "reference"), result["references"])
    with open(os.path.join(out_dir, "mapped.paf"), "w") as f:
        f.write("".join(ln + "\n" for ln in paf_lines(result, genome)))
    if reads is not None:
        with open(os.path.join(out_dir, "mapped.sam"), "w") as f:
            f.write("".join(ln + "\n" for ln in sam_lines(result, reads, genome)))
    report = dict(meta or {})
    if "ambiguity" in result:
        report.update(result["ambiguity"])
    report.update({"totals": result["totals"], "unmapped": result["unmapped"], "reads": result["reads"]})
    with open(os.path.join(out_dir, "map_report.json"), "w") as f:
        json.dump(report, f, indent=1)
    return report


def map_command(input_path, genome_path, out_dir, min_votes=MIN_VOTES, max_occ=MAX_OCC, band=BAND0, workspace_mb=4096, device_id=0,
                cigar=False, seed=DEFAULT_SEED, candidates=1, second_ratio=0.5):
    """The `map` command: called reads + genome -> the three outputs (with cigar: traced, and mapped.sam too); returns the report.
    seed: "gpu" votes with vote_reads, "host" with the per-read numpy `vote`; the outputs are the same.  candidates > 1: up to that
    many seeds a read are aligned and the files carry a mapping quality (map_reads); the report says so."""
    seeder = seeder_of(seed, workspace_mb, device_id)
    genome = load_genome(genome_path)
    reads = assess.load_reads(input_path)
    result = map_reads(reads, genome, min_votes, max_occ, band, workspace_mb, device_id, seeder=seeder, candidates=candidates,
                       second_ratio=second_ratio, top_seeder=top_seeder_of(seed, workspace_mb, device_id))
    meta = {"input": input_path, "genome": genome_path, "k": K, "min_votes": min_votes, "max_occ": max_occ, "band": band, "seed": seed}
    if candidates > 1:
        meta.update({"candidates": candidates, "second_ratio": second_ratio})
    if not cigar:
        return write_outputs(out_dir, result, genome, meta)
    add_cigars(result, reads, genome, workspace_mb, device_id)
    return write_outputs(out_dir, result, genome, dict(meta, cigar=True), reads)


def assess_genome(input_path, genome_path, min_votes=MIN_VOTES, max_occ=MAX_OCC, band=BAND0, workspace_mb=4096, device_id=0,
                  profile=False, seed=DEFAULT_SEED, candidates=1, second_ratio=0.5):
    """`assess -g`: map, then assess every mapped read against its cut-out (which is in the read's orientation, so the global
    alignment runs forward); the report's strand, contig, start and end come from the mapping.  Reads that did not map are the
    report's unpaired reads.  profile: the per-read cigar and the pooled error profile as well, in the read's orientation (not the
    genome's, unlike `map --cigar`); the report's profile_orientation says so.  seed: as for map_command."""
    seeder = seeder_of(seed, workspace_mb, device_id)
    reads = assess.load_reads(input_path)
    mapped = map_reads(reads, load_genome(genome_path), min_votes, max_occ, band, workspace_mb, device_id, seeder=seeder,
                       candidates=candidates, second_ratio=second_ratio, top_seeder=top_seeder_of(seed, workspace_mb, device_id))
    paired, unpaired = assess.pair_reads(reads, mapped["references"])
    rows = assess.align_pairs([p[1] for p in paired], [p[2] for p in paired], device_id)
    by = {r["name"]: r for r in mapped["reads"]}
    report = assess.build_report([p[0] for p in paired], rows, [by[p[0]]["strand"] for p in paired], unpaired,
                                 {"input": input_path, "genome": genome_path, "reference": None, "strand_mode": "mapped"})
    for rec in report["reads"]:
        rec.update({key: by[rec["name"]][key] for key in ("contig", "start", "end")})
    if profile:
        report["profile_orientation"] = "read"
        assess.add_profile(report, [assess.encode(p[1]) for p in paired], [assess.encode(p[2]) for p in paired], workspace_mb, device_id)
    return report
