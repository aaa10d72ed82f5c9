"""Read-to-read overlaps: which reads of a run share sequence, where, and in which arrangement -- without a genome.

Everything else that relates reads to each other goes through `-g <genome.fa>`; a run without a reference starts here.  The reads
are seeded against each other on the host (`candidates`, numpy: the definition of the seeding) and every candidate pair is aligned
on the GPU (chiron_align_overlap, csrc/overlap.hip): an exact dovetail alignment -- a suffix of one read against a prefix of the
other, containment as the limiting case -- inside a band of diagonals.  `chiron overlap` writes overlaps.paf and
overlap_report.json.  Layout, read correction, CIGARs for overlaps and seeding on the GPU are not here.

  reads      {name: sequence}; read i is the i-th name in sorted order.  All reads are concatenated with SEPARATOR code-4 bases between
             neighbours (`read_starts`); the index is map.build_index over that, k = 15, k-mers above max_occ dropped.
  seeding    read q, as given and as its reverse complement, is looked up in the index (the hits of map.hits).  A hit at concatenated position
             g lies in read t; only t > q counts, so each unordered pair is found once and a read never meets itself.  Its diagonal
             is delta = (g - start of t) - r, the target's position minus the query's: the d = j - i of the alignment table with
             the query as a and the target as b.  Per (t, strand): bins delta // 256 (floor) and the score "count plus the next
             bin's" are map.bin_scores; the best bin wins, ties to the smaller bin; below min_votes the pair is dropped; delta* is
             the lower median of the two bins' hits ordered by (delta, g).  A read keeps its max_overlaps best candidates: the
             highest scores, then the smaller t, then forward before reverse.  No cap of 8: this is not map.vote_top.
  band       [delta* - w, delta* + w] clipped to [-n, m], w = band.  THE BAND IS A RULE, NOT A CERTIFICATE: the aligned result
             is the best path inside it (include/chiron_amd.h), and an overlap on a far diagonal -- a repeat -- is another path
             that nothing inside the band excludes.
  edge       a result whose start or end diagonal lies on a band edge that is not the table's edge may continue outside: the
             pair's w doubles and it is aligned again in a follow-up call, at most MAX_WIDENINGS times; then it is counted
             `edge` and dropped.  map's window-edge rule, and a rule as well.
  type       from (s, e) alone.  The path starts on row 0 when s >= n (at b's base s - n, a from its first base) and on column 0
             otherwise (at a's base n - s); it ends on row n when e <= m (a to its last base) and on column m otherwise:
               row 0    -> row n     contained   a lies inside b            column 0 -> column m  contains    b lies inside a
               column 0 -> row n     dovetail_ab a's end meets b's start     row 0    -> column m  dovetail_ba b's end meets a's start
             A corner lies on a row and on a column; there the covered read decides: a path that covers all of a is contained,
             else one that covers all of b contains (column 0 to the corner (n, m) covers b: contains, not dovetail_ab).
             length is the shorter of the two spans, identity M / (M + E), E = (cost + M) / 2.
There is no CPU fallback: without the library or a GPU, align_overlap raises.  The defaults are not tuned on real reads.
"""
import json
import os

import numpy as np

from . import _lib, assess
from . import map as map_mod

K = map_mod.K
BIN = map_mod.BIN
SEPARATOR = map_mod.SEPARATOR
MAX_WIDENINGS = 3
MIN_VOTES, MAX_OCC, MAX_OVERLAPS, BAND, MIN_OVERLAP, MIN_IDENTITY = 4, 64, 128, 256, 500, 0.7
MAX_READ = _lib.OVERLAP_MAX_READ
LDS_SLOTS, MAX_GROUPS = _lib.ALIGN_LDS_SLOTS, _lib.ALIGN_MAX_GROUPS
TYPES = ("contained", "contains", "dovetail_ab", "dovetail_ba")
TYPE_LETTER = {"contained": "c", "contains": "C", "dovetail_ab": "d", "dovetail_ba": "D"}     # tp:A: holds one character

OVERLAP_DTYPE = np.dtype([("cost", np.int32), ("match", np.int32), ("start", np.int32), ("end", np.int32)])


# ----------------------------------------------------------------------------------------------------------------------------
# the kernel
# ----------------------------------------------------------------------------------------------------------------------------
def workspace_size(reads, total_bases, pairs, max_band):
    return _lib.sized("chiron_align_overlap_workspace_size", reads, total_bases, pairs, max_band)


def _call_shape(lens, pairs):
    """What one call over `pairs` (rows of a, b, dlo, dhi; lens the length of every read) holds: the reads it names (sorted),
    their bases, and its widest clipped band (0 for an empty one, which the library refuses)."""
    used = np.unique(pairs[:, :2])
    n, m = lens[pairs[:, 0]], lens[pairs[:, 1]]
    width = np.minimum(pairs[:, 3], m) - np.maximum(pairs[:, 2], -n) + 1
    return used, int(lens[used].sum()), int(max(width.max(), 0))


def align_overlap(reads, pairs, device_id=0):
    """One call of chiron_align_overlap.  reads: sequences (str, bytes or uint8 code arrays); pairs: rows of (a index, b index, dlo,
    dhi).  Only the reads the pairs name are copied, each once.  -> OVERLAP_DTYPE rows: cost, match, start (s), end (e)."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 4)
    out = np.zeros(len(pairs), dtype=OVERLAP_DTYPE)
    if len(pairs) == 0:
        return out
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    used, total, max_band = _call_shape(lens, pairs)
    coded = [assess.encode(reads[i]) for i in used]
    codes = np.ascontiguousarray(np.concatenate(coded + [np.zeros(1, np.uint8)]))
    read_off = np.concatenate([[0], np.cumsum(lens[used])]).astype(np.int64)
    cols = [np.ascontiguousarray(c, dtype=np.int32) for c in (np.searchsorted(used, pairs[:, 0]), np.searchsorted(used, pairs[:, 1]),
                                                               np.clip(pairs[:, 2], -(1 << 30), 1 << 30), np.clip(pairs[:, 3], -(1 << 30), 1 << 30))]
    need = []
    lib, ws, stream = _lib.device_workspace(lambda: need.append(workspace_size(len(used), total, len(pairs), max_band)) or need[0], device_id,
                                            "overlap.align_overlap", "overlap alignment")
    res = np.zeros((len(pairs), 5), dtype=np.int32)
    _lib.check(lib.chiron_align_overlap(device_id, codes.ctypes.data, read_off.ctypes.data, len(used), cols[0].ctypes.data, cols[1].ctypes.data,
                                        cols[2].ctypes.data, cols[3].ctypes.data, len(pairs), res.ctypes.data, ws.data_ptr(), need[0], 0, stream))
    del ws
    out["cost"], out["match"], out["start"], out["end"] = res[:, 0], res[:, 1], res[:, 2], res[:, 3]
    return out


def plan_batches(lens, pairs, budget_bytes, size=workspace_size):
    """Consecutive runs of pairs [(first, last + 1)] whose call fits the budget, each the longest that does (a call's size never
    falls when a pair is added: bisection over the host-only size function); a pair that alone exceeds it gets a run of its own."""
    lens = np.asarray(lens, dtype=np.int64)

    def fits(first, last):
        used, total, max_band = _call_shape(lens, pairs[first:last])
        return size(len(used), total, last - first, max_band) <= budget_bytes

    n, runs, first = len(pairs), [], 0
    while first < n:
        lo, hi = first + 1, min(n, first + (1 << 24))
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if fits(first, mid):
                lo = mid
            else:
                hi = mid - 1
        runs.append((first, lo))
        first = lo
    return runs


# ----------------------------------------------------------------------------------------------------------------------------
# seeding (host, numpy: the definition)
# ----------------------------------------------------------------------------------------------------------------------------
def read_starts(lens):
    """Where each read begins in the concatenation: SEPARATOR code-4 bases lie between neighbours."""
    lens = np.asarray(lens, dtype=np.int64)
    return (np.concatenate([[0], np.cumsum(lens[:-1] + SEPARATOR)]) if len(lens) else np.zeros(0)).astype(np.int64)


def build_index(reads, max_occ=MAX_OCC):
    """map's index over the concatenated reads (uint8 code arrays)."""
    parts = []
    for i, r in enumerate(reads):
        if i:
            parts.append(np.full(SEPARATOR, 4, np.uint8))
        parts.append(r)
    return map_mod.build_index(np.concatenate(parts) if parts else np.zeros(0, np.uint8), K, max_occ)


def _hits(index, codes):
    """map.hits -- (delta, g) of every seed hit -- with the read's k-mers looked up in sorted order: against an index of a whole run
    the binary searches then walk the index once instead of jumping through it.  The hits are the same, in another order."""
    idx_val, idx_pos = index
    rv, rp = map_mod.kmers(codes, K)
    order = np.argsort(rv, kind="stable")
    rv, rp = rv[order], rp[order]
    lo = np.searchsorted(idx_val, rv, side="left")
    cnt = np.searchsorted(idx_val, rv, side="right") - lo
    total = int(cnt.sum())
    if total == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    which = np.repeat(np.arange(len(rv)), cnt)
    g = idx_pos[lo[which] + np.arange(total) - np.repeat(np.cumsum(cnt) - cnt, cnt)]
    return g - rp[which], g


def candidates(index, reads, min_votes=MIN_VOTES, max_overlaps=MAX_OVERLAPS):
    """The seeding decision for every read (module docstring).  reads: uint8 code arrays, in index order.
    -> [dict(a, b, strand, votes, delta)], by a, then best first."""
    starts = read_starts([len(r) for r in reads])
    floor = max(int(min_votes), 1)
    out = []
    for q, codes in enumerate(reads):
        mine = []
        for strand, seq in (("forward", codes), ("reverse", assess.reverse_complement(codes))):
            delta, g = _hits(index, seq)
            if len(delta) == 0:
                continue
            t = np.searchsorted(starts, g, side="right") - 1
            later = t > q
            t, g = t[later], g[later]
            rel = delta[later] - starts[t]
            order = np.lexsort((g, rel, t))
            t, g, rel = t[order], g[order], rel[order]
            targets, first, count = np.unique(t, return_index=True, return_counts=True)
            for b, lo, cnt in zip(targets.tolist(), first.tolist(), count.tolist()):
                if cnt < floor:                                           # a score is at most the pair's hits
                    continue
                d = rel[lo:lo + cnt]
                bins, score = map_mod.bin_scores(d)
                best = int(np.argmax(score))                              # the first maximum: the smaller bin
                if int(score[best]) < floor:
                    continue
                beta = int(bins[best])
                sel = np.nonzero((d // BIN == beta) | (d // BIN == beta + 1))[0]      # already ordered by (delta, g)
                mine.append({"a": q, "b": b, "strand": strand, "votes": int(score[best]), "delta": int(d[sel[(len(sel) - 1) // 2]])})
        mine.sort(key=lambda c: (-c["votes"], c["b"], c["strand"] != "forward"))
        out.extend(mine[:max_overlaps])
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# from a result to an overlap
# ----------------------------------------------------------------------------------------------------------------------------
def classify(n, m, s, e):
    """-> (type, (a0, a1), (b0, b1)): the type and the spans of a and b the path covers, from (s, e) alone."""
    a0, b0 = (0, s - n) if s >= n else (n - s, 0)
    a1, b1 = (n, e) if e <= m else (m - e + n, m)
    if a0 == 0 and a1 == n:
        kind = "contained"
    elif b0 == 0 and b1 == m:
        kind = "contains"
    else:
        kind = "dovetail_ab" if a0 > 0 else "dovetail_ba"
    return kind, (a0, a1), (b0, b1)


def touches_edge(n, m, dlo, dhi, s, e):
    """Does the start or the end diagonal lie on an edge of the (clipped) band that is not the table's edge?"""
    return any((d == dlo and dlo > -n) or (d == dhi and dhi < m) for d in (s - n, e - n))


def band_pairs(lens, R, cands, widths):
    """The rows (a, b, dlo, dhi) an aligner takes for candidates at half-widths `widths`: lens holds the lengths of the R reads
    and then of their reverse complements, a reverse-strand candidate's a is R + a, the band is [delta - w, delta + w] clipped
    to [-n, m]."""
    pairs = np.zeros((len(cands), 4), dtype=np.int64)
    for k, (c, w) in enumerate(zip(cands, widths)):
        ia = c["a"] if c["strand"] == "forward" else R + c["a"]
        n, m = int(lens[ia]), int(lens[c["b"]])
        pairs[k] = (ia, c["b"], max(c["delta"] - w, -n), min(c["delta"] + w, m))
    return pairs


def overlap_pairs(reads, cands, band=BAND, min_overlap=MIN_OVERLAP, min_identity=MIN_IDENTITY, workspace_mb=4096, device_id=0,
                  aligner=None, size=workspace_size):
    """Align the candidates of `candidates` and keep the overlaps.  reads: uint8 code arrays.  aligner(seqs, pairs) -> OVERLAP_DTYPE
    rows replaces the GPU call (the tests' reference): seqs is reads followed by their reverse complements, so a reverse-strand
    candidate's a is seqs[len(reads) + a].  The calls are planned here, against workspace_mb, whoever aligns.
    -> dict(overlaps=[records by (a, b, strand)], aligned, realigned, edge, kept={type: count}, dropped={reason: count}, batches)."""
    if band < 0:
        raise ValueError("band must be 0 or more, not %r" % (band,))
    if aligner is None:
        def aligner(seqs, pairs):
            return align_overlap(seqs, pairs, device_id)
    R = len(reads)
    seqs = list(reads) + [assess.reverse_complement(r) for r in reads]
    lens = np.array([len(r) for r in seqs], dtype=np.int64)
    todo = [{"cand": c, "w": int(band), "widenings": 0} for c in cands]
    result = {"overlaps": [], "aligned": len(todo), "realigned": 0, "edge": 0, "kept": {t: 0 for t in TYPES},
              "dropped": {"short": 0, "identity": 0}, "batches": 0}
    while todo:
        pairs = band_pairs(lens, R, [t["cand"] for t in todo], [t["w"] for t in todo])
        got = np.zeros(len(todo), dtype=OVERLAP_DTYPE)
        for first, last in plan_batches(lens, pairs, int(workspace_mb) << 20, size):
            got[first:last] = aligner(seqs, pairs[first:last])
            result["batches"] += 1
        again = []
        for t, (ia, ib, dlo, dhi), r in zip(todo, pairs.tolist(), got):
            c = t["cand"]
            n, m = int(lens[ia]), int(lens[ib])
            cost, M, s, e = int(r["cost"]), int(r["match"]), int(r["start"]), int(r["end"])
            if touches_edge(n, m, dlo, dhi, s, e):
                if t["widenings"] < MAX_WIDENINGS:
                    t["widenings"] += 1
                    t["w"] *= 2
                    again.append(t)
                else:
                    result["edge"] += 1
                continue
            E = (cost + M) // 2
            kind, (a0, a1), (b0, b1) = classify(n, m, s, e)
            length = min(a1 - a0, b1 - b0)
            identity = M / (M + E) if M + E else 0.0
            if length < min_overlap:
                result["dropped"]["short"] += 1
                continue
            if identity < min_identity:
                result["dropped"]["identity"] += 1
                continue
            result["kept"][kind] += 1
            result["overlaps"].append({"a": c["a"], "b": ib, "strand": c["strand"], "type": kind, "a_len": n, "b_len": m,
                                       "a_start": a0, "a_end": a1, "b_start": b0, "b_end": b1, "length": length, "match": M, "edit": E,
                                       "cost": cost, "identity": identity, "votes": c["votes"], "band": t["w"], "widenings": t["widenings"]})
        result["realigned"] += len(again)
        todo = again
    result["overlaps"].sort(key=lambda o: (o["a"], o["b"], o["strand"] != "forward"))
    return result


def find_overlaps(reads, min_votes=MIN_VOTES, max_occ=MAX_OCC, max_overlaps=MAX_OVERLAPS, band=BAND, min_overlap=MIN_OVERLAP,
                  min_identity=MIN_IDENTITY, workspace_mb=4096, device_id=0, aligner=None, size=workspace_size):
    """{name: sequence} -> (names in index order, the result of overlap_pairs with reads and candidate_pairs added)."""
    names = sorted(reads)
    coded = [assess.encode(reads[name]) for name in names]
    for name, c in zip(names, coded):
        if len(c) > MAX_READ:
            raise ValueError("read %s has %d bases, an overlap takes at most %d" % (name, len(c), MAX_READ))
    cands = candidates(build_index(coded, max_occ), coded, min_votes, max_overlaps)
    result = overlap_pairs(coded, cands, band, min_overlap, min_identity, workspace_mb, device_id, aligner, size)
    result["reads"], result["candidate_pairs"] = len(names), len(cands)
    return names, result


def paf_lines(names, result):
    """The twelve PAF columns of every kept overlap, a the query and b the target: the residue-match column is M, the block
    length M + E, the mapping quality 255 (not available).  A reverse-strand overlap has `-` in column 5, the target as given and
    the query's span on the query's original strand (the PAF convention, as map writes it).  Then tp:A: with the type's letter
    (c contained, C contains, d dovetail_ab, D dovetail_ba: the tag holds one character), ty:Z: with its name, and ed:i: E."""
    lines = []
    for o in result["overlaps"]:
        n = o["a_len"]
        q0, q1 = (o["a_start"], o["a_end"]) if o["strand"] == "forward" else (n - o["a_end"], n - o["a_start"])
        cols = (names[o["a"]], n, q0, q1, "+" if o["strand"] == "forward" else "-", names[o["b"]], o["b_len"], o["b_start"], o["b_end"],
                o["match"], o["match"] + o["edit"], 255, "tp:A:" + TYPE_LETTER[o["type"]], "ty:Z:" + o["type"], "ed:i:%d" % o["edit"])
        lines.append("\t".join(str(v) for v in cols))
    return lines


def write_outputs(out_dir, names, result, meta=None):
    """overlaps.paf and overlap_report.json under out_dir; returns the report."""
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "overlaps.paf"), "w") as f:
        f.write("".join(ln + "\n" for ln in paf_lines(names, result)))
    report = dict(meta or {})
    report.update({"reads": result["reads"], "candidate_pairs": result["candidate_pairs"], "aligned": result["aligned"],
                   "realigned": result["realigned"], "edge": result["edge"], "kept": dict(result["kept"], total=len(result["overlaps"])),
                   "dropped": result["dropped"], "batches": result["batches"]})
    with open(os.path.join(out_dir, "overlap_report.json"), "w") as f:
        json.dump(report, f, indent=1)
    return report


def overlap_command(input_path, out_dir, min_votes=MIN_VOTES, max_occ=MAX_OCC, max_overlaps=MAX_OVERLAPS, band=BAND, min_overlap=MIN_OVERLAP,
                    min_identity=MIN_IDENTITY, workspace_mb=4096, device_id=0, aligner=None):
    """The `overlap` command: called reads -> overlaps.paf and overlap_report.json; returns the report."""
    reads = assess.load_reads(input_path)
    names, result = find_overlaps(reads, min_votes, max_occ, max_overlaps, band, min_overlap, min_identity, workspace_mb, device_id, aligner)
    meta = {"input": input_path, "parameters": {"k": K, "min_votes": min_votes, "max_occ": max_occ, "max_overlaps": max_overlaps, "band": band,
                                                "min_overlap": min_overlap, "min_identity": min_identity, "workspace_mb": workspace_mb}}
    return write_outputs(out_dir, names, result, meta)
