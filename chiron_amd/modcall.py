"""Modcall: per-read calls of modified bases at motif sites, from two k-mer level tables.

`squiggle --control` compares two samples position by position and says nothing about a single read; `squiggle --refine` knows only
the unmodified levels and pulls the borders wrong at a modified site.  This module gives the DP both tables, as nanopolish
call-methylation and Tombo's alternative model do: at every motif site of every read the samples around the site are fitted to the
window's expected levels under the canonical table and under the modified one, with the borders inside the window free under either
hypothesis, and the difference of the two costs is the call.

Both tables have a producer in the tree: `squiggle --kmer K` on an unmodified run writes the canonical kmer_levels.tsv, the same
command on a fully modified run the alternative one.

A read here is squiggle.py's: polish.py's dict(name, pos, ops, reverse, called, lead) plus `signal` (int16, squiggle.normalise) and
`starts` (int32 [bases + 1], squiggle.base_starts), in signal order.

  motif_sites     the genome positions of the modified base, per strand
  site_groups     on one strand, sites whose motif occurrences are fewer than k bases apart are one group, called as one: all
                  canonical against all modified (nanopolish's rule)
  group_window    a group's window: from k // 2 + flank positions before its first modified base to (k - 1 - k // 2) + flank after
                  its last one, in the strand's orientation
  window_rows     the window's two rows of levels, written in genome space: the true molecule is the genome, so miscalls and indels
                  of the basecall inside the window do not matter -- the DP re-segments the samples.  The alternative row takes the
                  alternative table's level for every base whose k-mer holds a WHOLE motif occurrence of the group and the canonical
                  level elsewhere: a k-mer that holds only a part of the motif has, in any table learned from a run, a level that
                  mixes contexts, and so is canonical under both hypotheses (a limit of the method)
  read_segment    the read's samples for a window: from the first sample of the read base aligned to the window's first position to
                  the last sample of the one aligned to its last

The scoring is the library's chiron_signal_score (csrc/site_score.hip): every (read, group) is one segment with two candidates.
Everything else is plain numpy.  There is no CPU fallback: the hook scorer= exists for the tests' reference.

Limits, written down: the sites of a group are not called independently (that is 2^n hypotheses); a window wider than 16 columns is
dropped; the cost is an L1 distance with one scale for all k-mers, not a Gaussian likelihood with per-k-mer spreads; every base of
the window must get a sample (no skips); a read's gain and offset are not re-estimated against the table (the median and MAD
normalisation stays squiggle's); the alternative table is not learned from a partly modified run; a window's outermost k-mers may
hold a whole motif occurrence of a neighbouring group, which is canonical under both hypotheses; nothing here was run on real reads,
and the default --min-delta is not tuned on them."""
import json
import os

import numpy as np

from . import _lib, label, squiggle

MAX_SAMPLES, MAX_COLUMNS, INFEASIBLE = _lib.SITE_MAX_SAMPLES, _lib.SITE_MAX_COLUMNS, _lib.SITE_INFEASIBLE
THREADS, MAX_GROUPS = _lib.SITE_THREADS, _lib.SITE_MAX_GROUPS
UNKNOWN = squiggle.UNKNOWN
SCALE = squiggle.SCALE
MIN_DELTA = 8.0                          # int16 units a sample; from a numpy sketch of the planted case, NOT tuned on real reads
FLANK = 2
GROUP_DROPS = ("window_off_read", "end_unaligned", "too_wide", "unknown_level", "too_long", "infeasible")
CALLS = ("modified", "canonical", "ambiguous")
CALL_COLUMNS = ("read", "contig", "pos", "sites", "strand", "samples", "columns", "c0", "c1", "delta", "call")
SITE_COLUMNS = ("contig", "pos", "strand", "groups", "modified", "canonical", "ambiguous", "fraction", "mean_delta")


# ----------------------------------------------------------------------------------------------------------------------------
# sites, groups, windows
# ----------------------------------------------------------------------------------------------------------------------------
def _motif_codes(motif, offset):
    if not motif or set(motif) - set("ACGT"):
        raise ValueError("motif %r is not over ACGT" % (motif,))
    if not 0 <= offset < len(motif):
        raise ValueError("motif offset %d outside 0 .. %d, the bases of %s" % (offset, len(motif) - 1, motif))
    return np.array(["ACGT".index(c) for c in motif], dtype=np.int64)


def _occurrences(codes, pattern):
    """The positions at which `pattern` starts in codes."""
    m = len(pattern)
    if len(codes) < m:
        return np.zeros(0, np.int64)
    hit = np.ones(len(codes) - m + 1, dtype=bool)
    for j in range(m):
        hit &= codes[j:len(codes) - m + 1 + j] == pattern[j]
    return np.flatnonzero(hit).astype(np.int64)


def motif_occurrences(genome, motif="CG"):
    """(forward, reverse): the genome positions at which an occurrence of the motif begins in genome coordinates -- on the reverse
    strand that is the position of the motif's LAST base, the occurrences being those of its reverse complement."""
    m = _motif_codes(motif, 0)
    codes = np.asarray(genome.codes, dtype=np.int64)
    return _occurrences(codes, m), _occurrences(codes, 3 - m[::-1])


def motif_sites(genome, motif="CG", offset=0):
    """(forward, reverse): the concatenated-genome positions of the modified base, increasing, per strand.  motif is over ACGT and
    offset names the modified base inside it; on the reverse strand the sites are the occurrences of the motif in the reverse
    complement."""
    _motif_codes(motif, offset)
    fwd, rev = motif_occurrences(genome, motif)
    return fwd + offset, rev + (len(motif) - 1 - offset)


def site_groups(occurrences, k):
    """occurrences: increasing positions of one strand.  -> [(first index, one past the last)] of the maximal runs in which every
    occurrence begins fewer than k positions behind its predecessor."""
    occ = np.asarray(occurrences, dtype=np.int64)
    if len(occ) == 0:
        return []
    cuts = np.flatnonzero(np.diff(occ) >= k) + 1
    edges = np.concatenate([[0], cuts, [len(occ)]])
    return [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]


def group_window(first, last, reverse, k, flank=FLANK):
    """first, last: the group's lowest and highest site, the genome positions of its modified bases.  -> (g0, g1), the window's
    genome positions g0 .. g1 - 1: k // 2 + flank before the group's first modified base and (k - 1 - k // 2) + flank after its
    last one in the strand's orientation, which on the reverse strand runs from high positions to low ones.  One site, k = 5 and
    flank 2 are 9 positions."""
    h = k // 2
    before, after = h + flank, (k - 1 - h) + flank
    if reverse:
        before, after = after, before
    return int(first) - before, int(last) + after + 1


def window_codes(genome, g0, g1, reverse, k):
    """int64 [g1 - g0], in the strand's orientation: squiggle.kmer_bins' code of the genome k-mer around every window position, the
    base itself at index k // 2 of it; -1 where the k-mer leaves the genome or holds a code above 3."""
    codes = np.asarray(genome.codes, dtype=np.int64)
    h = k // 2
    g = np.arange(g0, g1, dtype=np.int64)
    lo = g - (k - 1 - h if reverse else h)
    out = np.full(len(g), -1, dtype=np.int64)
    ok = (lo >= 0) & (lo + k <= len(codes))
    if ok.any():
        win = codes[lo[ok][:, None] + np.arange(k)[None, :]]
        good = (win <= 3).all(axis=1)
        if reverse:
            win = 3 - win[:, ::-1]
        code = (np.where(win <= 3, win, 0) * (4 ** np.arange(k - 1, -1, -1, dtype=np.int64))[None, :]).sum(axis=1)
        out[ok] = np.where(good, code, -1)
    return out[::-1] if reverse else out


def window_rows(genome, g0, g1, reverse, k, occurrences, motif_len, table, alt_table):
    """The window's two rows, int32 [g1 - g0] each in the strand's orientation: (canonical, alternative).  occurrences: where the
    group's motif occurrences begin, in genome coordinates.  A base takes the alternative table's level when its k-mer -- genome
    positions g - k // 2 .. on the forward strand, g - (k - 1 - k // 2) .. on the reverse one, k of them -- holds one of the
    occurrences whole, and the canonical level otherwise.  UNKNOWN where the k-mer has no code or the table that is asked no level."""
    code = window_codes(genome, g0, g1, reverse, k)
    known = code >= 0
    at = np.maximum(code, 0)
    row0 = np.where(known, np.asarray(table, dtype=np.int32)[at], UNKNOWN).astype(np.int32)
    h = k // 2
    g = np.arange(g0, g1, dtype=np.int64)
    lo = g - (k - 1 - h if reverse else h)
    whole = np.zeros(len(g), dtype=bool)
    for a in occurrences:
        whole |= (lo <= a) & (a + motif_len <= lo + k)
    if reverse:
        whole = whole[::-1]
    row1 = np.where(whole, np.where(known, np.asarray(alt_table, dtype=np.int32)[at], UNKNOWN), row0).astype(np.int32)
    return row0, row1


def read_segment(columns, span, g0, g1, reverse):
    """columns: squiggle._columns(read), span: squiggle._read_span(read).  -> (first base, last base) in signal order of the read bases
    aligned ('=' or 'X') to the window's first and last position in the strand's orientation, or the reason the group is dropped."""
    if g0 < span[0] or g1 > span[1]:
        return "window_off_read"
    g, idx = columns
    first, last = (g1 - 1, g0) if reverse else (g0, g1 - 1)
    a, b = np.flatnonzero(g == first), np.flatnonzero(g == last)
    if len(a) == 0 or len(b) == 0:
        return "end_unaligned"
    return int(idx[a[0]]), int(idx[b[0]])


# ----------------------------------------------------------------------------------------------------------------------------
# the kernel
# ----------------------------------------------------------------------------------------------------------------------------
def score_workspace_size(segments, samples, candidates, levels):
    """chiron_signal_score_workspace_size (host-only)."""
    return _lib.sized("chiron_signal_score_workspace_size", int(segments), int(samples), int(candidates), int(levels))


def score_call(segments, candidates, device_id=0):
    """One chiron_signal_score call.  segments: int16 arrays; candidates: (segment index, int32 levels [1 .. 16]) pairs, in any
    order.  -> int32 costs [candidates], INFEASIBLE for a candidate with more levels than its segment has samples."""
    sig = [np.ascontiguousarray(s, dtype=np.int16).reshape(-1) for s in segments]
    lv = [np.ascontiguousarray(e, dtype=np.int32).reshape(-1) for _, e in candidates]
    n_seg, n_cand = len(sig), len(lv)
    sample_off, level_off = label._offsets([len(s) for s in sig]), label._offsets([len(e) for e in lv])
    samples = np.ascontiguousarray(np.concatenate(sig + [np.zeros(1, np.int16)]))
    level = np.ascontiguousarray(np.concatenate(lv + [np.zeros(1, np.int32)]))
    seg = np.ascontiguousarray(np.asarray([g for g, _ in candidates], dtype=np.int32).reshape(-1))
    cost = np.zeros(max(n_cand, 1), dtype=np.int32)
    args = (samples.ctypes.data, sample_off.ctypes.data, n_seg, level.ctypes.data, level_off.ctypes.data, seg.ctypes.data if n_cand else None, n_cand,
            cost.ctypes.data)
    if n_cand == 0:                                     # nothing to score: the library touches no device
        _lib.check(_lib.load().chiron_signal_score(device_id, *args, None, 0, 0, None))
        return cost[:0].copy()
    size = lambda: score_workspace_size(n_seg, int(sample_off[-1]), n_cand, int(level_off[-1]))
    lib, ws, stream = _lib.device_workspace(size, device_id, "modcall.score", "site kernel")
    _lib.check(lib.chiron_signal_score(device_id, *args, ws.data_ptr(), size(), 0, stream))
    del ws
    return cost[:n_cand].copy()


def plan_score_batches(counts, budget_bytes):
    """counts: (segments, samples, candidates, levels) per read.  Consecutive runs of reads [(first, last + 1)] whose call fits the
    budget, each the longest that does (the size grows with every read: bisection); a read that alone exceeds it gets a run of its
    own."""
    c = np.concatenate([np.zeros((1, 4), np.int64), np.cumsum(np.asarray(counts, dtype=np.int64).reshape(-1, 4), axis=0)])
    n, runs, first = len(c) - 1, [], 0
    while first < n:
        lo, hi = first + 1, n
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if score_workspace_size(*(c[mid] - c[first]).tolist()) <= budget_bytes:
                lo = mid
            else:
                hi = mid - 1
        runs.append((first, lo))
        first = lo
    return runs


# ----------------------------------------------------------------------------------------------------------------------------
# the stage
# ----------------------------------------------------------------------------------------------------------------------------
def strand_groups(genome, k, motif="CG", offset=0):
    """Per strand (0 forward, 1 reverse): [dict(first, last: where the group's first and last occurrence begin; occurrences; sites:
    the positions of the modified bases)], in genome order."""
    out = []
    for reverse, occ in enumerate(motif_occurrences(genome, motif)):
        shift = (len(motif) - 1 - offset) if reverse else offset
        out.append([{"first": int(occ[a]), "last": int(occ[b - 1]), "occurrences": occ[a:b], "sites": tuple(int(v) + shift for v in occ[a:b])}
                    for a, b in site_groups(occ, k)])
    return out


def call_of(delta, min_delta=MIN_DELTA):
    return "modified" if delta >= min_delta else ("canonical" if delta <= -min_delta else "ambiguous")


def read_candidates(read, genome, groups, tables, k, motif_len, flank=FLANK):
    """The groups of the read's strand that have a site on the read's aligned stretch, each either a segment with its two rows or
    a drop.  -> ([dict(group, s0: first sample, s1: one past the last, row0, row1)], {reason: count})."""
    drops = {reason: 0 for reason in GROUP_DROPS[:-1]}
    reverse = bool(read["reverse"])
    span = squiggle._read_span(read)
    columns = squiggle._columns(read)
    starts = np.asarray(read["starts"], dtype=np.int64)
    low, high = (np.array([g["sites"][e] for g in groups], dtype=np.int64) for e in (0, -1))      # both increase: groups do not overlap
    kept = []
    for gi in range(int(np.searchsorted(high, span[0], side="left")), int(np.searchsorted(low, span[1], side="left"))):
        grp = groups[gi]
        g0, g1 = group_window(grp["sites"][0], grp["sites"][-1], reverse, k, flank)
        if g1 - g0 > MAX_COLUMNS:
            drops["too_wide"] += 1
            continue
        where = read_segment(columns, span, g0, g1, reverse)
        if isinstance(where, str):
            drops[where] += 1
            continue
        row0, row1 = window_rows(genome, g0, g1, reverse, k, grp["occurrences"], motif_len, tables[0], tables[1])
        if (row0 == UNKNOWN).any() or (row1 == UNKNOWN).any():
            drops["unknown_level"] += 1
            continue
        s0, s1 = int(starts[where[0]]), int(starts[where[1] + 1])
        if s1 - s0 > MAX_SAMPLES:
            drops["too_long"] += 1
            continue
        kept.append({"group": gi, "s0": s0, "s1": s1, "row0": row0, "row1": row1})
    return kept, drops


def modcall(reads, genome, tables, k, motif="CG", offset=0, flank=FLANK, min_delta=MIN_DELTA, workspace_mb=4096, device_id=0, scorer=None):
    """Calls every motif group of every read.  reads: squiggle.prepare's (signal and starts); tables: (canonical, alternative), int32
    [4^k] each as squiggle.load_level_table gives them.  The calls are consecutive runs of reads planned against workspace_mb with
    the host-only size function; every (read, group) is one segment and two adjacent candidates, canonical first.
    scorer(segments, candidates) -> int32 costs replaces the library call (the tests' reference).
    -> dict(rows: per scored (read, group) in read and genome order dict(read, strand, group, sites, samples, columns, c0, c1, delta
    = (c0 - c1) / samples in int16 units a sample, call), groups: {seen, scored, dropped by reason}, calls by kind, batches).
    delta >= min_delta is `modified`, delta <= -min_delta `canonical`, anything else `ambiguous`; the default min_delta comes from
    a sketch on planted reads and is not tuned on real ones."""
    tables = (np.asarray(tables[0], dtype=np.int32), np.asarray(tables[1], dtype=np.int32))
    if tables[0].shape != (4 ** k,) or tables[1].shape != (4 ** k,):
        raise ValueError("tables of %s and %s entries for k = %d" % (tables[0].shape, tables[1].shape, k))
    if flank < 0:
        raise ValueError("flank %d is negative" % flank)
    if scorer is None:
        import torch  # noqa: F401  before the planner loads the library: torch's ROCm runtime has to come up first (_lib.py)

        def scorer(segments, candidates):
            return score_call(segments, candidates, device_id)
    reads = list(reads)
    groups = strand_groups(genome, k, motif, offset)
    drops = {reason: 0 for reason in GROUP_DROPS}
    per_read = []
    for r in reads:
        kept, d = read_candidates(r, genome, groups[int(bool(r["reverse"]))], tables, k, len(motif), flank)
        for reason, n in d.items():
            drops[reason] += n
        per_read.append(kept)
    counts = [(len(kept), sum(c["s1"] - c["s0"] for c in kept), 2 * len(kept), 2 * sum(len(c["row0"]) for c in kept)) for kept in per_read]
    batches = plan_score_batches(counts, int(workspace_mb * (1 << 20))) if reads else []
    rows, calls, used = [], {kind: 0 for kind in CALLS}, 0
    for first, last in batches:
        segments, candidates, where = [], [], []
        for i in range(first, last):
            for c in per_read[i]:
                candidates += [(len(segments), c["row0"]), (len(segments), c["row1"])]
                segments.append(reads[i]["signal"][c["s0"]:c["s1"]])
                where.append((i, c))
        if not where:
            continue
        used += 1
        cost = np.asarray(scorer(segments, candidates), dtype=np.int64)
        for n, (i, c) in enumerate(where):
            c0, c1 = int(cost[2 * n]), int(cost[2 * n + 1])
            if c0 == INFEASIBLE or c1 == INFEASIBLE:
                drops["infeasible"] += 1
                continue
            samples = c["s1"] - c["s0"]
            delta = (c0 - c1) / samples
            strand = int(bool(reads[i]["reverse"]))
            rows.append({"read": reads[i]["name"], "strand": strand, "group": c["group"], "sites": groups[strand][c["group"]]["sites"],
                         "samples": samples, "columns": len(c["row0"]), "c0": c0, "c1": c1, "delta": delta, "call": call_of(delta, min_delta)})
            calls[rows[-1]["call"]] += 1
    dropped = sum(drops.values())
    return {"rows": rows, "groups": {"seen": len(rows) + dropped, "scored": len(rows), "dropped": drops}, "calls": calls, "batches": used}


# ----------------------------------------------------------------------------------------------------------------------------
# files and the command
# ----------------------------------------------------------------------------------------------------------------------------
def _place(genome, g):
    c = genome.contig_of(int(g))
    return genome.names[c], int(g) - int(genome.starts[c]) + 1


def call_lines(rows, genome):
    """mod_calls.tsv: one row per scored (read, group): the read, the contig and 1-based position of the group's first site, the
    number of its sites, the strand, the segment's samples, the window's columns, the two costs, delta and the call."""
    lines = ["\t".join(CALL_COLUMNS) + "\n"]
    for r in rows:
        contig, pos = _place(genome, r["sites"][0])
        lines.append("%s\t%s\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%.4f\t%s\n" % (r["read"], contig, pos, len(r["sites"]), "+-"[r["strand"]], r["samples"],
                                                                      r["columns"], r["c0"], r["c1"], r["delta"], r["call"]))
    return lines


def site_table(rows):
    """{(site position, strand): [groups scored, modified, canonical, ambiguous, sum of delta]}: every site of a group counts the
    group's call."""
    out = {}
    for r in rows:
        for g in r["sites"]:
            acc = out.setdefault((int(g), r["strand"]), [0, 0, 0, 0, 0.0])
            acc[0] += 1
            acc[1 + CALLS.index(r["call"])] += 1
            acc[4] += r["delta"]
    return out


def site_lines(rows, genome):
    """mod_sites.tsv: one row per site and strand with a scored group: groups scored, modified, canonical, ambiguous, fraction =
    modified / (modified + canonical) ('nan' without either) and the mean delta."""
    lines = ["\t".join(SITE_COLUMNS) + "\n"]
    for (g, strand), (n, mod, can, amb, total) in sorted(site_table(rows).items()):
        contig, pos = _place(genome, g)
        lines.append("%s\t%d\t%s\t%d\t%d\t%d\t%d\t%s\t%.4f\n" % (contig, pos, "+-"[strand], n, mod, can, amb,
                                                             "%.4f" % (mod / (mod + can)) if mod + can else "nan", total / n))
    return lines


def write_outputs(out_dir, result, genome, report):
    """mod_calls.tsv, mod_sites.tsv and modcall_report.json under out_dir; returns the report."""
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "mod_calls.tsv"), "w") as f:
        f.write("".join(call_lines(result["rows"], genome)))
    with open(os.path.join(out_dir, "mod_sites.tsv"), "w") as f:
        f.write("".join(site_lines(result["rows"], genome)))
    report = dict(report, groups=result["groups"], calls=result["calls"], batches=result["batches"], sites=len(site_table(result["rows"])),
                  files=["mod_calls.tsv", "mod_sites.tsv"])
    with open(os.path.join(out_dir, "modcall_report.json"), "w") as f:
        json.dump(report, f, indent=1)
    return report


def load_tables(table, alt_table, min_events=5):
    """(k, canonical, alternative) of two kmer_levels.tsv files; they must have the same k."""
    k, canonical = squiggle.load_level_table(table, min_events)
    k_alt, alternative = squiggle.load_level_table(alt_table, min_events)
    if k != k_alt:
        raise ValueError("%s holds %d-mers and %s %d-mers: the two tables must have the same k" % (table, k, alt_table, k_alt))
    return k, canonical, alternative


def modcall_command(args, scorer=None):
    """The `modcall` command: mapped.sam + the reads' signals + the genome + a model + two level tables -> mod_calls.tsv,
    mod_sites.tsv and modcall_report.json; returns the report."""
    import torch  # noqa: F401  the later stages take their workspaces from torch: its runtime has to be up before the engine loads the library (_lib.py)
    from . import map as map_mod, model as model_mod
    from .engine import Engine
    _motif_codes(args.motif, args.motif_offset)
    if args.flank < 0:
        raise ValueError("--flank %d is negative" % args.flank)
    k, canonical, alternative = load_tables(args.table, args.alt_table, args.table_min_events)      # read before the engine starts
    sam = squiggle._sam_of(args.input)
    genome = map_mod.load_genome(args.genome)
    spec, weights, _ = model_mod.load_model(args.model, allow_synthetic=args.synthetic_weights)
    low = []
    with Engine(spec, weights, max_batch=args.batch_size, segment_len=args.segment_len, device_id=args.device, dtype=args.dtype) as eng:
        ratio = eng.ratio
        loaded = squiggle.load_sample(sam, args.signal, genome, eng, args.batch_size, args.min_mapq, low)
    kept, read_drops = squiggle.prepare(loaded, args.segment_len, ratio, args.normalize, args.band, args.max_band, args.workspace_mb, args.device)
    result = modcall(kept, genome, (canonical, alternative), k, args.motif, args.motif_offset, args.flank, args.min_delta, args.workspace_mb,
                     args.device, scorer)
    report = {"input": args.input, "sam": sam, "signal": args.signal, "genome": args.genome, "model": args.model, "table": args.table,
              "alt_table": args.alt_table, "k": k, "table_min_events": args.table_min_events,
              "kmers_known": [int((canonical != UNKNOWN).sum()), int((alternative != UNKNOWN).sum())], "motif": args.motif,
              "motif_offset": args.motif_offset, "flank": args.flank, "min_delta": args.min_delta, "min_delta_tuned_on_real_reads": False,
              "normalize": args.normalize, "scale": SCALE, "segment_len": args.segment_len, "dtype": args.dtype, "band": args.band,
              "max_band": args.max_band, "workspace_mb": args.workspace_mb, "ratio": ratio, "min_mapq": args.min_mapq, "low_mapq": low[0],
              "reads": {"total": len(loaded), "used": len(kept), "dropped": read_drops}}
    return write_outputs(args.output, result, genome, report)
