"""Demux: split called reads of a multiplexed run by barcode and cut barcode and adapter sequence off their ends.

Every read gives two windows (end_windows): its first `window` bases, and its last `window` bases reversed.  Each window is
searched for every barcode on the GPU (chiron_demux_windows, csrc/demux.hip: the bit-parallel edit-distance automaton, one pattern a
lane, exact at any distance), which answers per window the best barcode, its edit distance, where it ends, and the distance of the
best barcode of another group.  The tail window is the read end reversed and NOT complemented, so it is searched with each barcode's
complement -- the reversed reverse-complement, what a barcode ligated to the other strand's start reads like from the read's end
inwards -- and both ends report the INNER boundary of the barcode as `end`: the head is cut at end, the tail at length - end.
classify turns the two ends into a barcode, `conflict` or `unclassified`; trim cuts at the hits.

A barcode file with a single adapter is plain adapter trimming into one bin.  Records of the barcode FASTA that share a name are
spellings of one barcode: they share a group and a bin and do not compete with each other for the margin.

The defaults (window 150, max_err 0.2, min_margin 2) are plausible for 24-base barcodes behind up to a hundred bases of adapter;
nobody has measured them on real reads.

Matching is the library's; everything else is plain numpy.  There is no CPU fallback: the hook matcher= exists for the tests' numpy
reference."""
import json
import os

import numpy as np

from . import _lib, assess

MAX_PATTERN, MAX_WINDOW, MAX_PATTERNS = _lib.DEMUX_MAX_PATTERN, _lib.DEMUX_MAX_WINDOW, _lib.DEMUX_MAX_PATTERNS
THREADS, MAX_GROUPS, NONE = _lib.DEMUX_THREADS, _lib.DEMUX_MAX_GROUPS, _lib.DEMUX_NONE
MAX_WINDOWS = 1 << 24                   # windows of one call
WINDOW, MAX_ERR, MIN_MARGIN = 150, 0.2, 2
REQUIRE = ("either", "both")
STATUSES = ("classified", "unclassified", "conflict", "empty")
UNCLASSIFIED = "unclassified"           # the bin of the unclassified and the conflicting reads
RESULT_KEYS = ("best", "dist", "end", "second")
TSV_COLUMNS = ("read", "length", "head_best", "head_dist", "head_end", "head_second", "head_hit", "tail_best", "tail_dist", "tail_end",
               "tail_second", "tail_hit", "status", "barcode", "kept_start", "kept_end")
_COMPLEMENT = np.array([3, 2, 1, 0, 4], dtype=np.uint8)


# ----------------------------------------------------------------------------------------------------------------------------
# patterns and windows
# ----------------------------------------------------------------------------------------------------------------------------
def load_patterns(fasta):
    """(names, codes) of the records of a barcode FASTA, in file order: names[q] the header's first word, codes[q] uint8 0..4.
    Records that share a name are spellings of one barcode (groups_of)."""
    records = assess.read_records(fasta)
    if not records:
        raise ValueError("%s holds no barcode" % fasta)
    for name, seq in records:
        if not 1 <= len(seq) <= MAX_PATTERN:
            raise ValueError("%s: barcode %s has %d bases, 1 to %d are searched" % (fasta, name, len(seq), MAX_PATTERN))
        if not name or "/" in name or name.startswith(".") or name == UNCLASSIFIED:
            raise ValueError("%s: barcode name %r cannot name a bin file" % (fasta, name))
    return [name for name, _ in records], [assess.encode(seq) for _, seq in records]


def groups_of(names):
    """(groups int32 [patterns], bins): the bin names in order of first appearance and every pattern's index into them."""
    bins = []
    for name in names:
        if name not in bins:
            bins.append(name)
    return np.array([bins.index(name) for name in names], dtype=np.int32), bins


def complement(codes):
    """A pattern as the reversed tail window shows it: complemented, not reversed."""
    return _COMPLEMENT[np.asarray(codes, dtype=np.uint8)]


def end_windows(reads, window=WINDOW):
    """(heads, tails) of reads (str, bytes or uint8 codes): read[:window], and read[-window:] reversed (not complemented).  A read
    shorter than `window` gives two overlapping windows of its whole length; a read of 0 bases two empty ones."""
    if not 1 <= window <= MAX_WINDOW:
        raise ValueError("window %d outside 1 .. %d" % (window, MAX_WINDOW))
    codes = [assess.encode(r) for r in reads]
    heads = [np.ascontiguousarray(c[:window]) for c in codes]
    tails = [np.ascontiguousarray(c[max(len(c) - window, 0):][::-1]) for c in codes]
    return heads, tails


# ----------------------------------------------------------------------------------------------------------------------------
# the kernel
# ----------------------------------------------------------------------------------------------------------------------------
def workspace_size(windows, window_bytes, patterns, want_matrix=False):
    """chiron_demux_workspace_size (host-only)."""
    return _lib.sized("chiron_demux_workspace_size", int(windows), int(window_bytes), int(patterns), int(bool(want_matrix)))


def plan_batches(window_lens, patterns, budget_bytes, want_matrix=False):
    """Consecutive runs of windows, [(first, last + 1)], as few as budget_bytes allows: every run is the longest whose workspace fits
    (the size grows with every window, so the longest fitting run is found by bisection), and never more than MAX_WINDOWS.  A
    window that alone exceeds the budget gets a run of its own.  Uses only the host-only size function."""
    total = np.concatenate([[0], np.cumsum(np.asarray(window_lens, dtype=np.int64))])
    n, runs, first = len(window_lens), [], 0
    while first < n:
        lo, hi = first + 1, min(n, first + MAX_WINDOWS)         # the run ends in lo .. hi; a single window always goes
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if workspace_size(mid - first, int(total[mid] - total[first]), patterns, want_matrix) <= budget_bytes:
                lo = mid
            else:
                hi = mid - 1
        runs.append((first, lo))
        first = lo
    return runs


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.int64)


def match_call(windows, patterns, groups, want_matrix=False, device_id=0):
    """One chiron_demux_windows call.  windows, patterns: lists of uint8 code arrays; groups: int per pattern.
    -> dict(best, dist, end, second: int32 [windows]) and, with want_matrix, pair_dist, pair_end: int16 [windows, patterns]."""
    wins = [np.ascontiguousarray(w, dtype=np.uint8).reshape(-1) for w in windows]
    pats = [np.ascontiguousarray(p, dtype=np.uint8).reshape(-1) for p in patterns]
    nw, npat = len(wins), len(pats)
    out = {k: np.zeros(nw, dtype=np.int32) for k in RESULT_KEYS}
    if want_matrix:
        out["pair_dist"] = np.zeros((nw, npat), dtype=np.int16)
        out["pair_end"] = np.zeros((nw, npat), dtype=np.int16)
    if nw == 0:
        return out
    win_off, pat_off = _offsets([len(w) for w in wins]), _offsets([len(p) for p in pats])
    win_codes = np.ascontiguousarray(np.concatenate(wins + [np.zeros(1, np.uint8)]))
    pat_codes = np.ascontiguousarray(np.concatenate(pats + [np.zeros(1, np.uint8)]))
    group = np.ascontiguousarray(np.asarray(groups, dtype=np.int32).reshape(-1))
    if len(group) != npat:
        raise ValueError("%d groups for %d patterns" % (len(group), npat))
    lib, ws, stream = _lib.device_workspace(lambda: workspace_size(nw, int(win_off[-1]), npat, want_matrix), device_id,
                                            "demux.match", "barcode search")
    _lib.check(lib.chiron_demux_windows(device_id, win_codes.ctypes.data, win_off.ctypes.data, nw, pat_codes.ctypes.data, pat_off.ctypes.data,
                                        group.ctypes.data, npat, 0, out["best"].ctypes.data, out["dist"].ctypes.data, out["end"].ctypes.data,
                                        out["second"].ctypes.data, out["pair_dist"].ctypes.data if want_matrix else None,
                                        out["pair_end"].ctypes.data if want_matrix else None, ws.data_ptr(), stream))
    del ws
    return out


def match_windows(windows, patterns, groups, workspace_mb=4096, device_id=0, want_matrix=False):
    """The best pattern of every window on the GPU, in runs planned against workspace_mb (which may be a fraction).  Heads and tails
    are searched with different patterns, so they are separate calls of this.  -> the dict of match_call plus "calls"."""
    out = {k: np.zeros(len(windows), dtype=np.int32) for k in RESULT_KEYS}
    if want_matrix:
        out["pair_dist"] = np.zeros((len(windows), len(patterns)), dtype=np.int16)
        out["pair_end"] = np.zeros((len(windows), len(patterns)), dtype=np.int16)
    if windows:
        import torch  # noqa: F401  before plan_batches loads the library: torch's ROCm runtime has to come up first (_lib.py)
    runs = plan_batches([len(w) for w in windows], len(patterns), int(workspace_mb * (1 << 20)), want_matrix)
    for first, last in runs:
        got = match_call(windows[first:last], patterns, groups, want_matrix, device_id)
        for k in got:
            out[k][first:last] = got[k]
    out["calls"] = len(runs)
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# the decision and the cut
# ----------------------------------------------------------------------------------------------------------------------------
def allowed_errors(pattern_len, max_err=MAX_ERR):
    """floor(max_err * length), the product taken 1e-9 up so that 0.2 * 25 allows 5 and not 4."""
    return np.floor(max_err * np.asarray(pattern_len, dtype=np.float64) + 1e-9).astype(np.int64)


def hits(end, pattern_lens, max_err=MAX_ERR, min_margin=MIN_MARGIN):
    """bool per window of one end (a dict of match_windows): dist <= allowed_errors(len(best)) and second - dist >= min_margin; a
    second of NONE (no pattern of another group) passes the margin."""
    best, dist, second = (np.asarray(end[k], dtype=np.int64) for k in ("best", "dist", "second"))
    lens = np.asarray(pattern_lens, dtype=np.int64)[best] if len(best) else np.zeros(0, np.int64)
    return (dist <= allowed_errors(lens, max_err)) & ((second == NONE) | (second - dist >= min_margin))


def classify(head, tail, pattern_lens, max_err=MAX_ERR, min_margin=MIN_MARGIN, require="either", groups=None):
    """Per read, from the results of its two windows: dict(head_hit, tail_hit: bool arrays; group: int32, the barcode's group or -1;
    status: list of "classified" / "unclassified" / "conflict").  groups: the patterns' groups (default: every pattern its own).
    either: one hit, or two hits that name the same group, gives that barcode; two hits that disagree are a conflict; no hit is
    unclassified.  both: both ends must hit and agree; two that disagree are a conflict, anything less is unclassified."""
    if require not in REQUIRE:
        raise ValueError("require %r is neither of %s" % (require, "/".join(REQUIRE)))
    groups = np.arange(len(pattern_lens), dtype=np.int32) if groups is None else np.asarray(groups, dtype=np.int32)
    hh, th = hits(head, pattern_lens, max_err, min_margin), hits(tail, pattern_lens, max_err, min_margin)
    n = len(hh)
    hg = groups[np.asarray(head["best"], dtype=np.int64)] if n else np.zeros(0, np.int32)
    tg = groups[np.asarray(tail["best"], dtype=np.int64)] if n else np.zeros(0, np.int32)
    group = np.full(n, -1, dtype=np.int32)
    status = []
    for r in range(n):
        if hh[r] and th[r]:
            if hg[r] == tg[r]:
                group[r] = hg[r]
                status.append("classified")
            else:
                status.append("conflict")
        elif (hh[r] or th[r]) and require == "either":
            group[r] = hg[r] if hh[r] else tg[r]
            status.append("classified")
        else:
            status.append("unclassified")
    return {"head_hit": hh, "tail_hit": th, "group": group, "status": status}


def trim(read, qual, head_hit, tail_hit):
    """Cuts at the hits only: head_hit / tail_hit are the `end` of the read's head / tail window, or None for an end without a
    hit.  -> (read[lo:hi], qual[lo:hi] or None, lo, hi) with lo = head_hit or 0 and hi = len(read) - (tail_hit or 0); None when the
    cuts meet or cross (the read is `empty`)."""
    n = len(read)
    lo = int(head_hit) if head_hit is not None else 0
    hi = n - int(tail_hit) if tail_hit is not None else n
    if lo >= hi:
        return None
    return read[lo:hi], (qual[lo:hi] if qual is not None else None), lo, hi


def demux(reads, patterns, groups, window=WINDOW, max_err=MAX_ERR, min_margin=MIN_MARGIN, require="either", do_trim=True, workspace_mb=4096,
          device_id=0, matcher=None):
    """reads: [(name, sequence str, quality str or None)]; patterns: code arrays; groups: int per pattern.
    matcher(windows, patterns, groups) -> the dict of match_windows replaces the GPU.
    -> dict(rows=[one dict per read: the TSV_COLUMNS but `barcode` as a group number, plus seq and qual as they are written],
    calls=(head calls, tail calls), fastq=every read came with qualities)."""
    if matcher is None:
        def matcher(wins, pats, grp):
            return match_windows(wins, pats, grp, workspace_mb, device_id)
    heads, tails = end_windows([seq for _, seq, _ in reads], window)
    head = matcher(heads, [np.asarray(p, dtype=np.uint8) for p in patterns], groups)
    tail = matcher(tails, [complement(p) for p in patterns], groups)
    lens = [len(p) for p in patterns]
    decided = classify(head, tail, lens, max_err, min_margin, require, groups)
    rows = []
    for r, (name, seq, qual) in enumerate(reads):
        status, lo, hi, out_seq, out_qual = decided["status"][r], 0, len(seq), seq, qual
        if status == "classified" and do_trim:
            cut = trim(seq, qual, int(head["end"][r]) if decided["head_hit"][r] else None, int(tail["end"][r]) if decided["tail_hit"][r] else None)
            if cut is None:
                status, lo, hi, out_seq, out_qual = "empty", 0, 0, "", None
            else:
                out_seq, out_qual, lo, hi = cut
        row = {"read": name, "length": len(seq), "status": status, "barcode": int(decided["group"][r]) if status in ("classified", "empty") else -1,
               "kept_start": lo, "kept_end": hi, "seq": out_seq, "qual": out_qual}
        for side, res, hit in (("head", head, decided["head_hit"]), ("tail", tail, decided["tail_hit"])):
            for k in RESULT_KEYS:
                row["%s_%s" % (side, k)] = int(res[k][r])
            row["%s_hit" % side] = int(hit[r])
        rows.append(row)
    return {"rows": rows, "calls": (int(head.get("calls", 1)), int(tail.get("calls", 1))),
            "fastq": bool(reads) and all(qual is not None for _, _, qual in reads)}


# ----------------------------------------------------------------------------------------------------------------------------
# files and the command
# ----------------------------------------------------------------------------------------------------------------------------
def read_records(path):
    """[(name, sequence, quality or None)] of a FASTA or FASTQ file: assess.read_records that keeps the quality line of the
    four-line FASTQ form.  A quality line as long as its sequence is required."""
    with open(path) as f:
        first = ""
        for line in f:
            if line.strip():
                first = line
                break
    if not first.startswith("@"):
        return [(name, seq, None) for name, seq in assess.read_records(path)]
    with open(path) as f:
        lines = [ln.rstrip("\r\n") for ln in f]
    out, i = [], 0
    while i < len(lines):
        if not lines[i].strip():
            i += 1
            continue
        if not lines[i].startswith("@") or i + 3 >= len(lines) or not lines[i + 2].startswith("+"):
            raise ValueError("%s: line %d does not start a four-line FASTQ record" % (path, i + 1))
        name, seq, qual = (lines[i][1:].split() or [""])[0], lines[i + 1].strip(), lines[i + 3].strip()
        if len(qual) != len(seq):
            raise ValueError("%s: read %s has %d bases and %d qualities" % (path, name, len(seq), len(qual)))
        out.append((name, seq, qual))
        i += 4
    return out


def load_reads(path):
    """[(name, sequence, quality or None)] in the order and under the names of assess.load_reads: a `call` output tree (its
    result/), a folder of files, or one file."""
    if os.path.isdir(path):
        sub = os.path.join(path, "result")
        folder = sub if os.path.isdir(sub) else path
        files = assess._seq_files(folder)
        files = [f for f in files if assess._stem(f) != "merged"] or files
    else:
        files = [path]
    reads = {}
    for f in files:
        recs = read_records(f)
        if len(recs) == 1:
            reads[assess._stem(f)] = recs[0][1:]
        else:
            for name, seq, qual in recs:
                reads[name] = (seq, qual)
    return [(name, seq, qual) for name, (seq, qual) in reads.items()]


def format_record(name, seq, qual):
    return "@%s\n%s\n+\n%s\n" % (name, seq, qual) if qual is not None else ">%s\n%s\n" % (name, seq)


def tsv_lines(rows, bins):
    """demux.tsv: head_best / tail_best are pattern indices into the barcode file's records, a second of NONE and the barcode of a
    read without one are '-'."""
    lines = ["\t".join(TSV_COLUMNS) + "\n"]
    for row in rows:
        shown = dict(row, barcode=bins[row["barcode"]] if row["barcode"] >= 0 else "-")
        for side in ("head", "tail"):
            if shown[side + "_second"] == NONE:
                shown[side + "_second"] = "-"
        lines.append("\t".join(str(shown[k]) for k in TSV_COLUMNS) + "\n")
    return lines


def write_outputs(out_dir, result, names, bins, meta=None):
    """<bin>.<ext> per barcode that got a read, unclassified.<ext> (the unclassified and the conflicting reads, untrimmed), demux.tsv
    and demux_report.json under out_dir; ext is fastq when every read has qualities, else fasta (qualities are then dropped).
    head_best / tail_best of demux.tsv are pattern indices into the barcode file's records.  Returns the report."""
    os.makedirs(out_dir, exist_ok=True)
    rows = result["rows"]
    fastq = result["fastq"]
    ext = "fastq" if fastq else "fasta"
    files = {}
    for row in rows:
        if row["status"] == "empty":
            continue
        target = bins[row["barcode"]] if row["status"] == "classified" else UNCLASSIFIED
        files.setdefault(target, []).append(format_record(row["read"], row["seq"], row["qual"] if fastq else None))
    for target, records in files.items():
        with open(os.path.join(out_dir, "%s.%s" % (target, ext)), "w") as f:
            f.write("".join(records))
    with open(os.path.join(out_dir, "demux.tsv"), "w") as f:
        f.write("".join(tsv_lines(rows, bins)))
    report = dict(meta or {})
    report["reads"] = len(rows)
    report["patterns"] = len(names)
    report["status"] = {s: sum(1 for row in rows if row["status"] == s) for s in STATUSES}
    report["bins"] = {b: sum(1 for row in rows if row["status"] == "classified" and row["barcode"] == k) for k, b in enumerate(bins)}
    report["files"] = sorted("%s.%s" % (target, ext) for target in files)
    report["bases"] = {"in": sum(row["length"] for row in rows), "written": sum(len(row["seq"]) for row in rows if row["status"] != "empty")}
    report["calls"] = {"head": result["calls"][0], "tail": result["calls"][1]}
    with open(os.path.join(out_dir, "demux_report.json"), "w") as f:
        json.dump(report, f, indent=1)
    return report


def demux_command(input_path, barcodes, out_dir, window=WINDOW, max_err=MAX_ERR, min_margin=MIN_MARGIN, require="either", do_trim=True,
                  workspace_mb=4096, device_id=0, matcher=None):
    """The `demux` command: called reads + a barcode FASTA -> the bin files, demux.tsv and demux_report.json; returns the report."""
    names, patterns = load_patterns(barcodes)
    groups, bins = groups_of(names)
    reads = load_reads(input_path)
    if not reads:
        raise ValueError("no read under %s" % input_path)
    result = demux(reads, patterns, groups, window, max_err, min_margin, require, do_trim, workspace_mb, device_id, matcher)
    meta = {"input": input_path, "barcodes": barcodes, "window": window, "max_err": max_err, "min_margin": min_margin, "require": require,
            "trim": bool(do_trim), "workspace_mb": workspace_mb}
    return write_outputs(out_dir, result, names, bins, meta)
