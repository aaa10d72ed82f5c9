"""Locate: where on a genome a stretch of raw signal comes from, without calling its bases.

Every other stage that puts a read on a genome starts from called bases.  This one starts from the samples and a pore model -- the
kmer_levels.tsv that `squiggle --kmer` writes: the genome becomes one row of expected levels for both strands (reference_levels), a
read's first few thousand samples, normalised as squiggle normalises them, become a query (query_of), and the library's
chiron_signal_locate (csrc/locate.hip) runs an exact subsequence dynamic time warping of every query against every column of that
row.  It is what adaptive-sampling and target-enrichment tools compute (UNCALLED, Sigmap, RawHash, DTWax), here without seeding or
banding: every cell of Q x R is visited.

The library gives, per query and per block of 1024 columns, the least cost of a path that ends in the block, the column where it
ends and the column where it starts.  summarise turns those triples into a best locus, its cost per sample, and a margin to the
best block that lies a whole query away; both the GPU path and the tests' reference go through it, so they agree exactly.

The DP is the library's; everything else is plain numpy.  There is no CPU fallback: the hook locator= exists for the tests'
reference.  Costs are in squiggle's int16 units, 256 to one MAD-scaled unit of current.

With events= (`locate --events`) the query is not the samples but the levels of the events that the library's host-only detector
chiron_signal_events cuts them into (events_of), about one a base, and the DP is chiron_event_locate (csrc/event_locate.hip), whose
path may skip a column at a penalty: a detector that misses a border leaves a base without an event.  A row of the DP is an event, so
a prefix may be as long as 2^17 samples as long as it gives at most 8192 events; more are cut off and counted."""
import json
import os

import numpy as np

from . import _lib, label, squiggle

BREAK, NONE = _lib.LOCATE_BREAK, _lib.LOCATE_NONE
MAX_QUERY, BLOCK, MAX_REF = _lib.LOCATE_MAX_QUERY, _lib.LOCATE_BLOCK, _lib.LOCATE_MAX_REF
CHUNK, THREADS, MAX_GROUPS = _lib.LOCATE_CHUNK, _lib.LOCATE_THREADS, _lib.LOCATE_MAX_GROUPS
READ_DROPS = ("too_short", "flat_signal")
STATUSES = ("placed", "ambiguous", "unplaced")
LOCATED_COLUMNS = ("read", "samples", "contig", "start", "end", "strand", "cost_per_sample", "margin", "status")
DEFAULT_PREFIX, DEFAULT_MIN_SAMPLES = 2000, 200
DEFAULT_MIN_MARGIN = 1.0                 # int16 units a sample; not tuned on real reads
EVENT_MAX_SAMPLES, EVENT_MAX_QUERY, EVENT_MAX_PENALTY = _lib.EVENT_MAX_SAMPLES, _lib.EVENT_MAX_QUERY, _lib.EVENT_MAX_PENALTY
EVENT_DEFAULTS = {"window": 3, "threshold": 3.0, "radius": 2, "penalty": 150}        # threshold: t^2; not tuned on real reads
_COMPLEMENT = np.array([3, 2, 1, 0, 4], dtype=np.int64)


# ----------------------------------------------------------------------------------------------------------------------------
# the reference: expected levels of both strands, and the way back from a column
# ----------------------------------------------------------------------------------------------------------------------------
class ColumnMap(object):
    """Where the columns of reference_levels' row lie on the genome.  Per contig c the row holds its len_c forward columns, one
    break, its len_c reverse columns -- the reverse complement read left to right, as a reverse-strand read's signal runs -- and,
    before the next contig, one more break.  first[2 c + strand] is the first column of that stretch."""

    def __init__(self, names, lengths):
        self.names = list(names)
        self.lengths = np.asarray(lengths, dtype=np.int64)
        first, at = [], 0
        for n in self.lengths.tolist():
            first += [at, at + n + 1]
            at += 2 * n + 2
        self.first = np.asarray(first, dtype=np.int64)
        self.columns = max(at - 1, 0)                    # no break behind the last contig

    def column_to_locus(self, col):
        """(contig index, 0-based position on the contig's forward strand, strand 0 forward / 1 reverse) of a column, or None for a
        break or a column outside the row."""
        col = int(col)
        if not 0 <= col < self.columns:
            return None
        seg = int(np.searchsorted(self.first, col, side="right") - 1)
        c, strand = seg // 2, seg % 2
        i = col - int(self.first[seg])
        n = int(self.lengths[c])
        if i >= n:
            return None
        return c, (n - 1 - i if strand else i), strand

    def locus_to_column(self, contig, pos, strand):
        n = int(self.lengths[contig])
        if not 0 <= pos < n:
            raise ValueError("position %d outside contig %s of %d bases" % (pos, self.names[contig], n))
        return int(self.first[2 * contig + int(strand)]) + (n - 1 - int(pos) if strand else int(pos))


def column_to_locus(column_map, col):
    """ColumnMap.column_to_locus as a function."""
    return column_map.column_to_locus(col)


def _strand_levels(codes, table, k):
    """int32 [len(codes)]: the table's level of the k-mer around every position, the position itself at index k // 2 of it
    (squiggle.kmer_bins' convention); BREAK where the window leaves the sequence, holds a code above 3, or has no entry."""
    n, h = len(codes), k // 2
    out = np.full(n, BREAK, dtype=np.int32)
    if n >= k:
        win = codes[np.arange(n - k + 1)[:, None] + np.arange(k)[None, :]]
        code = (np.minimum(win, 3) * (4 ** np.arange(k - 1, -1, -1, dtype=np.int64))[None, :]).sum(axis=1)
        lv = table[code]
        out[h:h + n - k + 1] = np.where((win <= 3).all(axis=1) & (lv != squiggle.UNKNOWN), lv, BREAK)
    return out


def reference_levels(genome, table, k):
    """The genome as one row of expected levels under a k-mer level table (squiggle.load_level_table / table_of).
    -> (int32 [columns], ColumnMap).  Per contig: the forward levels, a break, the levels of the reverse complement; a break between
    contigs.  A break also stands where the k-mer window leaves the contig, on N, and for k-mers the table gave UNKNOWN."""
    table = np.asarray(table, dtype=np.int32)
    if not 1 <= k <= squiggle.MAX_K or table.shape != (4 ** k,):
        raise ValueError("a table of %s entries for k = %d" % (table.shape, k))
    known = table[table != squiggle.UNKNOWN]
    if known.size and (known.min() < -32767 or known.max() > 32767):
        raise ValueError("the table holds levels outside -32767 .. 32767")
    cmap = ColumnMap(genome.names, genome.lengths)
    if cmap.columns > MAX_REF:
        raise ValueError("both strands of the genome are %d columns, at most %d" % (cmap.columns, MAX_REF))
    row = np.full(cmap.columns, BREAK, dtype=np.int32)
    codes = np.asarray(genome.codes, dtype=np.int64)
    for c, n in enumerate(cmap.lengths.tolist()):
        fwd = codes[int(genome.starts[c]):int(genome.starts[c]) + n]
        a, b = int(cmap.first[2 * c]), int(cmap.first[2 * c + 1])
        row[a:a + n] = _strand_levels(fwd, table, k)
        row[b:b + n] = _strand_levels(_COMPLEMENT[fwd[::-1]], table, k)
    return row, cmap


# ----------------------------------------------------------------------------------------------------------------------------
# queries, the library call, the summary
# ----------------------------------------------------------------------------------------------------------------------------
def query_of(signal, skip=0, prefix=DEFAULT_PREFIX, mode="mad", min_samples=DEFAULT_MIN_SAMPLES, limit=MAX_QUERY):
    """squiggle.normalise of signal[skip : skip + prefix], on that prefix only.  -> (int16 query, None), or (None, reason) for a
    prefix of fewer than min_samples samples (too_short) or a flat one (flat_signal: one value throughout, or under mad a MAD of 0).
    limit: the longest prefix there may be (EVENT_MAX_SAMPLES where the query goes through events_of)."""
    if not 1 <= prefix <= limit:
        raise ValueError("prefix %d outside 1 .. %d" % (prefix, limit))
    part = np.asarray(signal).reshape(-1)[max(int(skip), 0):max(int(skip), 0) + int(prefix)]
    if len(part) < max(int(min_samples), 1):
        return None, "too_short"
    q = squiggle.normalise(part, mode)
    if q is None or part.min() == part.max():           # no spread to scale by (mad), or one value throughout
        return None, "flat_signal"
    return q, None


def workspace_size(items, samples, ref_len):
    """chiron_signal_locate_workspace_size (host-only)."""
    return _lib.sized("chiron_signal_locate_workspace_size", int(items), int(samples), int(ref_len))


def workspace_size_events(items, events, ref_len):
    """chiron_event_locate_workspace_size (host-only)."""
    return _lib.sized("chiron_event_locate_workspace_size", int(items), int(events), int(ref_len))


def event_threshold(t2):
    """The detector's integer threshold of a t^2: round(256 t^2)."""
    return int(round(256.0 * float(t2)))


def events_of(query, window=EVENT_DEFAULTS["window"], threshold=event_threshold(EVENT_DEFAULTS["threshold"]), radius=EVENT_DEFAULTS["radius"],
              max_events=EVENT_MAX_QUERY):
    """chiron_signal_events (host-only) on one int16 query; threshold is the integer one, 256 t^2.
    -> (int16 levels [count], int32 borders [count + 1], truncated): event k is query[borders[k] : borders[k + 1]]."""
    x = np.ascontiguousarray(query, dtype=np.int16).reshape(-1)
    n = len(x)
    off = np.array([0, n], dtype=np.int64)
    count, truncated = np.zeros(1, np.int32), np.zeros(1, np.uint8)
    border, level = np.zeros(n + 1, np.int32), np.zeros(max(n, 1), np.int16)
    _lib.check(_lib.load().chiron_signal_events(x.ctypes.data if n else None, off.ctypes.data, 1, int(window), int(radius), int(threshold), int(max_events), 0,
                                                count.ctypes.data, border.ctypes.data, level.ctypes.data, truncated.ctypes.data))
    c = int(count[0])
    return level[:c].copy(), border[:c + 1].copy(), bool(truncated[0])


def blocks_of_ref(ref_len):
    return (int(ref_len) + BLOCK - 1) // BLOCK


def _dp_call(entry, size, who, what, queries, ref, extra, device_id):
    """One call of a locate entry point of the library: queries and ref as locate_call takes them, extra the arguments between
    ref_len and block_out, size the entry's workspace size function, who and what the names _lib.device_workspace reports under."""
    qs = [np.ascontiguousarray(q, dtype=np.int16).reshape(-1) for q in queries]
    level = np.ascontiguousarray(np.concatenate([np.asarray(ref, dtype=np.int32).reshape(-1), np.zeros(1, np.int32)]))
    items, ref_len = len(qs), len(level) - 1
    off = label._offsets([len(q) for q in qs])
    values = np.ascontiguousarray(np.concatenate(qs + [np.zeros(1, np.int16)]))
    out = np.zeros((items, blocks_of_ref(ref_len), 3), dtype=np.int32)
    args = (values.ctypes.data, off.ctypes.data, items, level.ctypes.data, ref_len) + tuple(extra) + (out.ctypes.data if out.size else None,)
    if items == 0 or ref_len == 0:                      # nothing to compute: the library checks its arguments and touches no device
        _lib.check(getattr(_lib.load(), entry)(device_id, *args, None, 0, 0, None))
        return out
    import torch  # noqa: F401  before the size function loads the library: torch's ROCm runtime has to come up first (_lib.py)
    need = size(items, int(off[-1]), ref_len)
    lib, ws, stream = _lib.device_workspace(need, device_id, who, what)
    _lib.check(getattr(lib, entry)(device_id, *args, ws.data_ptr(), need, 0, stream))
    del ws
    return out


def event_locate_call(queries, ref, penalty=EVENT_DEFAULTS["penalty"], device_id=0):
    """One chiron_event_locate call.  queries: int16 arrays of 1 .. EVENT_MAX_QUERY event levels; ref: int32 levels or BREAK; penalty:
    what a skipped column costs, 0 .. EVENT_MAX_PENALTY.  -> int32 [items][blocks][3], as locate_call."""
    return _dp_call("chiron_event_locate", workspace_size_events, "locate.event_locate_call", "event locate kernel", queries, ref, (int(penalty),), device_id)


def locate_call(queries, ref, device_id=0):
    """One chiron_signal_locate call.  queries: int16 arrays of 1 .. MAX_QUERY samples; ref: int32 levels or BREAK.
    -> int32 [items][blocks][3]: per block of BLOCK columns the least cost of a path that ends in it, the smallest column where one
    ends, and the smallest column where such a path starts; NONE in all three for a block without a path."""
    return _dp_call("chiron_signal_locate", workspace_size, "locate.locate_call", "locate kernel", queries, ref, (), device_id)


def summarise(blocks, q_len):
    """One query's block triples int32 [blocks][3] -> dict(best = (cost, end column, start column) or None, second = the least cost
    among the blocks whose end column lies more than q_len columns from the best end, or None, per_sample = best cost / q_len,
    margin = (second - best) / q_len or None).  The best is the least cost at the smallest column."""
    b = np.asarray(blocks, dtype=np.int64).reshape(-1, 3)
    live = b[b[:, 0] != NONE]
    if len(live) == 0:
        return {"best": None, "second": None, "per_sample": None, "margin": None}
    first = live[np.lexsort((live[:, 1], live[:, 0]))[0]]
    away = live[np.abs(live[:, 1] - first[1]) > int(q_len)]
    second = int(away[:, 0].min()) if len(away) else None
    return {"best": (int(first[0]), int(first[1]), int(first[2])), "second": second, "per_sample": int(first[0]) / int(q_len),
            "margin": None if second is None else (second - int(first[0])) / int(q_len)}


def plan_batches(lengths, ref_len, budget_bytes, size=workspace_size):
    """Consecutive runs of queries [(first, last + 1)] whose call fits the budget, each the longest that does (the size grows with
    every query: bisection over the host-only size function `size`); a query that alone exceeds it gets a run of its own."""
    off = label._offsets(lengths)
    n, runs, first = len(lengths), [], 0
    while first < n:
        lo, hi = first + 1, n
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if size(mid - first, int(off[mid] - off[first]), ref_len) <= budget_bytes:
                lo = mid
            else:
                hi = mid - 1
        runs.append((first, lo))
        first = lo
    return runs


def locate(reads, ref, column_map, skip=0, prefix=DEFAULT_PREFIX, mode="mad", min_samples=DEFAULT_MIN_SAMPLES, max_cost=None,
           min_margin=DEFAULT_MIN_MARGIN, workspace_mb=4096, device_id=0, locator=None, events=None):
    """reads: [(name, samples as read)].  Every read's query against the row `ref`, in calls planned against workspace_mb.
    locator(queries, ref) -> int32 [items][blocks][3] replaces the library call (the tests' reference).
    -> dict(rows: per kept read dict(read, samples, contig, start, end, strand, cost_per_sample, margin, status, end_column,
    start_column), dropped: counts by reason, status: counts, batches).  start .. end is the 0-based half-open stretch of the
    contig's forward strand the path covers.  status: unplaced without any path or with a cost per sample above max_cost;
    ambiguous with a margin below min_margin; placed otherwise (a read without a second locus has no margin and is placed).
    events: None, or a dict over EVENT_DEFAULTS (window, threshold as t^2, radius, penalty).  Then the prefix may be as long as
    EVENT_MAX_SAMPLES, a read's query is events_of its normalised prefix, at most EVENT_MAX_QUERY events, and the call is
    event_locate_call (locator(queries, ref) gets the event levels).  A row has `events` as well; cost_per_sample and margin are
    per event, not per sample; a path spans at most 2 x events columns, which is what a second locus has to lie away by.  The result
    has truncated (reads whose events were cut off at EVENT_MAX_QUERY) and samples_per_event (the mean over all reads) as well."""
    ev = None if events is None else dict(EVENT_DEFAULTS, **events)
    if ev is not None and set(ev) != set(EVENT_DEFAULTS):
        raise ValueError("events= takes %s, not %s" % (sorted(EVENT_DEFAULTS), sorted(set(ev) - set(EVENT_DEFAULTS))))
    if locator is None:
        import torch  # noqa: F401  before the planner loads the library: torch's ROCm runtime has to come up first (_lib.py)

        def locator(queries, level):
            return locate_call(queries, level, device_id) if ev is None else event_locate_call(queries, level, ev["penalty"], device_id)
    ref = np.asarray(ref, dtype=np.int32)
    dropped = {reason: 0 for reason in READ_DROPS}
    names, used, queries, truncated = [], [], [], 0
    for name, signal in reads:
        q, reason = query_of(signal, skip, prefix, mode, min_samples, MAX_QUERY if ev is None else EVENT_MAX_SAMPLES)
        if q is None:
            dropped[reason] += 1
            continue
        names.append(name)
        used.append(len(q))
        if ev is not None:
            q, _, cut = events_of(q, ev["window"], event_threshold(ev["threshold"]), ev["radius"], EVENT_MAX_QUERY)
            truncated += int(cut)
        queries.append(q)
    size = workspace_size if ev is None else workspace_size_events
    batches = plan_batches([len(q) for q in queries], len(ref), int(workspace_mb * (1 << 20)), size) if queries else []
    rows, counts = [], {s: 0 for s in STATUSES}
    for first, last in batches:
        got = np.asarray(locator(queries[first:last], ref))
        for name, n, q, blocks in zip(names[first:last], used[first:last], queries[first:last], got):
            s = summarise(blocks, len(q) if ev is None else 2 * len(q))
            row = {"read": name, "samples": n, "contig": None, "start": None, "end": None, "strand": None, "cost_per_sample": s["per_sample"],
                   "margin": s["margin"], "end_column": None, "start_column": None}
            if ev is not None:                                                  # summarise divided by 2 x events: per event instead
                row["events"] = len(q)
                row["cost_per_sample"] = None if s["best"] is None else s["best"][0] / len(q)
                row["margin"] = None if s["second"] is None else (s["second"] - s["best"][0]) / len(q)
            if s["best"] is None or (max_cost is not None and row["cost_per_sample"] > max_cost):
                row["status"] = "unplaced"
            else:
                row["status"] = "ambiguous" if row["margin"] is not None and row["margin"] < min_margin else "placed"
            if s["best"] is not None:
                _, end_col, start_col = s["best"]
                c, at_end, strand = column_map.column_to_locus(end_col)
                _, at_start, _ = column_map.column_to_locus(start_col)         # no path crosses a break: the same contig and strand
                lo, hi = (at_end, at_start) if strand else (at_start, at_end)
                row.update(contig=column_map.names[c], start=lo, end=hi + 1, strand="+-"[strand], end_column=end_col, start_column=start_col)
            counts[row["status"]] += 1
            rows.append(row)
    out = {"rows": rows, "dropped": dropped, "status": counts, "batches": len(batches)}
    if ev is not None:
        total = sum(len(q) for q in queries)
        out.update(truncated=truncated, samples_per_event=(sum(used) / total if total else None))
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# files and the command
# ----------------------------------------------------------------------------------------------------------------------------
def parse_targets(text, column_map):
    """'contig:start-end,...' (1-based, inclusive, as samtools words a region; a bare contig is all of it) -> [(contig index,
    0-based start, end)]."""
    out = []
    for part in [p for p in (text or "").split(",") if p.strip()]:
        name, _, span = part.strip().partition(":")
        if name not in column_map.names:
            raise ValueError("--targets: no contig %r in the genome" % name)
        c = column_map.names.index(name)
        lo, hi = 0, int(column_map.lengths[c])
        if span:
            a, _, b = span.partition("-")
            try:
                lo, hi = int(a.replace(",", "")) - 1, int(b.replace(",", ""))
            except ValueError:
                raise ValueError("--targets: %r is not contig:start-end" % part)
            if not 0 <= lo < hi <= int(column_map.lengths[c]):
                raise ValueError("--targets: %r leaves contig %s of %d bases" % (part, name, int(column_map.lengths[c])))
        out.append((c, lo, hi))
    return out


def on_target(row, targets, column_map):
    """Whether a located row's stretch overlaps one of parse_targets' stretches."""
    if row["contig"] is None:
        return False
    c = column_map.names.index(row["contig"])
    return any(c == tc and row["start"] < hi and row["end"] > lo for tc, lo, hi in targets)


def located_lines(rows, targets=None, column_map=None, events=False):
    """located.tsv: one row per read that gave a query.  events: a column `events` behind `samples` (locate(events=...)'s rows;
    cost_per_sample and margin are per event there)."""
    columns = LOCATED_COLUMNS[:2] + (("events",) if events else ()) + LOCATED_COLUMNS[2:]
    lines = ["\t".join(columns + (("target",) if targets is not None else ())) + "\n"]
    for r in rows:
        placed = r["contig"] is not None
        fields = [r["read"], str(r["samples"]), r["contig"] if placed else ".", str(r["start"]) if placed else ".", str(r["end"]) if placed else ".",
                  r["strand"] if placed else ".", "%.3f" % r["cost_per_sample"] if r["cost_per_sample"] is not None else ".",
                  "%.3f" % r["margin"] if r["margin"] is not None else ".", r["status"]]
        if events:
            fields.insert(2, str(r["events"]))
        if targets is not None:
            fields.append("on_target" if r["status"] == "placed" and on_target(r, targets, column_map) else "off_target")
        lines.append("\t".join(fields) + "\n")
    return lines


def find_reads(path):
    """[(name, path, kind)] of the .signal files under <path>/raw or <path>, or else of the .fast5 files under <path>."""
    signals = label.find_signals(path)
    if signals:
        return [(name, p, "signal") for name, p in signals]
    return [(os.path.splitext(f)[0], os.path.join(path, f), "fast5") for f in sorted(os.listdir(path)) if f.endswith(".fast5")]


def load_reads(path):
    """[(name, float32 samples)] through signal_io, unnormalised: query_of normalises the prefix it cuts."""
    from . import signal_io
    out = []
    for name, p, kind in find_reads(path):
        read = signal_io.read_signal if kind == "signal" else signal_io.read_signal_fast5
        out.append((name, np.asarray(read(p, normalize=signal_io.SIG_NORM))))
    return out


def locate_command(args, locator=None):
    """The `locate` command: signals + genome + level table -> located.tsv and locate_report.json; returns the report.  locator=
    is locate()'s hook."""
    from . import map as map_mod
    k, table = squiggle.load_level_table(args.table, args.table_min_events)        # read before anything else: a wrong file ends here
    genome = map_mod.load_genome(args.genome)
    ref, cmap = reference_levels(genome, table, k)
    targets = parse_targets(args.targets, cmap) if args.targets else None
    reads = load_reads(args.signal)
    if not reads:
        raise ValueError("no .signal or .fast5 file under %s" % args.signal)
    ev = None
    if getattr(args, "events", False):
        ev = {"window": args.event_window, "threshold": args.event_threshold, "radius": args.event_radius, "penalty": args.skip_penalty}
        if not 2 <= ev["window"] <= _lib.EVENT_MAX_WINDOW or not 1 <= ev["radius"] <= _lib.EVENT_MAX_RADIUS:
            raise ValueError("--event-window outside 2 .. %d or --event-radius outside 1 .. %d" % (_lib.EVENT_MAX_WINDOW, _lib.EVENT_MAX_RADIUS))
        if not 1 <= event_threshold(ev["threshold"]) <= _lib.EVENT_MAX_THRESHOLD or not 0 <= ev["penalty"] <= EVENT_MAX_PENALTY:
            raise ValueError("--event-threshold below 1 / 256 or --skip-penalty outside 0 .. %d" % EVENT_MAX_PENALTY)
    got = locate(reads, ref, cmap, skip=args.skip, prefix=args.prefix, mode=args.normalize, min_samples=args.min_samples, max_cost=args.max_cost,
                 min_margin=args.min_margin, workspace_mb=args.workspace_mb, device_id=args.device, locator=locator, events=ev)
    os.makedirs(args.output, exist_ok=True)
    with open(os.path.join(args.output, "located.tsv"), "w") as f:
        f.write("".join(located_lines(got["rows"], targets, cmap, events=ev is not None)))
    report = {"signal": args.signal, "genome": args.genome, "table": args.table, "k": k, "table_min_events": args.table_min_events,
              "kmers_known": int((table != squiggle.UNKNOWN).sum()), "skip": args.skip, "prefix": args.prefix, "min_samples": args.min_samples,
              "normalize": args.normalize, "scale": squiggle.SCALE, "max_cost": args.max_cost, "min_margin": args.min_margin,
              "workspace_mb": args.workspace_mb, "columns": int(len(ref)), "break_columns": int((ref == BREAK).sum()),
              "reads": {"total": len(reads), "used": len(got["rows"]), "dropped": got["dropped"]}, "status": got["status"], "batches": got["batches"],
              "files": ["located.tsv"]}
    if ev is not None:                                  # cost_per_sample, margin, --max-cost and --min-margin are per event here
        report["events"] = {"window": ev["window"], "threshold": ev["threshold"], "threshold_int": event_threshold(ev["threshold"]), "radius": ev["radius"],
                            "skip_penalty": ev["penalty"], "max_events": EVENT_MAX_QUERY, "truncated": got["truncated"],
                            "samples_per_event": got["samples_per_event"], "cost_unit": "per_event"}
    if targets is not None:
        report["targets"] = args.targets
        report["on_target"] = sum(1 for r in got["rows"] if r["status"] == "placed" and on_target(r, targets, cmap))
    with open(os.path.join(args.output, "locate_report.json"), "w") as f:
        json.dump(report, f, indent=1)
    return report
