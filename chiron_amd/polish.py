"""Polish: rescore the variants a pileup proposes with the reads' own CTC likelihoods.

`pileup` ends in a majority vote over base calls.  The vote cannot tell a confident read from an ambiguous one: at low depth a
2-against-2 tie goes to the draft, and a systematic error is voted in.  The network's frame scores can.  For every candidate
variant (candidates_from_counts: from the pileup's count planes) and every read that covers it, the frames the read spent on the
flanked window are scored against the window's two alleles -- the draft's and the edited one -- by the CTC forward recurrence on
the GPU (chiron_ctc_score, csrc/ctc_score.hip: one wavefront per candidate, doubles, the frames read in place), and the variant's
log-likelihood ratio is the sum over its reads.  A greedy pass accepts the best non-overlapping variants (decide) and `apply` edits
the draft.  Every candidate is scored against the UNEDITED draft; a further round is the user's loop: `map -g polished.fasta`,
then `polish` again.

A read is (pos, ops) as in pileup.py plus what ties it to its signal: dict(name, pos, ops, reverse, called, lead, logits) --
`called` the whole called sequence in SIGNAL orientation (uint8 codes 0..3), `lead` the bases of it in genome orientation before
the first aligned one (a soft clip), `logits` float32 [frames, 5] in signal order.  Frames are tied to read bases by the forced
alignment of the logits to `called` (label.align): it is the labelling the logits fit; a genome cut 12 % away would drag the path.

Counting, aligning and scoring are the library's; everything else is plain numpy.  There is no CPU fallback: the hooks scorer= and
frame_aligner= exist for the tests' numpy references."""
import json
import os

import numpy as np

from . import _lib, assess, label, pileup

MAX_FRAMES, MAX_LABEL = _lib.SCORE_MAX_FRAMES, _lib.SCORE_MAX_LABEL
THREADS, MAX_GROUPS = _lib.SCORE_THREADS, _lib.SCORE_MAX_GROUPS
STATUS_SCORED, STATUS_INFEASIBLE = 0, 1
TYPES = ("SUB", "DEL", "INS")
VARIANT_COLUMNS = ("contig", "pos", "type", "ref", "alt", "depth", "count", "reads_scored", "llr", "accepted")
READ_DROPS = ("no_signal", "no_frames", "outside_acgt", "infeasible", "band_exhausted")
ITEM_DROPS = ("no_read_base", "too_many_frames", "allele_too_long", "infeasible")


# ----------------------------------------------------------------------------------------------------------------------------
# the kernel
# ----------------------------------------------------------------------------------------------------------------------------
def workspace_size(frames, items, candidates, label_bytes):
    """chiron_ctc_score_workspace_size (host-only)."""
    return _lib.sized("chiron_ctc_score_workspace_size", int(frames), int(items), int(candidates), int(label_bytes))


def plan_batches(items, candidates, budget_bytes):
    """Consecutive runs of items, [(first, last + 1, frame lo, frame hi)], each run's workspace within budget_bytes; a run is handed
    the frames lo .. hi) that its items span and nothing else, so items should come in frame order.  An item that alone exceeds the
    budget gets a run of its own.  Uses only the host-only size function."""
    runs, first = [], 0
    lo = hi = n_cand = n_bytes = 0
    for i, (b, e) in enumerate(items):
        c, nb = len(candidates[i]), sum(len(l) for l in candidates[i])
        if i > first and workspace_size(max(hi, e) - min(lo, b), i + 1 - first, n_cand + c, n_bytes + nb) > budget_bytes:
            runs.append((first, i, lo, hi))
            first = i
        if i == first:
            lo, hi, n_cand, n_bytes = b, e, c, nb
        else:
            lo, hi, n_cand, n_bytes = min(lo, b), max(hi, e), n_cand + c, n_bytes + nb
    if len(items) > first:
        runs.append((first, len(items), lo, hi))
    return runs


def score_call(scores, items, candidates, device_id=0):
    """One chiron_ctc_score call.  scores float32 [frames, 5]; items [(begin, end)]; candidates [[uint8 codes] per item].
    -> (loglik float64 [candidates], status int32 [candidates]), candidates in item order."""
    x = np.ascontiguousarray(scores, dtype=np.float32).reshape(-1, 5)
    labs = [np.ascontiguousarray(l, dtype=np.uint8).reshape(-1) for ls in candidates for l in ls]
    n_items, n_cand = len(items), len(labs)
    begin = np.array([b for b, _ in items] + [0], dtype=np.int64)
    end = np.array([e for _, e in items] + [0], dtype=np.int64)
    cand_off = label._offsets([len(ls) for ls in candidates])
    label_off = label._offsets([len(l) for l in labs])
    labels = np.ascontiguousarray(np.concatenate(labs + [np.zeros(1, np.uint8)]))
    loglik = np.zeros(max(n_cand, 1), dtype=np.float64)
    status = np.zeros(max(n_cand, 1), dtype=np.int32)
    if n_items == 0 or n_cand == 0:
        return loglik[:n_cand], status[:n_cand]
    lib, ws, stream = _lib.device_workspace(lambda: workspace_size(x.shape[0], n_items, n_cand, int(label_off[-1])), device_id,
                                            "polish.score", "likelihood kernel")
    _lib.check(lib.chiron_ctc_score(device_id, x.ctypes.data, x.shape[0], begin.ctypes.data, end.ctypes.data, cand_off.ctypes.data, n_items,
                                    labels.ctypes.data, label_off.ctypes.data, n_cand, 0, loglik.ctypes.data, status.ctypes.data,
                                    ws.data_ptr(), stream))
    del ws
    return loglik[:n_cand], status[:n_cand]


def score(scores, items, candidates, workspace_mb=4096, device_id=0):
    """log p(candidate | the item's frames) for every candidate of every item, on the GPU, in runs planned against workspace_mb
    (which may be a fraction).  -> {"loglik": [float64 array per item], "status": [int32 array per item]}: 0 scored, 1 infeasible
    (fewer frames than bases + adjacent equal bases; loglik -inf)."""
    if len(items) != len(candidates):
        raise ValueError("%d items against %d candidate lists" % (len(items), len(candidates)))
    x = np.ascontiguousarray(scores, dtype=np.float32).reshape(-1, 5)
    out_l, out_s = [], []
    if items:
        import torch  # noqa: F401  before plan_batches loads the library: torch's ROCm runtime has to come up first (_lib.py)
    for first, last, lo, hi in plan_batches(items, candidates, int(workspace_mb * (1 << 20))):
        ll, st = score_call(x[lo:hi], [(b - lo, e - lo) for b, e in items[first:last]], candidates[first:last], device_id)
        at = 0
        for ls in candidates[first:last]:
            out_l.append(ll[at:at + len(ls)].copy())
            out_s.append(st[at:at + len(ls)].copy())
            at += len(ls)
    return {"loglik": out_l, "status": out_s}


# ----------------------------------------------------------------------------------------------------------------------------
# candidates, segments, alleles
# ----------------------------------------------------------------------------------------------------------------------------
def threshold(depth, min_alt=2, min_frac=0.2):
    """max(min_alt, ceil(min_frac * depth)) per position; the product is taken 1e-9 short, so that 0.2 * 10 asks for 2 and not 3."""
    d = np.asarray(depth, dtype=np.float64)
    return np.maximum(int(min_alt), np.ceil(min_frac * d - 1e-9).astype(np.int64))


def candidates_from_counts(counts, depth, genome, min_alt=2, min_frac=0.2):
    """The candidate variants the count planes of pileup.count(want_counts=True) name, in position order and per position as
    substitutions (by code), the deletion, insertions (by code): every base that is not the reference base, the single-base
    deletion, and each single-base insertion directly after the position (slot 0) whose count is at least threshold(depth).
    Positions whose reference code is 4 are skipped.  -> [dict(g, type, alt, count, depth)], g in concatenated coordinates, alt a
    code (-1 for the deletion)."""
    counts = np.asarray(counts)
    ref = np.asarray(genome.codes)
    thr = threshold(depth, min_alt, min_frac)
    usable = ref != 4
    found = []
    for order, (kind, plane, code) in enumerate([("SUB", c, c) for c in range(4)] + [("DEL", pileup.PLANE_DEL, -1)] +
                                                [("INS", pileup.PLANE_INS + c, c) for c in range(4)]):
        keep = usable & (counts[plane] >= thr) & (counts[plane] > 0)
        if kind == "SUB":
            keep &= ref != code
        found += [(int(g), order, kind, code) for g in np.flatnonzero(keep)]
    found.sort()
    return [{"g": g, "type": kind, "alt": code, "count": int(counts[_plane(kind, code), g]), "depth": int(depth[g])} for g, _, kind, code in found]


def _plane(kind, code):
    return code if kind == "SUB" else pileup.PLANE_DEL if kind == "DEL" else pileup.PLANE_INS + code


def read_prefix(ops):
    """before[q], q = 0 .. m: the read-consuming columns ('=', 'X', 'I') before the q-th reference-consuming column ('=', 'X',
    'D'); before[m] is all of them."""
    ops = np.asarray(ops, dtype=np.uint8)
    consumed = np.concatenate([[0], np.cumsum(ops != 3)])
    return np.concatenate([consumed[:-1][ops != 2], consumed[-1:]]).astype(np.int64)


def segment(pos, ops, n, g0, g1, before=None):
    """The read bases an alignment (pos, ops) of a read of n aligned bases puts on the reference positions g0 .. g1): (i_lo, i_hi),
    i_lo the read-consuming columns before the reference-consuming column at g0 and i_hi the same for g1 -- every read-consuming
    column when g1 == pos + m.  An insertion counts with the reference base it follows, as in the pileup.  None unless
    pos <= g0 <= g1 <= pos + m.  The indices are in genome orientation; a reverse-strand read holds them at n - i_hi .. n - i_lo).
    before: read_prefix(ops), when the caller asks for many windows of one alignment."""
    if before is None:
        before = read_prefix(ops)
    m = len(before) - 1
    if before[-1] != n:
        raise ValueError("the columns consume %d read bases, the read has %d" % (before[-1], n))
    if not (pos <= g0 <= g1 <= pos + m):
        return None
    return int(before[g0 - pos]), int(before[g1 - pos])


def read_window(read, g0, g1, before=None):
    """The bases lo .. hi) of read["called"], in SIGNAL orientation, that the read (a dict of the module's docstring) puts on the
    reference positions g0 .. g1): segment(), moved past the leading soft clip and mirrored for a reverse-strand read.  None when
    the alignment does not cover the window; ValueError when the columns and the clip ask for more bases than the read has."""
    if before is None:
        before = read_prefix(read["ops"])
    n, lead, aligned = len(read["called"]), int(read["lead"]), int(before[-1])
    if lead < 0 or lead + aligned > n:
        raise ValueError("read %s: %d clipped and %d aligned bases, the called sequence has %d" % (read.get("name", "?"), lead, aligned, n))
    seg = segment(int(read["pos"]), read["ops"], aligned, g0, g1, before)
    if seg is None:
        return None
    lo, hi = seg[0] + lead, seg[1] + lead
    return (n - hi, n - lo) if read["reverse"] else (lo, hi)


def alleles(genome, cand, flank):
    """(reference allele, alternative allele) of a candidate: genome[g - flank .. g + flank] and the same with the edit applied;
    None when the window leaves the candidate's contig."""
    g = cand["g"]
    c = genome.contig_of(g)
    c0 = int(genome.starts[c])
    if g - flank < c0 or g + flank + 1 > c0 + int(genome.lengths[c]):
        return None
    ref = np.asarray(genome.codes[g - flank:g + flank + 1], dtype=np.uint8)
    if cand["type"] == "SUB":
        alt = ref.copy()
        alt[flank] = cand["alt"]
    elif cand["type"] == "DEL":
        alt = np.delete(ref, flank)
    else:
        alt = np.insert(ref, flank + 1, cand["alt"])
    return ref, alt.astype(np.uint8)


# ----------------------------------------------------------------------------------------------------------------------------
# the decision and the edit
# ----------------------------------------------------------------------------------------------------------------------------
def decide(records, flank, min_reads=3, min_llr=0.0):
    """Marks records (dict(g, type, alt, reads_scored, llr)) accepted or not, in place, and returns the accepted ones in position
    order.  Eligible: reads_scored >= min_reads and llr > min_llr.  Every llr was taken against the unedited draft, so the eligible
    ones are taken by descending llr (ties by position, then type, then code) and one is accepted only when no accepted variant
    lies within `flank` positions of it."""
    for r in records:
        r["accepted"] = False
    eligible = [r for r in records if r["reads_scored"] >= min_reads and r["llr"] > min_llr]
    eligible.sort(key=lambda r: (-r["llr"], r["g"], TYPES.index(r["type"]), r["alt"]))
    taken = []
    for r in eligible:
        if all(abs(r["g"] - t["g"]) > flank for t in taken):
            r["accepted"] = True
            taken.append(r)
    return sorted(taken, key=lambda r: r["g"])


def apply(genome, accepted):
    """{contig: sequence}: the genome with the accepted variants applied, at most one per position."""
    edits = {}
    for r in accepted:
        if r["g"] in edits:
            raise ValueError("two accepted variants at position %d" % r["g"])
        edits[r["g"]] = r
    out = {}
    for c, name in enumerate(genome.names):
        c0 = int(genome.starts[c])
        codes = np.asarray(genome.codes[c0:c0 + int(genome.lengths[c])], dtype=np.uint8)
        parts, at = [], 0
        for g in sorted(g for g in edits if c0 <= g < c0 + len(codes)):
            r, t = edits[g], g - c0
            parts.append(codes[at:t])
            if r["type"] == "SUB":
                parts.append(np.array([r["alt"]], np.uint8))
            elif r["type"] == "INS":
                parts.append(np.array([codes[t], r["alt"]], np.uint8))
            at = t + 1
        parts.append(codes[at:])
        out[name] = "".join("ACGTN"[v] for v in np.concatenate(parts))
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# the pipeline
# ----------------------------------------------------------------------------------------------------------------------------
def align_frames(reads, band=label.BAND0, max_band=label.MAX_BAND, workspace_mb=4096, device_id=0, frame_aligner=None):
    """label.align of every read's logits to its called sequence, in batches.  frame_aligner(scores_list, labels_list, band0,
    max_band) -> the dict of label.align replaces the GPU.  -> (start arrays with the frame count appended, status array)."""
    if frame_aligner is None:
        import torch  # noqa: F401  before plan_batches loads the library (_lib.py)

        def frame_aligner(xs, ls, b, mb):
            return label.align(xs, ls, band0=b, max_band=mb, device_id=device_id)
    starts, status = [None] * len(reads), np.zeros(len(reads), dtype=np.int32)
    frames = [r["logits"].shape[0] for r in reads]
    bases = [len(r["called"]) for r in reads]
    for batch in label.plan_batches(frames, bases, band, max_band, int(workspace_mb * (1 << 20))):
        got = frame_aligner([reads[i]["logits"] for i in batch], [reads[i]["called"] for i in batch], band, max_band)
        for k, i in enumerate(batch):
            status[i] = got["status"][k]
            starts[i] = np.concatenate([np.asarray(got["start"][k], dtype=np.int64), [frames[i]]])
    return starts, status


def polish(reads, genome, counts, depth, flank=8, min_alt=2, min_frac=0.2, min_llr=0.0, min_reads=3, band=label.BAND0,
           max_band=label.MAX_BAND, workspace_mb=4096, device_id=0, scorer=None, frame_aligner=None):
    """Candidates from the count planes, scored by every read that covers their window, decided and counted.  reads: the dicts of
    the module's docstring.  scorer(scores, items, candidates) -> the dict of `score` and frame_aligner (align_frames) replace the
    GPU.  -> dict(variants=[records in position order], accepted=[the accepted ones], report); a record is its candidate plus
    reads_scored, llr, logliks [(reference allele, alternative allele) per scoring read, in read order] and accepted."""
    if scorer is None:
        def scorer(x, items, cands):
            return score(x, items, cands, workspace_mb, device_id)
    cands = candidates_from_counts(counts, depth, genome, min_alt, min_frac)
    records, windows = [], []
    skipped = {"contig_end": 0}
    for cd in cands:
        pair = alleles(genome, cd, flank)
        if pair is None:
            skipped["contig_end"] += 1
            continue
        records.append(dict(cd, reads_scored=0, llr=0.0, logliks=[]))
        windows.append(pair)
    read_drops = {reason: 0 for reason in READ_DROPS}
    usable = []
    for r in reads:
        if r.get("logits") is None:
            read_drops["no_signal"] += 1
        elif r["logits"].shape[0] == 0 or len(r["called"]) == 0:
            read_drops["no_frames"] += 1
        elif np.any(np.asarray(r["called"]) > 3):
            read_drops["outside_acgt"] += 1
        else:
            usable.append(r)
    starts, status = align_frames(usable, band, max_band, workspace_mb, device_id, frame_aligner)
    kept = []
    for r, st, s in zip(usable, status, starts):
        if st != 0:
            read_drops[label.STATUS_NAMES[int(st)]] += 1
        else:
            kept.append((r, s))
    item_drops = {reason: 0 for reason in ITEM_DROPS}
    items, labels, owner = [], [], []
    gs = np.array([rec["g"] for rec in records], dtype=np.int64)
    frame0 = 0
    for r, start in kept:
        before = read_prefix(r["ops"])
        m, pos = len(before) - 1, int(r["pos"])
        # the candidates whose window pos <= g - flank, g + flank + 1 <= pos + m this read covers
        for v in range(int(np.searchsorted(gs, pos + flank, "left")), int(np.searchsorted(gs, pos + m - flank - 1, "right"))):
            g = int(gs[v])
            lo, hi = read_window(r, g - flank, g + flank + 1, before)
            pair = tuple(assess.reverse_complement(a) for a in windows[v]) if r["reverse"] else windows[v]
            if hi <= lo:
                item_drops["no_read_base"] += 1
            elif start[hi] - start[lo] > MAX_FRAMES:
                item_drops["too_many_frames"] += 1
            elif max(len(a) for a in pair) > MAX_LABEL:
                item_drops["allele_too_long"] += 1
            else:
                items.append((frame0 + int(start[lo]), frame0 + int(start[hi])))
                labels.append([np.ascontiguousarray(a, dtype=np.uint8) for a in pair])
                owner.append(v)
        frame0 += r["logits"].shape[0]
    scores = np.concatenate([r["logits"] for r, _ in kept]) if kept else np.zeros((0, 5), np.float32)
    got = scorer(scores, items, labels) if items else {"loglik": [], "status": []}
    for v, ll, st in zip(owner, got["loglik"], got["status"]):
        if st[0] != STATUS_SCORED or st[1] != STATUS_SCORED:
            item_drops["infeasible"] += 1
            continue
        records[v]["reads_scored"] += 1
        records[v]["llr"] += float(ll[1]) - float(ll[0])
        records[v]["logliks"].append((float(ll[0]), float(ll[1])))
    accepted = decide(records, flank, min_reads, min_llr)
    scored_items = sum(rec["reads_scored"] for rec in records)
    report = {"flank": flank, "min_alt": min_alt, "min_frac": min_frac, "min_llr": min_llr, "min_reads": min_reads, "band": band,
              "max_band": max_band,
              "candidates": {"total": len(cands), "scored": len(records), "skipped": skipped},
              "reads": {"total": len(reads), "used": len(kept), "dropped": read_drops},
              "items": {"total": scored_items + sum(item_drops.values()), "scored": scored_items, "dropped": item_drops},
              "frames": int(scores.shape[0]),
              "eligible": sum(1 for rec in records if rec["reads_scored"] >= min_reads and rec["llr"] > min_llr),
              "accepted": {kind: sum(1 for rec in accepted if rec["type"] == kind) for kind in TYPES}}
    report["accepted"]["total"] = len(accepted)
    return {"variants": records, "accepted": accepted, "report": report}


# ----------------------------------------------------------------------------------------------------------------------------
# files and the command
# ----------------------------------------------------------------------------------------------------------------------------
def variant_rows(records, genome):
    """The records as polish_variants.tsv shows them: pos 1-based in the contig, ref / alt as letters ('-' for the side an indel
    lacks; an insertion follows pos)."""
    rows = []
    for r in records:
        c = genome.contig_of(r["g"])
        base = "ACGTN"[int(genome.codes[r["g"]])]
        ref, alt = (base, "ACGT"[r["alt"]]) if r["type"] == "SUB" else (base, "-") if r["type"] == "DEL" else ("-", "ACGT"[r["alt"]])
        rows.append({"contig": genome.names[c], "pos": r["g"] - int(genome.starts[c]) + 1, "type": r["type"], "ref": ref, "alt": alt,
                     "depth": r["depth"], "count": r["count"], "reads_scored": r["reads_scored"], "llr": "%.6f" % r["llr"],
                     "accepted": int(r["accepted"])})
    return rows


def read_strands(path, min_mapq=0):
    """Per SAM line that pileup.read_sam uses, in its order: (name, FLAG 16 set, whole SEQ as codes, leading soft clip).  The same
    lines are skipped as there (unmapped, secondary, supplementary, CIGAR '*', SEQ '*', a MAPQ below min_mapq)."""
    out = []
    with open(path) as f:
        for line in f:
            if line.startswith("@") or not line.strip():
                continue
            col = line.rstrip("\r\n").split("\t")
            flag = int(col[1])
            if flag & 0x904 or col[5] == "*" or col[9] == "*" or pileup.below_mapq(int(col[4]), min_mapq):
                continue
            out.append((col[0], bool(flag & 16), assess.encode(col[9]), pileup.cigar_columns(col[5], col[0])[1]))
    return out


def reads_from_sam(sam, genome, min_mapq=0):
    """(pileup source, reads without logits): the alignments of pileup.read_sam and, per alignment, the read dict of this module
    with `called` turned into signal orientation.  min_mapq: as for pileup.read_sam; the source's low_mapq counts the drops."""
    source = pileup.read_sam(sam, genome, min_mapq)
    strands = read_strands(sam, min_mapq)
    if [s[0] for s in strands] != source["names"]:
        raise ValueError("%s: the strands and the alignments name different reads" % sam)
    reads = []
    for (name, reverse, seq, lead), (pos, _, ops) in zip(strands, source["alignments"]):
        reads.append({"name": name, "pos": pos, "ops": ops, "reverse": reverse, "lead": lead,
                      "called": assess.reverse_complement(seq) if reverse else seq, "logits": None})
    return source, reads


def write_outputs(out_dir, result, genome, meta=None):
    """polished.fasta, polish_variants.tsv and polish_report.json under out_dir; returns the report."""
    os.makedirs(out_dir, exist_ok=True)
    sequences = apply(genome, result["accepted"])
    with open(os.path.join(out_dir, "polished.fasta"), "w") as f:
        f.write("".join(">%s\n%s\n" % (name, sequences[name]) for name in genome.names))
    with open(os.path.join(out_dir, "polish_variants.tsv"), "w") as f:
        f.write("\t".join(VARIANT_COLUMNS) + "\n")
        f.write("".join("\t".join(str(row[key]) for key in VARIANT_COLUMNS) + "\n" for row in variant_rows(result["variants"], genome)))
    report = dict(meta or {})
    report.update(result["report"])
    report["contigs"] = [{"name": name, "length": int(n), "polished_length": len(sequences[name])} for name, n in zip(genome.names, genome.lengths)]
    with open(os.path.join(out_dir, "polish_report.json"), "w") as f:
        json.dump(report, f, indent=1)
    return report


def polish_command(args):
    """The `polish` command: mapped.sam + the reads' signals + the genome + a model -> the three outputs; returns the report."""
    import torch  # noqa: F401  the later stages take their workspaces from torch: its runtime has to be up before the engine loads the library (_lib.py)
    from . import map as map_mod, model as model_mod, signal_io
    from .engine import Engine
    sam = args.input
    if os.path.isdir(sam):
        sam = os.path.join(sam, "mapped.sam")
        if not os.path.exists(sam):
            raise ValueError("%s has no mapped.sam: run `chiron map` with --cigar, which writes it" % args.input)
    genome = map_mod.load_genome(args.genome)
    min_mapq = getattr(args, "min_mapq", 0)
    source, reads = reads_from_sam(sam, genome, min_mapq)
    signals = dict(label.find_signals(args.signal))
    spec, weights, _ = model_mod.load_model(args.model, allow_synthetic=args.synthetic_weights)
    with Engine(spec, weights, max_batch=args.batch_size, segment_len=args.segment_len, device_id=args.device, dtype=args.dtype) as eng:
        for r in reads:
            if r["name"] in signals:
                sig = signal_io.read_signal(signals[r["name"]], normalize=signal_io.SIG_NORM)   # as `call` reads it
                r["logits"] = label.read_frames(eng, sig, args.batch_size)[0]
    piled = pileup.count(source["alignments"], genome, args.min_depth, args.workspace_mb, args.device, want_counts=True)
    result = polish(reads, genome, piled["counts"], piled["depth"], flank=args.flank, min_alt=args.min_alt, min_frac=args.min_frac,
                    min_llr=args.min_llr, min_reads=args.min_reads, band=args.band, max_band=args.max_band, workspace_mb=args.workspace_mb,
                    device_id=args.device)
    meta = {"input": args.input, "sam": sam, "signal": args.signal, "genome": args.genome, "model": args.model, "segment_len": args.segment_len,
            "dtype": args.dtype, "min_depth": args.min_depth, "workspace_mb": args.workspace_mb, "alignments_used": source["used"],
            "alignments_skipped": source["skipped"],
            "vote_variants": len(pileup.variants(piled["call"], piled["depth"], piled["counts"], genome))}
    if min_mapq > 0:
        meta.update({"min_mapq": min_mapq, "low_mapq": source["low_mapq"]})
    return write_outputs(args.output, result, genome, meta)
