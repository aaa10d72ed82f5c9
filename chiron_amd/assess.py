"""Read-level assessment: how close are the reads a model calls to the sequences they should have been?

`chiron call` leaves result/<read>.fastq and, when a fast5 carries one, reference/<read>_ref.fastq (extract.py).  This module
pairs the two, aligns every pair globally with unit costs on the GPU (chiron_align_pairs, csrc/assess.hip) and reports the
numbers basecallers are judged by: identity, mismatch, insertion and deletion rates -- the arithmetic the reference project
leaves to utils/assess.sh (graphmap, samtools, jsa.hts.errorAnalysis).  A reference here is the per-read sequence; with a genome
instead, `chiron map` (map.py) finds each read's place in it and cuts that sequence out, and `assess -g` does both in one go.

Per pair (read of n bases, reference of m) the kernel returns (E, M): the Levenshtein distance and the largest number of
matching columns over the alignments of that cost.  The counts follow without a traceback:
    mismatches X = n + m - 2M - E,  insertions I = n - M - X (read bases the reference lacks),  deletions D = m - M - X,
    identity = M / (M + X + I + D), and the three error rates over the same denominator.
Bases compare case-insensitively, U is T, and any other character (N included) matches nothing, not even itself.
With `--profile` the alignment itself is computed as well (chiron_align_trace, csrc/trace.hip): the canonical optimal alignment's
columns, from which cigar() and error_profile() read which substitutions occur and how homopolymers are called.
There is no CPU fallback: without the library or a GPU, align_pairs and align_ops raise.
"""
import ctypes as C
import os

import numpy as np

from . import _lib

THREADS = _lib.ALIGN_THREADS          # cells of one anti-diagonal a workgroup updates per pass
LDS_SLOTS = _lib.ALIGN_LDS_SLOTS      # widest band (in diagonals) the kernel keeps in LDS
BAND0 = _lib.ALIGN_BAND0              # the first band half-width
MAX_LEN = _lib.ALIGN_MAX_LEN

RESULT_DTYPE = np.dtype([("read_len", np.int32), ("ref_len", np.int32), ("edit", np.int32), ("match", np.int32),
                         ("mismatch", np.int32), ("insertion", np.int32), ("deletion", np.int32), ("identity", np.float64),
                         ("band", np.int32)])

_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _ch in enumerate("ACGT"):
    _CODE[ord(_ch)] = _CODE[ord(_ch.lower())] = _i
_CODE[ord("U")] = _CODE[ord("u")] = 3
_COMPLEMENT = np.array([3, 2, 1, 0, 4], dtype=np.uint8)
SEQ_EXTENSIONS = (".fastq", ".fq", ".fasta", ".fa")


def encode(seq):
    """Bases -> codes: A, C, G, T/U = 0..3 in either case, anything else 4 (matches nothing).  str, bytes or codes."""
    if isinstance(seq, np.ndarray) and seq.dtype == np.uint8:
        return seq
    if isinstance(seq, str):
        seq = seq.encode("latin-1", "replace")
    return _CODE[np.frombuffer(bytes(seq), dtype=np.uint8)]


def reverse_complement(codes):
    return _COMPLEMENT[codes[::-1]]


def read_records(path):
    """[(name, sequence)] of a FASTA or FASTQ file, told apart by the first character; one or many records.  The name is the
    header's first word.  FASTA sequences may span lines; FASTQ records are the four-line form every writer here produces."""
    with open(path) as f:
        lines = [ln.rstrip("\r\n") for ln in f]
    while lines and not lines[0].strip():
        lines.pop(0)
    if not lines:
        return []
    out = []
    if lines[0].startswith(">"):
        name, parts = None, []
        for ln in lines:
            if ln.startswith(">"):
                if name is not None:
                    out.append((name, "".join(parts)))
                name, parts = (ln[1:].split() or [""])[0], []
            else:
                parts.append(ln.strip())
        out.append((name, "".join(parts)))
        return out
    if not lines[0].startswith("@"):
        raise ValueError("%s: neither FASTA ('>') nor FASTQ ('@')" % path)
    i = 0
    while i < len(lines):
        if not lines[i].strip():
            i += 1
            continue
        if not lines[i].startswith("@") or i + 1 >= len(lines):
            raise ValueError("%s: line %d is not a FASTQ header" % (path, i + 1))
        out.append(((lines[i][1:].split() or [""])[0], lines[i + 1].strip()))
        i += 4
    return out


def _stem(path):
    return os.path.splitext(os.path.basename(path))[0]


def _seq_files(folder):
    return sorted(os.path.join(folder, f) for f in os.listdir(folder) if f.lower().endswith(SEQ_EXTENSIONS))


def load_reads(path):
    """{name: sequence} of the called reads: a `call` output tree (its result/), a folder of files, or one file.  A
    single-record file is named after the file (as result/<read>.fastq is); records of a multi-record file keep their names.
    merged.<ext> of a folder repeats its single-read files and is skipped when those are there."""
    if os.path.isdir(path):
        sub = os.path.join(path, "result")
        folder = sub if os.path.isdir(sub) else path
        files = _seq_files(folder)
        singles = [f for f in files if _stem(f) != "merged"]
        files = singles or files
    else:
        files = [path]
    reads = {}
    for f in files:
        recs = read_records(f)
        if len(recs) == 1:
            reads[_stem(f)] = recs[0][1]
        else:
            for name, seq in recs:
                reads[name] = seq
    return reads


def load_references(path):
    """{name: sequence} of the references: a folder of <stem>_ref.fastq / <stem>.fasta / <stem>.fastq, or one file whose
    records are looked up by name (a single-record file also answers to its file name, without `_ref`)."""
    files = _seq_files(path) if os.path.isdir(path) else [path]
    refs = {}
    for f in files:
        recs = read_records(f)
        stem = _stem(f)
        if stem.endswith("_ref"):
            stem = stem[:-4]
        if len(recs) == 1:
            refs[stem] = recs[0][1]
            refs.setdefault(recs[0][0], recs[0][1])
        else:
            for name, seq in recs:
                refs[name] = seq
    return refs


def pair_reads(reads, refs):
    """-> ([(name, read, reference)] in name order, [unpaired names])."""
    paired, unpaired = [], []
    for name in sorted(reads):
        if name in refs:
            paired.append((name, reads[name], refs[name]))
        else:
            unpaired.append(name)
    return paired, unpaired


def counts(n, m, edit, match):
    """(X, I, D) from the lengths and (E, M)."""
    x = n + m - 2 * match - edit
    return x, n - match - x, m - match - x


def rates(match, mismatch, insertion, deletion):
    """identity and the three error rates over M + X + I + D; all 0 for an empty alignment."""
    total = match + mismatch + insertion + deletion
    if total == 0:
        return {"identity": 0.0, "mismatch_rate": 0.0, "insertion_rate": 0.0, "deletion_rate": 0.0}
    return {"identity": match / total, "mismatch_rate": mismatch / total, "insertion_rate": insertion / total,
            "deletion_rate": deletion / total}


def workspace_size(pairs, max_len):
    return _lib.sized("chiron_align_workspace_size", pairs, max_len)


def align_pairs(reads, refs, device_id=0):
    """Align reads[p] against refs[p] (str, bytes or uint8 code arrays) on the GPU, all pairs in one launch.
    -> structured array (RESULT_DTYPE): read_len, ref_len, edit, match, mismatch, insertion, deletion, identity, band."""
    if len(reads) != len(refs):
        raise ValueError("%d reads against %d references" % (len(reads), len(refs)))
    pairs = len(reads)
    a = [encode(s) for s in reads]
    b = [encode(s) for s in refs]
    out = np.zeros(pairs, dtype=RESULT_DTYPE)
    if pairs == 0:
        return out
    codes, lens_a, lens_b, read_off, ref_off = _lib.pack_pairs(a, b)
    max_len = int(max(lens_a.max(), lens_b.max()))
    lib, ws, stream = _lib.device_workspace(lambda: workspace_size(pairs, max_len), device_id, "assess.align_pairs", "alignment")
    edit = np.zeros(pairs, dtype=np.int32)
    match = np.zeros(pairs, dtype=np.int32)
    band = np.zeros(pairs, dtype=np.int32)
    _lib.check(lib.chiron_align_pairs(device_id, codes.ctypes.data, read_off.ctypes.data, ref_off.ctypes.data, pairs, 0,
                                      edit.ctypes.data, match.ctypes.data, band.ctypes.data, ws.data_ptr(), stream))
    del ws
    out["read_len"], out["ref_len"], out["edit"], out["match"], out["band"] = lens_a, lens_b, edit, match, band
    x, i, d = counts(lens_a, lens_b, edit.astype(np.int64), match.astype(np.int64))
    out["mismatch"], out["insertion"], out["deletion"] = x, i, d
    total = (match + x + i + d).astype(np.float64)
    out["identity"] = np.where(total > 0, match / np.maximum(total, 1.0), 0.0)
    return out


OP_LETTERS = "=XID"                   # the column codes of chiron_align_trace: match, mismatch, insertion (read only), deletion (reference only)
HP_MAX_RUN, HP_MAX_CALLED = 10, 20    # the homopolymer table's last row and column collect everything beyond them


def trace_pair_size(n, m, edit):
    """(back-pointer bytes, band in diagonals) of one pair, from the library's host-only helper."""
    nbytes, band = C.c_int64(), C.c_int64()
    _lib.check(_lib.load().chiron_align_trace_pair_size(n, m, edit, C.byref(nbytes), C.byref(band)))
    return int(nbytes.value), int(band.value)


def trace_workspace_size(pairs, backpointer_bytes, max_len, max_band):
    return _lib.sized("chiron_align_trace_workspace_size", pairs, backpointer_bytes, max_len, max_band)


def plan_trace_batches(read_lens, ref_lens, edits, budget_bytes):
    """Consecutive pairs grouped so that each group's workspace stays within the budget (a single pair always forms a group).
    -> [(indices, workspace bytes)]; host-only."""
    batches, cur, cur_bytes, bp, ml, mb = [], [], 0, 0, 0, 0
    for i, (n, m, e) in enumerate(zip(read_lens, ref_lens, edits)):
        pb, band = trace_pair_size(int(n), int(m), int(e))
        nbp, nml, nmb = bp + pb, max(ml, int(n), int(m)), max(mb, band)
        need = trace_workspace_size(len(cur) + 1, nbp, nml, nmb)
        if cur and need > budget_bytes:
            batches.append((cur, cur_bytes))
            cur, nbp, nml, nmb = [], pb, max(int(n), int(m)), band
            need = trace_workspace_size(1, nbp, nml, nmb)
        cur.append(i)
        cur_bytes, bp, ml, mb = need, nbp, nml, nmb
    if cur:
        batches.append((cur, cur_bytes))
    return batches


def trace_pairs(a, b, edit, match, workspace_bytes, device_id=0):
    """One chiron_align_trace call on code arrays a[p], b[p] with their known (edit, match).  -> ([uint8 op arrays], status)."""
    pairs = len(a)
    codes, _, _, read_off, ref_off = _lib.pack_pairs(a, b)
    edit = np.ascontiguousarray(edit, dtype=np.int32)
    match = np.ascontiguousarray(match, dtype=np.int32)
    ops_off = np.concatenate([[0], np.cumsum(edit.astype(np.int64) + match)]).astype(np.int64)
    ops = np.zeros(max(int(ops_off[-1]), 1), dtype=np.uint8)
    status = np.zeros(pairs, dtype=np.int32)
    lib, ws, stream = _lib.device_workspace(workspace_bytes, device_id, "assess.align_ops", "traceback")
    _lib.check(lib.chiron_align_trace(device_id, codes.ctypes.data, read_off.ctypes.data, ref_off.ctypes.data, pairs, edit.ctypes.data,
                                      match.ctypes.data, ops_off.ctypes.data, 0, ops.ctypes.data, status.ctypes.data, ws.data_ptr(), stream))
    del ws
    return [ops[ops_off[p]:ops_off[p + 1]].copy() for p in range(pairs)], status


def align_ops(reads, refs, workspace_mb=4096, device_id=0):
    """The canonical optimal alignment of reads[p] against refs[p] (str, bytes or uint8 code arrays): a list of uint8 arrays, one
    byte per column (0 '=', 1 'X', 2 'I', 3 'D').  align_pairs gives (E, M); the pairs are then traced in batches whose
    workspace stays within workspace_mb (a single pair always forms a batch)."""
    if len(reads) != len(refs):
        raise ValueError("%d reads against %d references" % (len(reads), len(refs)))
    a = [encode(s) for s in reads]
    b = [encode(s) for s in refs]
    if not a:
        return []
    rows = align_pairs(a, b, device_id)
    out = [None] * len(a)
    for batch, nbytes in plan_trace_batches(rows["read_len"], rows["ref_len"], rows["edit"], workspace_mb << 20):
        ops, status = trace_pairs([a[i] for i in batch], [b[i] for i in batch], rows["edit"][batch], rows["match"][batch], nbytes, device_id)
        if status.any():
            raise RuntimeError("chiron_align_trace: pair %d does not have the (E, M) chiron_align_pairs gave it" % batch[int(np.nonzero(status)[0][0])])
        for i, o in zip(batch, ops):
            out[i] = o
    return out


def cigar(ops):
    """Run-length string over =XID of an op array; '*' for an empty alignment."""
    ops = np.asarray(ops, dtype=np.uint8)
    if len(ops) == 0:
        return "*"
    ends = np.concatenate([np.nonzero(ops[1:] != ops[:-1])[0] + 1, [len(ops)]])
    starts = np.concatenate([[0], ends[:-1]])
    return "".join("%d%s" % (e - s, OP_LETTERS[ops[s]]) for s, e in zip(starts, ends))


def error_profile(read, ref, ops):
    """Which errors the canonical alignment `ops` of read against ref holds, as integer tables (nested lists):
      substitution[r][c]   '=' and 'X' columns with reference base r and read base c, both 0..3 (the diagonal counts matches)
      other_mismatch       'X' columns with a code 4 on either side
      insertion[c]         'I' columns by the inserted read code, deletion[c] 'D' columns by the deleted reference code (0..4)
      homopolymer[L][c]    maximal runs of one base (0..3) of length L in the reference whose called length is c: the number of
                           read bases equal to the run's base in the run's span, which is the columns after the column of the
                           previous reference base up to and including the column of the run's last base (the run's own columns
                           and the insertions directly before and inside it).  L above 10 counts in row 10, c above 20 in column
                           20; row 0 stays empty."""
    a, b = encode(read), encode(ref)
    ops = np.asarray(ops, dtype=np.uint8)
    on_read, on_ref = ops != 3, ops != 2
    if int(on_read.sum()) != len(a) or int(on_ref.sum()) != len(b):
        raise ValueError("the alignment covers %d read and %d reference bases, the sequences have %d and %d"
                         % (int(on_read.sum()), int(on_ref.sum()), len(a), len(b)))
    ca = np.full(len(ops), 5, dtype=np.int64)          # the read code of each column, 5 where it has none
    cb = np.full(len(ops), 5, dtype=np.int64)
    ca[on_read] = a
    cb[on_ref] = b
    sub = np.zeros((4, 4), dtype=np.int64)
    diag = ops < 2
    both = diag & (ca < 4) & (cb < 4)
    np.add.at(sub, (cb[both], ca[both]), 1)
    hp = np.zeros((HP_MAX_RUN + 1, HP_MAX_CALLED + 1), dtype=np.int64)
    if len(b):
        col_of = np.nonzero(on_ref)[0]                  # the column of every reference base
        cuts = np.nonzero(b[1:] != b[:-1])[0] + 1
        first = np.concatenate([[0], cuts])
        last = np.concatenate([cuts, [len(b)]]) - 1
        called = np.zeros((4, len(ops) + 1), dtype=np.int64)
        for base in range(4):
            called[base, 1:] = np.cumsum(ca == base)
        base = b[first].astype(np.int64)
        keep = base < 4
        span_end = col_of[last] + 1
        span_start = np.where(first > 0, col_of[np.maximum(first - 1, 0)] + 1, 0)
        c = called[np.minimum(base, 3), span_end] - called[np.minimum(base, 3), span_start]
        np.add.at(hp, (np.minimum(last - first + 1, HP_MAX_RUN)[keep], np.minimum(c, HP_MAX_CALLED)[keep]), 1)
    return {"substitution": sub.tolist(), "other_mismatch": int(((ops == 1) & ~both).sum()),
            "insertion": np.bincount(ca[ops == 2], minlength=5)[:5].tolist(),
            "deletion": np.bincount(cb[ops == 3], minlength=5)[:5].tolist(), "homopolymer": hp.tolist()}


def merge(profiles):
    """The sum of error profiles, table by table; the empty profile for none."""
    out = error_profile("", "", np.zeros(0, np.uint8))
    for prof in profiles:
        for key, val in prof.items():
            out[key] = (np.asarray(out[key], dtype=np.int64) + np.asarray(val, dtype=np.int64)).tolist()
    return out


def add_profile(report, reads, refs, workspace_mb=4096, device_id=0):
    """Trace reads[k] against refs[k] (the pairs of report["reads"], in its order) and add `cigar` per read and the pooled
    `profile` to the report."""
    ops = align_ops(reads, refs, workspace_mb, device_id)
    for rec, o in zip(report["reads"], ops):
        rec["cigar"] = cigar(o)
    report["profile"] = merge(error_profile(a, b, o) for a, b, o in zip(reads, refs, ops))
    return report


def choose_strand(fwd, rev):
    """Per pair the better of the forward and the reverse-complement alignment: smaller E, then larger M; forward wins ties.
    -> (chosen rows, ["forward" | "reverse"])."""
    take_rev = (rev["edit"] < fwd["edit"]) | ((rev["edit"] == fwd["edit"]) & (rev["match"] > fwd["match"]))
    return np.where(take_rev, rev, fwd), ["reverse" if r else "forward" for r in take_rev]


def build_report(names, rows, strands, unpaired, meta=None):
    """The report: per read its lengths, E, M, X, I, D, the four rates and the strand; pooled rates from the summed counts;
    mean and median per-read identity; the unpaired reads, listed and counted."""
    per_read = []
    for name, r, strand in zip(names, rows, strands):
        rec = {"name": name, "read_len": int(r["read_len"]), "ref_len": int(r["ref_len"]), "edit": int(r["edit"]),
               "match": int(r["match"]), "mismatch": int(r["mismatch"]), "insertion": int(r["insertion"]),
               "deletion": int(r["deletion"]), "strand": strand, "band": int(r["band"])}
        rec.update(rates(rec["match"], rec["mismatch"], rec["insertion"], rec["deletion"]))
        per_read.append(rec)
    sums = {k: int(sum(r[k] for r in per_read)) for k in ("match", "mismatch", "insertion", "deletion", "edit", "read_len", "ref_len")}
    pooled = dict(sums)
    pooled.update(rates(sums["match"], sums["mismatch"], sums["insertion"], sums["deletion"]))
    ident = [r["identity"] for r in per_read]
    report = {"paired": len(per_read), "unpaired_count": len(unpaired), "unpaired": list(unpaired), "pooled": pooled,
              "identity_mean": float(np.mean(ident)) if ident else None,
              "identity_median": float(np.median(ident)) if ident else None, "reads": per_read}
    if meta:
        report.update(meta)
    return report


def assess(input_path, reference_path=None, strand="forward", device_id=0, profile=False, workspace_mb=4096):
    """Pair, align, report.  reference_path None: the `call` output tree's own reference/ folder.  profile: also trace every
    pair (on the strand that won) and add the per-read cigar and the pooled error profile."""
    if strand not in ("forward", "both"):
        raise ValueError("strand must be forward or both, not %r" % (strand,))
    if reference_path is None:
        reference_path = os.path.join(input_path, "reference")
        if not os.path.isdir(reference_path):
            raise ValueError("%s has no reference/ folder: give the references with -r" % input_path)
    reads = load_reads(input_path)
    refs = load_references(reference_path)
    paired, unpaired = pair_reads(reads, refs)
    names = [p[0] for p in paired]
    a = [encode(p[1]) for p in paired]
    b = [encode(p[2]) for p in paired]
    if strand == "both" and paired:
        both = align_pairs(a + a, b + [reverse_complement(s) for s in b], device_id)
        rows, strands = choose_strand(both[:len(a)], both[len(a):])
    else:
        rows = align_pairs(a, b, device_id)
        strands = ["forward"] * len(a)
    report = build_report(names, rows, strands, unpaired,
                          {"input": input_path, "reference": reference_path, "strand_mode": strand})
    if profile:
        add_profile(report, a, [reverse_complement(s) if st == "reverse" else s for s, st in zip(b, strands)], workspace_mb, device_id)
    return report
