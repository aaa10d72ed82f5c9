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
There is no CPU fallback: without the library or a GPU, align_pairs raises.
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
    n = C.c_size_t()
    _lib.check(_lib.load().chiron_align_workspace_size(pairs, max_len, C.byref(n)))
    return int(n.value)


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
    codes = np.ascontiguousarray(np.concatenate(a + b + [np.zeros(1, np.uint8)]))
    lens_a = np.array([len(s) for s in a], dtype=np.int64)
    lens_b = np.array([len(s) for s in b], dtype=np.int64)
    read_off = np.concatenate([[0], np.cumsum(lens_a)]).astype(np.int64)
    ref_off = (read_off[-1] + np.concatenate([[0], np.cumsum(lens_b)])).astype(np.int64)
    max_len = int(max(lens_a.max(), lens_b.max()))
    import torch                                  # before the library loads: its ROCm runtime has to come up first (_lib.py)
    nbytes = workspace_size(pairs, max_len)       # raises CHIRON_ERR_OVERFLOW past MAX_LEN before the GPU is touched
    lib = _lib.load()
    if not torch.cuda.is_available():
        raise RuntimeError("chiron_amd.assess.align_pairs needs a GPU: the alignment has no CPU fallback")
    dev = torch.device("cuda", device_id)
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
    edit = np.zeros(pairs, dtype=np.int32)
    match = np.zeros(pairs, dtype=np.int32)
    band = np.zeros(pairs, dtype=np.int32)
    stream = torch.cuda.current_stream(dev)
    _lib.check(lib.chiron_align_pairs(device_id, codes.ctypes.data, read_off.ctypes.data, ref_off.ctypes.data, pairs, 0,
                                      edit.ctypes.data, match.ctypes.data, band.ctypes.data, ws.data_ptr(),
                                      C.c_void_p(stream.cuda_stream)))
    del ws
    out["read_len"], out["ref_len"], out["edit"], out["match"], out["band"] = lens_a, lens_b, edit, match, band
    x, i, d = counts(lens_a, lens_b, edit.astype(np.int64), match.astype(np.int64))
    out["mismatch"], out["insertion"], out["deletion"] = x, i, d
    total = (match + x + i + d).astype(np.float64)
    out["identity"] = np.where(total > 0, match / np.maximum(total, 1.0), 0.0)
    return out


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


def assess(input_path, reference_path=None, strand="forward", device_id=0):
    """Pair, align, report.  reference_path None: the `call` output tree's own reference/ folder."""
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
    return build_report(names, rows, strands, unpaired,
                        {"input": input_path, "reference": reference_path, "strand_mode": strand})
