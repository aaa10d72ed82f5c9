"""Pileup: what do the mapped reads, taken together, say about the genome they were mapped to?

`chiron map --cigar` leaves mapped.sam: every mapped read in genome orientation with its canonical alignment over =XID, gaps
left-aligned so that the same indel lands on the same position in every read.  This module sums those columns per genome position
on the GPU (chiron_pileup, csrc/pileup.hip), calls the majority there, and writes the consensus sequence, the list of places where
the reads disagree with the genome, and a report -- consensus identity is what basecallers are compared on next to read identity.

An alignment is (pos, read, ops): pos in the concatenated coordinates of map.Genome, read the uint8 codes 0..4 in genome
orientation, ops one byte per column as chiron_align_trace codes them (0 '=', 1 'X', 2 'I', 3 'D').  The definition of the counts
(base, del, ins[k], over, clipped, depth) and of the call rule is in include/chiron_amd.h and DESIGN section 16; the counts come back
PLANAR, int32 [PLANES][positions]: planes 0..4 base, 5 del, 6 + 5k + c ins, the last one over.  A call record is 8 bytes: the
consensus code (0..3, 4 N, 5 deleted), the number of inserted bases, their four codes, the status (0 called, 1 low depth), 0.
Counting is the library's; everything after it is plain numpy.  There is no CPU fallback: without the library or a GPU, count raises.
"""
import ctypes as C
import json
import os
import re

import numpy as np

from . import _lib, assess

INS_SLOTS = _lib.PILEUP_INS_SLOTS
PLANES = _lib.PILEUP_PLANES
THREADS = _lib.PILEUP_THREADS
CHUNK = _lib.PILEUP_CHUNK
MAX_COLUMNS, MAX_TILE = _lib.PILEUP_MAX_COLUMNS, _lib.PILEUP_MAX_TILE
PLANE_DEL, PLANE_INS, PLANE_OVER = 5, 6, PLANES - 1
DELETED = 5
SKIP_REASONS = ("unmapped", "secondary", "supplementary", "no_cigar", "no_seq")
_LETTERS = np.frombuffer(b"ACGTN", dtype=np.uint8)
_OP_CODE = {"=": 0, "X": 1, "I": 2, "D": 3, "M": 0}
_CIGAR_ITEM = re.compile(r"(\d+)(.)")


# ----------------------------------------------------------------------------------------------------------------------------
# alignments: from a CIGAR, a SAM file, a map_reads result
# ----------------------------------------------------------------------------------------------------------------------------
def cigar_columns(text, name="?"):
    """A CIGAR -> (ops, leading soft clip, trailing soft clip).  '=', 'X', 'I', 'D' are the columns of assess.cigar; 'M' is a
    diagonal column, coded 0 (the count never looks at the letter of a diagonal column); 'S' stands at an end and clips that many
    read bases there; 'H' is ignored; '*' is the empty alignment.  Any other letter is a ValueError that names the read."""
    if text == "*":
        return np.zeros(0, np.uint8), 0, 0
    items = _CIGAR_ITEM.findall(text)
    if not items or "".join(n + ch for n, ch in items) != text:
        raise ValueError("read %s: %r is not a CIGAR" % (name, text))
    parts, lead, trail = [], 0, 0
    for n, ch in items:
        n = int(n)
        if ch == "H":
            continue
        if ch == "S":
            if parts:
                trail += n
            else:
                lead += n
            continue
        if ch not in _OP_CODE:
            raise ValueError("read %s: CIGAR operation %r is not one of = X I D M S H" % (name, ch))
        if trail:
            raise ValueError("read %s: a soft clip inside the CIGAR %r" % (name, text))
        parts.append(np.full(n, _OP_CODE[ch], np.uint8))
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), lead, trail


def ops_from_cigar(text, name="?"):
    """The columns of a CIGAR: the inverse of assess.cigar (see cigar_columns for M, S and H)."""
    return cigar_columns(text, name)[0]


def _source(alignments, names, skipped=None, soft_clipped=0, low_mapq=0):
    skip = {reason: 0 for reason in SKIP_REASONS}
    skip.update(skipped or {})
    return {"alignments": alignments, "names": names, "used": len(alignments), "skipped": skip, "soft_clipped": int(soft_clipped),
            "low_mapq": int(low_mapq)}


def below_mapq(mapq, min_mapq):
    """Whether a SAM line's MAPQ fails the floor: 255 means not available and always passes."""
    return mapq != 255 and mapq < min_mapq


def read_sam(path, genome, min_mapq=0):
    """The alignments of a SAM file against a map.Genome, from RNAME, the 1-based POS, CIGAR and SEQ.  Lines with FLAG 0x4
    (unmapped), 0x100 (secondary) or 0x800 (supplementary), CIGAR '*' or SEQ '*' are skipped and counted per reason.  An unknown
    contig, or an alignment that runs past its contig's end, is a ValueError.  Of the other lines, those with a MAPQ below
    min_mapq are dropped and counted as low_mapq (255, not available, always passes; with min_mapq 0 nothing is dropped).
    -> dict(alignments=[(pos, read codes, ops)], names, used, skipped={reason: lines}, soft_clipped=read bases under 'S',
    low_mapq)."""
    contig = {name: c for c, name in enumerate(genome.names)}
    alns, names, soft, low = [], [], 0, 0
    skipped = {reason: 0 for reason in SKIP_REASONS}
    with open(path) as f:
        for number, line in enumerate(f, 1):
            if line.startswith("@") or not line.strip():
                continue
            col = line.rstrip("\r\n").split("\t")
            if len(col) < 11:
                raise ValueError("%s: line %d has %d columns, a SAM line has at least 11" % (path, number, len(col)))
            name, flag, rname, pos, cig, seq = col[0], int(col[1]), col[2], int(col[3]), col[5], col[9]
            reason = ("unmapped" if flag & 0x4 else "secondary" if flag & 0x100 else "supplementary" if flag & 0x800 else
                      "no_cigar" if cig == "*" else "no_seq" if seq == "*" else None)
            if reason:
                skipped[reason] += 1
                continue
            if below_mapq(int(col[4]), min_mapq):
                low += 1
                continue
            if rname not in contig:
                raise ValueError("%s: read %s lies on contig %s, which the genome does not have" % (path, name, rname))
            ops, lead, trail = cigar_columns(cig, name)
            codes = assess.encode(seq)
            if int((ops != 3).sum()) + lead + trail != len(codes):
                raise ValueError("%s: the CIGAR of read %s consumes %d bases, its SEQ has %d"
                                 % (path, name, int((ops != 3).sum()) + lead + trail, len(codes)))
            c = contig[rname]
            span = int((ops != 2).sum())
            if pos < 1 or pos - 1 + span > int(genome.lengths[c]):
                raise ValueError("%s: read %s covers %d .. %d of contig %s, which has %d bases"
                                 % (path, name, pos, pos - 1 + span, rname, int(genome.lengths[c])))
            alns.append((int(genome.starts[c]) + pos - 1, codes[lead:len(codes) - trail], ops))
            names.append(name)
            soft += lead + trail
    return _source(alns, names, skipped, soft, low)


def from_map(result, reads, genome):
    """The same alignments from a map_reads result that went through add_cigars, in memory."""
    contig = {name: c for c, name in enumerate(genome.names)}
    alns, names = [], []
    for r in result["reads"]:
        if r["status"] != "mapped" or "cigar" not in r:
            continue
        codes = assess.encode(reads[r["name"]])
        alns.append((int(genome.starts[contig[r["contig"]]]) + r["start"], codes if r["strand"] == "forward" else assess.reverse_complement(codes),
                     ops_from_cigar(r["cigar"], r["name"])))
        names.append(r["name"])
    return _source(alns, names)


# ----------------------------------------------------------------------------------------------------------------------------
# the kernel
# ----------------------------------------------------------------------------------------------------------------------------
def workspace_size(alignments, read_bytes, column_bytes, tile_len):
    return _lib.sized("chiron_pileup_workspace_size", alignments, read_bytes, column_bytes, tile_len)


def pack(alignments):
    """-> (codes, read_off, ops, ops_off, pos) as the library takes them."""
    reads = [np.asarray(a[1], dtype=np.uint8) for a in alignments]
    cols = [np.asarray(a[2], dtype=np.uint8) for a in alignments]
    codes = np.ascontiguousarray(np.concatenate(reads + [np.zeros(1, np.uint8)]))
    ops = np.ascontiguousarray(np.concatenate(cols + [np.zeros(1, np.uint8)]))
    read_off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    ops_off = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    return codes, read_off, ops, ops_off, np.array([a[0] for a in alignments], dtype=np.int64)


def pileup_tile(alignments, g0, g1, ref_codes, min_depth, device_id=0, packed=None):
    """One chiron_pileup call: the tile [g0, g1) of the alignments [(pos, read, ops)].
    -> (counts int32 [PLANES, g1 - g0], depth int32 [g1 - g0], call uint8 [g1 - g0, 8], clipped).  packed: pack(alignments), when
    the caller already has it."""
    codes, read_off, ops, ops_off, pos = packed or pack(alignments)
    n, tile = len(pos), max(int(g1) - int(g0), 0)
    ref = np.ascontiguousarray(ref_codes, dtype=np.uint8)
    if len(ref) != tile:
        raise ValueError("%d reference codes for a tile of %d positions" % (len(ref), tile))
    counts = np.zeros((PLANES, tile), dtype=np.int32)
    depth = np.zeros(tile, dtype=np.int32)
    call = np.zeros((tile, 8), dtype=np.uint8)
    clipped = C.c_int64()
    import torch  # noqa: F401  before the library loads: its ROCm runtime has to come up first (_lib.py)
    nbytes = workspace_size(n, int(read_off[-1]), int(ops_off[-1]), tile)      # raises CHIRON_ERR_OVERFLOW before the GPU is touched
    lib, ws, stream = _lib.load(), None, None
    if tile > 0:                                  # the empty tile is validated on the host and touches no device
        lib, ws, stream = _lib.device_workspace(nbytes, device_id, "pileup.count", "pileup")
    _lib.check(lib.chiron_pileup(device_id, codes.ctypes.data, read_off.ctypes.data, ops.ctypes.data, ops_off.ctypes.data, pos.ctypes.data, n,
                                 int(g0), int(g1), ref.ctypes.data if tile else None, min_depth, 0, counts.ctypes.data, depth.ctypes.data,
                                 call.ctypes.data, C.byref(clipped), ws.data_ptr() if tile else None, stream))
    del ws
    return counts, depth, call, int(clipped.value)


def _spans(alignments):
    """Per alignment: first position, one past its last position (pos + m), read bytes, column bytes."""
    n = len(alignments)
    start, end = np.zeros(n, np.int64), np.zeros(n, np.int64)
    rb, cb = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for p, (pos, read, ops) in enumerate(alignments):
        ops = np.asarray(ops, dtype=np.uint8)
        start[p], end[p], rb[p], cb[p] = pos, pos + int((ops != 2).sum()), len(read), len(ops)
    return start, end, rb, cb


def plan_tiles(alignments, total, budget_bytes, max_tile=MAX_TILE):
    """Cut [0, total) into consecutive tiles so that one call's workspace -- for the tile and the alignments handed to it -- stays
    within the budget; a tile of one position is always allowed.  A tile [g0, g1) is handed every alignment that has a position in
    it, pos < g1 and pos + m > g0: one that straddles an edge goes to both tiles, and an insertion counts with the tile of the
    reference base it follows, which is one of the alignment's positions.  Host-only.
    -> [(g0, g1, indices of its alignments, workspace bytes)]."""
    start, end, rb, cb = _spans(alignments)
    live = end > start

    def need(g0, g1):
        sel = live & (start < g1) & (end > g0)
        return workspace_size(int(sel.sum()), int(rb[sel].sum()), int(cb[sel].sum()), g1 - g0), sel

    tiles, g0 = [], 0
    while g0 < total:
        lo, hi = g0 + 1, min(total, g0 + max_tile)            # the size is monotone in g1: bisect for the largest tile that fits
        nbytes, sel = need(g0, hi)
        if nbytes > budget_bytes:
            while lo < hi:
                mid = (lo + hi + 1) // 2
                if need(g0, mid)[0] <= budget_bytes:
                    lo = mid
                else:
                    hi = mid - 1
            nbytes, sel = need(g0, lo)
            hi = lo
        tiles.append((g0, hi, np.nonzero(sel)[0].tolist(), nbytes))
        g0 = hi
    return tiles


def count(alignments, genome, min_depth=3, workspace_mb=4096, device_id=0, counter=None, want_counts=False):
    """Count and call the alignments [(pos, read, ops)] over the whole concatenated genome, tile by tile (plan_tiles).
    workspace_mb may be a fraction.  counter(alignments, g0, g1, ref_codes, min_depth) -> (counts, depth, call, clipped) replaces
    the library call (the tests' reference).  -> dict(depth int32 [G], call uint8 [G, 8], clipped, over_total[, counts int32 [PLANES, G]]); clipped is the 'I'
    columns before an alignment's first or after its last reference base, over all alignments."""
    if counter is None:
        import torch  # noqa: F401  before plan_tiles loads the library: torch's ROCm runtime has to come up first (_lib.py)

        def counter(alns, g0, g1, ref, md):
            return pileup_tile(alns, g0, g1, ref, md, device_id)
    alignments = list(alignments)
    total = len(genome.codes)
    depth = np.zeros(total, dtype=np.int32)
    call = np.zeros((total, 8), dtype=np.uint8)
    counts = np.zeros((PLANES, total), dtype=np.int32) if want_counts else None
    over_total = 0
    for g0, g1, idx, _ in plan_tiles(alignments, total, int(workspace_mb * (1 << 20))):
        c, d, k, _ = counter([alignments[i] for i in idx], g0, g1, genome.codes[g0:g1], min_depth)
        depth[g0:g1], call[g0:g1] = d, k
        over_total += int(np.asarray(c[PLANE_OVER], dtype=np.int64).sum())
        if want_counts:
            counts[:, g0:g1] = c
    # clipping does not depend on the tile: the empty tile validates every alignment once and launches nothing
    clipped = counter(alignments, 0, 0, genome.codes[0:0], min_depth)[3]
    out = {"depth": depth, "call": call, "clipped": int(clipped), "over_total": over_total}
    if want_counts:
        out["counts"] = counts
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# after the counting: consensus, variants, the command
# ----------------------------------------------------------------------------------------------------------------------------
def consensus(call, genome):
    """{contig: sequence}: per position of the contig the emitted base (none where the call is a deletion), then its inserted
    bases.  The separator positions between contigs are skipped."""
    out = {}
    for c, name in enumerate(genome.names):
        g0 = int(genome.starts[c])
        rec = call[g0:g0 + int(genome.lengths[c])]
        chars = np.zeros((len(rec), 1 + INS_SLOTS), dtype=np.uint8)
        keep = rec[:, 0] != DELETED
        chars[keep, 0] = _LETTERS[rec[keep, 0]]
        for k in range(INS_SLOTS):
            on = rec[:, 1] > k
            chars[on, 1 + k] = _LETTERS[rec[on, 2 + k]]
        flat = chars.reshape(-1)
        out[name] = flat[flat != 0].tobytes().decode("ascii")
    return out


def variants(call, depth, counts, genome):
    """One record per position where the call differs from the genome, in position order: dict(contig, pos (1-based), type (SUB |
    DEL | INS), ref, alt, depth, count).  A SUB or DEL comes before the INS of the same position; an INS is reported at its anchor
    with ref '-' and alt the inserted string; a DEL has alt '-'.  count is the winning count (for INS the first slot's total over
    all five codes), -1 when counts is None."""
    out = []
    for c, name in enumerate(genome.names):
        g0 = int(genome.starts[c])
        L = int(genome.lengths[c])
        rec, ref = call[g0:g0 + L], genome.codes[g0:g0 + L]
        for t in np.nonzero((rec[:, 0] != ref) | (rec[:, 1] > 0))[0]:
            g, code, r = g0 + int(t), int(rec[t, 0]), int(ref[t])
            base = {"contig": name, "pos": int(t) + 1, "depth": int(depth[g])}
            if code == DELETED:
                out.append(dict(base, type="DEL", ref="ACGTN"[r], alt="-", count=-1 if counts is None else int(counts[PLANE_DEL, g])))
            elif code != r:
                out.append(dict(base, type="SUB", ref="ACGTN"[r], alt="ACGTN"[code], count=-1 if counts is None else int(counts[code, g])))
            if rec[t, 1]:
                first = -1 if counts is None else int(counts[PLANE_INS:PLANE_INS + 5, g].astype(np.int64).sum())
                out.append(dict(base, type="INS", ref="-", alt="".join("ACGTN"[int(v)] for v in rec[t, 2:2 + int(rec[t, 1])]), count=first))
    return out


VARIANT_COLUMNS = ("contig", "pos", "type", "ref", "alt", "depth", "count")


def variant_lines(records):
    return ["\t".join(VARIANT_COLUMNS)] + ["\t".join(str(r[key]) for key in VARIANT_COLUMNS) for r in records]


def build_report(result, records, sequences, genome, source, meta=None):
    """The report of the `pileup` command: per contig and in total."""
    contigs, min_depth = [], (meta or {}).get("min_depth", 0)
    for c, name in enumerate(genome.names):
        g0 = int(genome.starts[c])
        L = int(genome.lengths[c])
        d = result["depth"][g0:g0 + L]
        mine = [r for r in records if r["contig"] == name]
        contigs.append({"name": name, "length": L, "consensus_length": len(sequences[name]),
                        "mean_depth": float(d.astype(np.float64).mean()) if L else 0.0,
                        "low_depth": int((result["call"][g0:g0 + L, 6] == 1).sum()),
                        "substitutions": sum(1 for r in mine if r["type"] == "SUB"),
                        "deletions": sum(1 for r in mine if r["type"] == "DEL"),
                        "insertions": sum(1 for r in mine if r["type"] == "INS"),
                        "inserted_bases": sum(len(r["alt"]) for r in mine if r["type"] == "INS")})
    totals = {key: sum(c[key] for c in contigs) for key in ("length", "consensus_length", "low_depth", "substitutions", "deletions", "insertions",
                                                          "inserted_bases")}
    totals["mean_depth"] = (sum(c["mean_depth"] * c["length"] for c in contigs) / totals["length"]) if totals["length"] else 0.0
    report = dict(meta or {})
    report.update({"contigs": contigs, "totals": totals, "clipped": result["clipped"] + source["soft_clipped"], "over_total": result["over_total"],
                   "alignments_used": source["used"], "alignments_skipped": source["skipped"], "min_depth": min_depth})
    return report


def write_outputs(out_dir, result, genome, source, meta=None):
    """consensus.fasta (one record per contig, under the contig's name), variants.tsv (a header line, then one line per record)
    and pileup_report.json under out_dir; returns the report."""
    os.makedirs(out_dir, exist_ok=True)
    sequences = consensus(result["call"], genome)
    records = variants(result["call"], result["depth"], result.get("counts"), genome)
    with open(os.path.join(out_dir, "consensus.fasta"), "w") as f:
        f.write("".join(">%s\n%s\n" % (name, sequences[name]) for name in genome.names))
    with open(os.path.join(out_dir, "variants.tsv"), "w") as f:
        f.write("".join(ln + "\n" for ln in variant_lines(records)))
    report = build_report(result, records, sequences, genome, source, meta)
    with open(os.path.join(out_dir, "pileup_report.json"), "w") as f:
        json.dump(report, f, indent=1)
    return report


def pileup_command(input_path, genome_path, out_dir, min_depth=3, workspace_mb=4096, device_id=0, min_mapq=0):
    """The `pileup` command: a `map --cigar` output directory (its mapped.sam) or a SAM file + the genome -> the three outputs.
    min_mapq > 0: alignments below it are dropped (read_sam) and the report gains min_mapq and low_mapq, their count."""
    from . import map as map_mod
    sam = input_path
    if os.path.isdir(input_path):
        sam = os.path.join(input_path, "mapped.sam")
        if not os.path.exists(sam):
            raise ValueError("%s has no mapped.sam: run `chiron map` with --cigar, which writes it" % input_path)
    genome = map_mod.load_genome(genome_path)
    source = read_sam(sam, genome, min_mapq)
    result = count(source["alignments"], genome, min_depth, workspace_mb, device_id, want_counts=True)
    meta = {"input": input_path, "sam": sam, "genome": genome_path, "min_depth": min_depth, "workspace_mb": workspace_mb, "ins_slots": INS_SLOTS}
    if min_mapq > 0:
        meta.update({"min_mapq": min_mapq, "low_mapq": source["low_mapq"]})
    return write_outputs(out_dir, result, genome, source, meta)
