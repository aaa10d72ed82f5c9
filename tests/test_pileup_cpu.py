"""CPU: the pileup's definition and host side.  tests/pileup_ref.py walks every alignment column by column; here
it is checked against an independent formulation, the call rule clause by clause, the CIGAR and SAM readers, the tile plan, the
library's argument validation (no device is looked for), and the whole pipeline end to end on the references alone."""
import ctypes as C
import os

import numpy as np
import pytest

from chiron_amd import _lib, assess, map as cmap, pileup

import map_ref
import pileup_cases as cases
import pileup_ref

S = pileup_ref.S


def test_constants_agree():
    assert (pileup.INS_SLOTS, pileup.PLANES) == (pileup_ref.S, pileup_ref.PLANES) == (4, 27)
    assert (pileup.PLANE_DEL, pileup.PLANE_INS, pileup.PLANE_OVER) == (pileup_ref.DEL, pileup_ref.INS, pileup_ref.OVER)
    assert pileup.THREADS == 256 and pileup.CHUNK % pileup.THREADS == 0


def test_reference_counts_equal_the_padded_row_formulation():
    """200 random alignment sets, indel-rich, with N, over tiles that cut alignments at both ends."""
    rng = np.random.default_rng(160)
    seen_over = seen_clip = 0
    for k in range(200):
        tile = int(rng.integers(1, 60))
        alns = cases.random_set(rng, int(rng.integers(0, 12)), tile, max_columns=40, p_ins=(0.1, 0.35, 0.6)[k % 3], p_del=0.15, n_rate=0.05)
        g0 = int(rng.integers(-5, 10))
        g1 = g0 + tile
        a, ca = pileup_ref.count_columns(alns, g0, g1)
        b, cb = pileup_ref.padded_counts(alns, g0, g1)
        assert np.array_equal(a, b) and ca == cb, k
        seen_over += int(a[pileup_ref.OVER].sum())
        seen_clip += ca
    assert seen_over > 20 and seen_clip > 100


def _call(base, dele=0, ins=None, r=0, min_depth=3):
    ins = ins or [[0] * 5 for _ in range(S)]
    return pileup_ref.call_position(base, dele, ins, r, min_depth)


def test_call_rule_clause_by_clause():
    # depth below, at and above min_depth
    assert _call([0, 2, 0, 0, 0], r=0) == (2, [0, 0, 0, 0, 0, 0, 1, 0], "low")
    assert _call([0, 3, 0, 0, 0], r=0) == (3, [1, 0, 0, 0, 0, 0, 0, 0], "base")
    assert _call([0, 4, 0, 0, 0], r=0)[1][0] == 1
    assert _call([0, 1, 1, 0, 0], dele=0, r=0, min_depth=2)[0] == 2
    # low depth emits no insertion, whatever the slots hold
    assert _call([0, 2, 0, 0, 0], ins=[[2, 0, 0, 0, 0]] + [[0] * 5] * 3, r=3)[1] == [3, 0, 0, 0, 0, 0, 1, 0]
    # a tie between two non-reference bases goes to the smaller code; one that the reference base is in goes to it
    assert _call([0, 0, 3, 3, 0], r=0)[1:] == ([2, 0, 0, 0, 0, 0, 0, 0], "tie_code")
    assert _call([0, 0, 3, 3, 0], r=3)[1:] == ([3, 0, 0, 0, 0, 0, 0, 0], "tie_ref")
    assert _call([2, 2, 2, 2, 0], r=2)[1][0] == 2 and _call([2, 2, 2, 2, 0], r=4)[1][0] == 0
    # deletion equal to a base: the base wins; deletion greater: nothing is emitted
    assert _call([0, 3, 0, 0, 0], dele=3, r=0)[1:] == ([1, 0, 0, 0, 0, 0, 0, 0], "tie_deletion")
    assert _call([0, 3, 0, 0, 0], dele=4, r=1)[1:] == ([5, 0, 0, 0, 0, 0, 0, 0], "deletion")
    # only N observed: the reference base; the reference itself N: the majority, or N when nothing was seen
    assert _call([0, 0, 0, 0, 5], r=2)[1:] == ([2, 0, 0, 0, 0, 0, 0, 0], "only_n")
    assert _call([0, 0, 4, 1, 0], r=4)[1][0] == 2 and _call([0, 0, 0, 0, 3], r=4)[1][0] == 4
    assert _call([0] * 5, r=1, min_depth=0) == (0, [1, 0, 0, 0, 0, 0, 0, 0], "only_n")
    # an insertion slot needs more than half the depth; the chain stops at the first slot that fails although a later one passes
    ins = [[0, 3, 0, 0, 0], [0, 0, 1, 0, 1], [0, 0, 0, 4, 0], [0] * 5]
    assert _call([4, 0, 0, 0, 0], ins=ins, r=0)[1] == [0, 1, 1, 0, 0, 0, 0, 0]
    ins[1] = [0, 0, 2, 0, 1]
    assert _call([4, 0, 0, 0, 0], ins=ins, r=0)[1] == [0, 3, 1, 2, 3, 0, 0, 0]
    assert _call([4, 0, 0, 0, 0], ins=[[0, 2, 0, 0, 0]] + [[0] * 5] * 3, r=0)[1][1] == 0        # exactly half is not enough
    # ties inside a slot go to the smaller code; a slot of only N emits N; an insertion follows a deleted position too
    assert _call([4, 0, 0, 0, 0], ins=[[0, 0, 2, 2, 0]] + [[0] * 5] * 3, r=0)[1] == [0, 1, 2, 0, 0, 0, 0, 0]
    assert _call([4, 0, 0, 0, 0], ins=[[0, 0, 0, 0, 3]] + [[0] * 5] * 3, r=0)[1] == [0, 1, 4, 0, 0, 0, 0, 0]
    assert _call([1, 0, 0, 0, 0], dele=3, ins=[[0, 0, 0, 3, 0]] + [[0] * 5] * 3, r=0)[1] == [5, 1, 3, 0, 0, 0, 0, 0]


def test_ops_from_cigar():
    rng = np.random.default_rng(161)
    for _ in range(50):
        ops = rng.integers(0, 4, int(rng.integers(0, 80))).astype(np.uint8)
        assert np.array_equal(pileup.ops_from_cigar(assess.cigar(ops)), ops)
    assert pileup.ops_from_cigar("*").tolist() == []
    assert pileup.ops_from_cigar("2M1I1D1X").tolist() == [0, 0, 2, 3, 1]
    ops, lead, trail = pileup.cigar_columns("5H3S2=1I2M4S7H")
    assert (ops.tolist(), lead, trail) == ([0, 0, 2, 0, 0], 3, 4)
    ops, lead, trail = pileup.cigar_columns("2=6S")
    assert (ops.tolist(), lead, trail) == ([0, 0], 0, 6)
    for bad in ("3N2=", "2=1P", "2=3S1=", "=", "2", "2=x"):
        with pytest.raises(ValueError) as ei:
            pileup.ops_from_cigar(bad, "readQ")
        assert "readQ" in str(ei.value), bad


def _mapped_case():
    rng = np.random.default_rng(162)
    contigs = [("ctgA", cases.assess_ref.random_seq(900, rng)), ("ctgB", cases.assess_ref.random_seq(700, rng))]
    genome = cmap.Genome(contigs)
    reads = {"fwd": cases.assess_ref.mutate(contigs[0][1][100:400], 0.1, rng),
             "rev": map_ref.revcomp(cases.assess_ref.mutate(contigs[1][1][200:450], 0.1, rng))}
    seeds = {"fwd": {"strand": "forward", "delta": 100, "contig": 0}, "rev": {"strand": "reverse", "delta": 915 + 200, "contig": 1}}
    res = cmap.map_reads(reads, genome, seeds=seeds, aligner=lambda rs, ws, b: map_ref.infix_rows(rs, ws, b, cmap.INFIX_DTYPE))
    cmap.add_cigars(res, reads, genome, tracer=cases.reference_tracer)
    return contigs, genome, reads, res


def test_read_sam_and_from_map(tmp_path):
    contigs, genome, reads, res = _mapped_case()
    lines = cmap.sam_lines(res, reads, genome)
    assert len(lines) == 5
    fwd = lines[3].split("\t")
    extra = ["\t".join(["u1", "4", "*", "0", "0", "*", "*", "0", "0", "ACGT", "*"]),
             "\t".join(fwd[:1] + ["256"] + fwd[2:]), "\t".join(fwd[:1] + ["2048"] + fwd[2:]), "\t".join(fwd[:1] + ["2064"] + fwd[2:]),
             "\t".join(fwd[:5] + ["*"] + fwd[6:]), "\t".join(fwd[:9] + ["*"] + fwd[10:]), ""]
    path = tmp_path / "mapped.sam"
    path.write_text("".join(ln + "\n" for ln in lines + extra))
    src = pileup.read_sam(str(path), genome)
    assert src["used"] == 2 and src["names"] == ["fwd", "rev"] and src["soft_clipped"] == 0
    assert src["skipped"] == {"unmapped": 1, "secondary": 1, "supplementary": 2, "no_cigar": 1, "no_seq": 1}
    mem = pileup.from_map(res, reads, genome)
    by = {r["name"]: r for r in res["reads"]}
    for (pos, read, ops), (pos2, read2, ops2), name in zip(src["alignments"], mem["alignments"], src["names"]):
        assert pos == pos2 and np.array_equal(read, read2) and np.array_equal(ops, ops2)
        c = genome.names.index(by[name]["contig"])
        assert pos == int(genome.starts[c]) + by[name]["start"] and assess.cigar(ops) == by[name]["cigar"]
        assert int((ops != 3).sum()) == len(read) and int((ops != 2).sum()) == by[name]["end"] - by[name]["start"]
    assert np.array_equal(src["alignments"][1][1], assess.reverse_complement(assess.encode(reads["rev"])))
    # soft clips shorten the read and are counted; M is a diagonal column
    soft = fwd[:5] + ["2S" + "%dM" % (len(fwd[9]) - 5) + "3S"] + fwd[6:]
    path.write_text("\t".join(soft) + "\n")
    src = pileup.read_sam(str(path), genome)
    pos, read, ops = src["alignments"][0]
    assert src["soft_clipped"] == 5 and len(read) == len(fwd[9]) - 5 == len(ops) and not ops.any()
    assert np.array_equal(read, assess.encode(fwd[9])[2:-3])
    # an unknown contig, a read past its contig's end, a CIGAR that disagrees with SEQ, a CIGAR letter that is not taken
    for cols, word in ((fwd[:2] + ["ctgZ"] + fwd[3:], "ctgZ"), (fwd[:3] + ["800"] + fwd[4:], "covers"),
                       (fwd[:5] + ["10="] + fwd[6:], "consumes"), (fwd[:5] + ["10N"] + fwd[6:], "fwd")):
        path.write_text("\t".join(cols) + "\n")
        with pytest.raises(ValueError) as ei:
            pileup.read_sam(str(path), genome)
        assert word in str(ei.value)


def test_tile_plan(built):
    rng = np.random.default_rng(163)
    total = 5000
    alns = cases.random_set(rng, 400, total, max_columns=300)
    # an alignment whose insertion is anchored at position 999 and that goes on to 1000; one that ends at 999 with a trailing 'I'
    ins_at_edge = (995, np.zeros(7, np.uint8), np.array([0, 0, 0, 0, 0, 2, 0], np.uint8))
    ends_at_edge = (995, np.zeros(6, np.uint8), np.array([0, 0, 0, 0, 0, 2], np.uint8))
    empty = (500, np.zeros(3, np.uint8), np.array([2, 2, 2], np.uint8))
    alns += [ins_at_edge, ends_at_edge, empty]
    one = pileup.plan_tiles(alns, total, 4096 << 20)
    assert len(one) == 1 and one[0][:2] == (0, total) and one[0][3] <= 4096 << 20
    assert len(alns) - 1 not in one[0][2]                               # no reference base: it has no position in any tile
    forced = pileup.plan_tiles(alns, total, 4096 << 20, max_tile=1000)
    assert [t[:2] for t in forced] == [(k, k + 1000) for k in range(0, total, 1000)]
    a, b, c = len(alns) - 3, len(alns) - 2, len(alns) - 1
    assert a in forced[0][2] and a in forced[1][2] and b in forced[0][2] and b not in forced[1][2]
    assert all(c not in t[2] for t in forced)
    budget = 100 << 10
    tiles = pileup.plan_tiles(alns, total, budget)
    assert len(tiles) > 3 and tiles[0][0] == 0 and tiles[-1][1] == total
    assert all(t[1] == u[0] for t, u in zip(tiles, tiles[1:])) and all(t[0] < t[1] for t in tiles)
    start, end, rb, cb = pileup._spans(alns)
    for g0, g1, idx, nbytes in tiles:
        assert nbytes <= budget
        want = [p for p in range(len(alns)) if end[p] > start[p] and start[p] < g1 and end[p] > g0]
        assert idx == want
        ix = np.array(idx, dtype=np.int64)
        assert nbytes == pileup.workspace_size(len(idx), int(rb[ix].sum()), int(cb[ix].sum()), g1 - g0)
        if g1 < total:                                                  # the tile is maximal: one more position would not fit
            more = np.array([p for p in range(len(alns)) if end[p] > start[p] and start[p] < g1 + 1 and end[p] > g0], dtype=np.int64)
            assert pileup.workspace_size(len(more), int(rb[more].sum()), int(cb[more].sum()), g1 + 1 - g0) > budget
    tiny = pileup.plan_tiles(alns[:20], 7, 1)                           # a tile of one position is always allowed
    assert [t[:2] for t in tiny] == [(k, k + 1) for k in range(7)]
    # count() hands every tile its alignments and concatenates: identical to one tile, through the reference counter
    total = 300
    alns = cases.random_set(rng, 60, total, max_columns=50, p_ins=0.4) + [(295, ins_at_edge[1], ins_at_edge[2]), (20, empty[1], empty[2])]
    genome = cmap.Genome([("c", "".join("ACGT"[v] for v in rng.integers(0, 4, total)))])
    whole = pileup.count(alns, genome, counter=pileup_ref.counter, want_counts=True)
    split = pileup.count(alns, genome, workspace_mb=0, counter=pileup_ref.counter, want_counts=True)      # budget 0: one position a tile
    for key in ("depth", "call", "counts"):
        assert np.array_equal(whole[key], split[key]), key
    planes, clipped = pileup_ref.count_columns(alns, 0, total)
    assert np.array_equal(whole["counts"], planes) and whole["clipped"] == split["clipped"] == clipped >= 4
    assert whole["over_total"] == split["over_total"] == int(planes[pileup_ref.OVER].sum())


def _raw(lib, alns, g0, g1, min_depth=3, ref=None, flags=0, n=None, read_off=None, ops_off=None):
    codes, r_off, ops, o_off, pos = pileup.pack(alns)
    r_off = r_off if read_off is None else np.asarray(read_off, np.int64)
    o_off = o_off if ops_off is None else np.asarray(ops_off, np.int64)
    tile = max(g1 - g0, 0)
    ref = np.zeros(min(tile, 1 << 16), np.uint8) if ref is None else ref
    counts = np.zeros((pileup.PLANES, min(tile, 1 << 16)), np.int32)
    depth = np.zeros(min(tile, 1 << 16), np.int32)
    call = np.zeros((min(tile, 1 << 16), 8), np.uint8)
    clipped = C.c_int64(-1)
    st = lib.chiron_pileup(0, codes.ctypes.data, r_off.ctypes.data, ops.ctypes.data, o_off.ctypes.data, pos.ctypes.data,
                           len(alns) if n is None else n, g0, g1, ref.ctypes.data, min_depth, flags, counts.ctypes.data, depth.ctypes.data,
                           call.ctypes.data, C.byref(clipped), None, None)
    return st, clipped.value


def test_abi_sizes_and_argument_errors(built):
    """Every refusal comes before a device is looked for: this test runs without one (with one, the accepted calls would go on to
    ask for a workspace, which is refused as CHIRON_ERR_INVALID too, after the host checks)."""
    lib = _lib.load()
    n = C.c_size_t()
    size = lambda *a: (lib.chiron_pileup_workspace_size(*a, C.byref(n)), n.value)
    assert size(0, 0, 0, 0) == (_lib.OK, 0)
    base = (1000, 300000, 330000, 5000)
    st, ref_bytes = size(*base)
    assert st == _lib.OK and ref_bytes >= 1000 * 32 + 300000 + 330000 + 5000 * (1 + 4 * pileup.PLANES + 4 + 8)
    for k in range(4):                                                  # monotone in each argument
        prev = 0
        for v in (0, 1, 255, 256, 257, 4096, 100000, 1 << 24):
            args = list(base)
            args[k] = v
            st, nbytes = size(*args)
            assert st == _lib.OK and nbytes >= prev
            prev = nbytes
        args = list(base)
        args[k] = -1
        assert size(*args)[0] == _lib.ERR_INVALID
    assert size((1 << 24) + 1, 0, 0, 1)[0] == _lib.ERR_OVERFLOW
    assert size(1, 0, 0, pileup.MAX_TILE + 1)[0] == _lib.ERR_OVERFLOW and size(1, 0, 0, pileup.MAX_TILE)[0] == _lib.OK
    assert size(1, (1 << 48) + 1, 0, 1)[0] == _lib.ERR_OVERFLOW and size(1, 0, (1 << 48) + 1, 1)[0] == _lib.ERR_OVERFLOW
    with pytest.raises(_lib.ChironError):
        pileup.workspace_size(-1, 0, 0, 0)

    good = [(3, np.array([0, 1, 2, 3, 4], np.uint8), np.array([2, 0, 0, 3, 0, 2], np.uint8)), (0, np.zeros(0, np.uint8), np.zeros(0, np.uint8))]
    # the empty tile validates and counts the clipping without a device
    assert _raw(lib, good, 5, 5) == (_lib.OK, 2)
    assert _raw(lib, [], 0, 0) == (_lib.OK, 0)
    assert _raw(lib, [(0, np.array([1, 4], np.uint8), np.array([2, 2], np.uint8))], 0, 0) == (_lib.OK, 2)
    invalid = [
        dict(alns=good, g0=6, g1=5), dict(alns=good, g0=-1, g1=5), dict(alns=good, g0=0, g1=5, min_depth=-1), dict(alns=good, g0=0, g1=5, flags=1),
        dict(alns=good, g0=0, g1=5, n=-1),
        dict(alns=good, g0=0, g1=5, read_off=[-1, 4, 4]), dict(alns=good, g0=0, g1=5, read_off=[0, 4, 3]),
        dict(alns=good, g0=0, g1=5, ops_off=[-2, 6, 6]), dict(alns=good, g0=0, g1=5, ops_off=[0, 6, 5]),
        dict(alns=[(0, np.array([0, 5], np.uint8), np.array([0, 0], np.uint8))], g0=0, g1=5),              # a code above 4
        dict(alns=[(0, np.array([0, 1], np.uint8), np.array([0, 4], np.uint8))], g0=0, g1=5),              # an op above 3
        dict(alns=[(0, np.array([0, 1], np.uint8), np.array([0, 0, 2], np.uint8))], g0=0, g1=5),           # columns consume 3, the read has 2
        dict(alns=[(0, np.array([0, 1], np.uint8), np.array([0, 3, 3], np.uint8))], g0=0, g1=5),           # columns consume 1
        dict(alns=good, g0=0, g1=3, ref=np.array([0, 7, 0], np.uint8)),                                    # a reference code above 4
    ]
    for kw in invalid:
        assert _raw(lib, **kw)[0] == _lib.ERR_INVALID, kw
        assert lib.chiron_last_error()
    big = pileup.MAX_COLUMNS + 1
    overflow = [dict(alns=good, g0=0, g1=pileup.MAX_TILE + 1), dict(alns=good, g0=0, g1=5, n=(1 << 24) + 1),
                dict(alns=good[:1], g0=0, g1=5, ops_off=[0, big]), dict(alns=good[:1], g0=0, g1=5, read_off=[0, big])]
    for kw in overflow:
        assert _raw(lib, **kw)[0] == _lib.ERR_OVERFLOW, kw
    import torch
    if not torch.cuda.is_available():
        assert _raw(lib, good, 0, 5)[0] == _lib.ERR_INVALID                # accepted by the host checks; the null workspace is next
        with pytest.raises(RuntimeError) as ei:
            pileup.count(good, cmap.Genome([("c", "ACGTACGT")]))
        assert "no CPU fallback" in str(ei.value)


@pytest.fixture(scope="module")
def end_to_end():
    truth, given, reads, seeds = cases.end_to_end_case()
    genome = cmap.Genome(given)
    res = cmap.map_reads(reads, genome, seeds=seeds, aligner=lambda rs, ws, b: map_ref.infix_rows(rs, ws, b, cmap.INFIX_DTYPE))
    cmap.add_cigars(res, reads, genome, tracer=cases.reference_tracer)
    return truth, given, reads, genome, res


def test_end_to_end_on_the_references(end_to_end, tmp_path):
    """map_reads(aligner=map_ref), add_cigars(tracer=trace_ref), count(counter=pileup_ref): the consensus is closer to the truth
    than the genome that was handed in.  Measured on the CPU with the reference alone, seed 2: the given genome has 42 edits against
    the truth (summed over the two contigs), the consensus 13."""
    truth, given, reads, genome, res = end_to_end
    assert res["totals"]["mapped"] == 60
    source = pileup.from_map(res, reads, genome)
    result = pileup.count(source["alignments"], genome, counter=pileup_ref.counter, want_counts=True)
    want = cases.reference_consensus(source, genome)
    for key in ("counts", "depth", "call"):
        assert np.array_equal(result[key], want[key]), key
    assert result["clipped"] == want["clipped"]
    seqs = pileup.consensus(result["call"], genome)
    recs = pileup.variants(result["call"], result["depth"], result["counts"], genome)
    assert seqs == want["consensus"] and recs == want["variants"]
    blind = pileup.variants(result["call"], result["depth"], None, genome)
    assert [dict(r, count=-1) for r in recs] == blind
    before, after = cases.edits_against(truth, dict(given)), cases.edits_against(truth, seqs)
    print("edits against the truth: given genome %d, consensus %d" % (before, after))
    assert after < before
    # the SAM route gives the same alignments, and the writers what the report says
    (tmp_path / "m").mkdir()
    cmap.write_outputs(str(tmp_path / "m"), res, genome, reads=reads)
    sam = pileup.read_sam(str(tmp_path / "m" / "mapped.sam"), genome)
    assert sam["used"] == 60 and all(a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
                                     for a, b in zip(sam["alignments"], source["alignments"]))
    report = pileup.write_outputs(str(tmp_path / "p"), result, genome, sam, {"min_depth": 3})
    assert dict(assess.read_records(str(tmp_path / "p" / "consensus.fasta"))) == seqs
    lines = (tmp_path / "p" / "variants.tsv").read_text().splitlines()
    assert lines[0].split("\t") == list(pileup.VARIANT_COLUMNS) and len(lines) == 1 + len(recs)
    assert [ln.split("\t") for ln in lines[1:]] == [[str(r[k]) for k in pileup.VARIANT_COLUMNS] for r in recs]
    t = report["totals"]
    assert t["substitutions"] + t["deletions"] + t["insertions"] == len(recs) and t["length"] == sum(len(s) for _, s in given)
    assert t["consensus_length"] == sum(len(s) for s in seqs.values()) == t["length"] - t["deletions"] + t["inserted_bases"]
    assert report["alignments_used"] == 60 and report["clipped"] == want["clipped"] and report["over_total"] == result["over_total"]
    assert [c["name"] for c in report["contigs"]] == ["ctgA", "ctgB"]
    assert report["contigs"][0]["low_depth"] == int((want["call"][:len(given[0][1]), 6] == 1).sum())


def test_command_names_the_missing_sam(tmp_path):
    (tmp_path / "out").mkdir()
    (tmp_path / "g.fa").write_text(">c\nACGT\n")
    with pytest.raises(ValueError) as ei:
        pileup.pileup_command(str(tmp_path / "out"), str(tmp_path / "g.fa"), str(tmp_path / "p"))
    assert "--cigar" in str(ei.value)
