"""CPU: the alignment traceback's definition and host side.  The reference walk (tests/trace_ref.py) against a brute force over
every alignment of small pairs; the tight band w* = (E - |m-n|) / 2 in plain Python (enough on 1000 pairs, not slack: w* - 1 is
not); cigar, error_profile and merge on hand-written cases; the C ABI's host-only refusals and size functions (no GPU is looked
for); SAM and PAF formatting from a map_reads result made with the reference aligner and the reference tracer."""
import ctypes as C
import itertools

import numpy as np
import pytest

from chiron_amd import _lib, assess, map as cmap

import assess_ref
import map_ref
import trace_ref


def _ops(text):
    return np.array(["=XID".index(ch) for ch in text], dtype=np.uint8)


def test_reference_walk_is_the_smallest_reversed_string_of_every_small_pair():
    """Every pair over {A, C} with n, m <= 5 (3969 pairs), and seeded pairs with N among the letters."""
    seqs = ["".join(t) for k in range(6) for t in itertools.product("AC", repeat=k)]
    pairs = [(a, b) for a in seqs for b in seqs]
    rng = np.random.default_rng(11)
    pairs += [(assess_ref.random_seq(int(rng.integers(0, 6)), rng, "ACN"), assess_ref.random_seq(int(rng.integers(0, 6)), rng, "ACN"))
              for _ in range(400)]
    pairs += [("N", "N"), ("NN", "N"), ("ANA", "ANA"), ("NNNNN", "NNNNN")]
    for a, b in pairs:
        E, M, ops = trace_ref.full_trace(a, b)
        bE, bM, bops = trace_ref.brute(a, b)
        assert (E, M) == (bE, bM) == assess_ref.exhaustive(a, b) if len(a) + len(b) <= 6 else (E, M) == (bE, bM), (a, b)
        assert ops.tolist() == bops.tolist(), (a, b, trace_ref.cigar(ops), trace_ref.cigar(bops))
        trace_ref.check_ops(a, b, ops, E, M)


def test_the_tight_band_holds_every_optimal_alignment_and_is_not_slack():
    """1000 seeded pairs with n, m <= 40: the walk inside w* equals the full-table walk on all of them; at w* - 1 (where w* >= 1)
    some pair differs, so the bound is not slack by construction."""
    rng = np.random.default_rng(12)
    narrower_differs = 0
    for k in range(1000):
        a = assess_ref.random_seq(int(rng.integers(0, 41)), rng, "ACGTN" if k % 5 == 0 else "AC" if k % 3 == 0 else "ACGT")
        b = assess_ref.mutate(a, 0.3, rng)[:40] if k % 2 else assess_ref.random_seq(int(rng.integers(0, 41)), rng, "AC" if k % 3 == 0 else "ACGT")
        E, M, ops = trace_ref.full_trace(a, b)
        w = trace_ref.tight_band(len(a), len(b), E)
        assert w >= 0
        bE, bM, bops = trace_ref.banded_trace(a, b, w)
        assert (bE, bM) == (E, M) and bops.tolist() == ops.tolist(), (a, b, w)
        if w >= 1:
            nE, nM, nops = trace_ref.banded_trace(a, b, w - 1)
            narrower_differs += (nE, nM) != (E, M) or nops.tolist() != ops.tolist()
    assert narrower_differs > 0


def test_cigar_and_error_profile_on_hand_written_cases():
    assert assess.cigar(_ops("")) == "*" == trace_ref.cigar(_ops(""))
    assert assess.cigar(_ops("=")) == "1="
    assert assess.cigar(_ops("==XIIDD=")) == "2=1X2I2D1=" == trace_ref.cigar(_ops("==XIIDD="))
    # a homopolymer called one short and one long: the gap is left-aligned, and the run is counted at (5, 4) and at (4, 5)
    E, M, ops = trace_ref.full_trace("AAAA", "AAAAA")
    assert assess.cigar(ops) == "1D4="
    prof = assess.error_profile("AAAA", "AAAAA", ops)
    assert prof["homopolymer"][5][4] == 1 and np.sum(prof["homopolymer"]) == 1
    assert prof["deletion"] == [1, 0, 0, 0, 0] and prof["insertion"] == [0] * 5 and prof["substitution"][0][0] == 4
    E, M, ops = trace_ref.full_trace("AAAAA", "AAAA")
    assert assess.cigar(ops) == "1I4="
    prof = assess.error_profile("AAAAA", "AAAA", ops)
    assert prof["homopolymer"][4][5] == 1 and np.sum(prof["homopolymer"]) == 1 and prof["insertion"] == [1, 0, 0, 0, 0]
    # read ACGTTN-A against reference ACCTTNGA: one substitution G for C, N against N is a mismatch that is no substitution
    read, ref, ops = "ACGTTNA", "ACCTTNGA", _ops("==X==XD=")
    prof = assess.error_profile(read, ref, ops)
    want = trace_ref.error_profile(read, ref, ops)
    assert prof == want
    assert prof["substitution"][1][2] == 1 and prof["other_mismatch"] == 1 and prof["deletion"] == [0, 0, 1, 0, 0]
    assert np.trace(prof["substitution"]) == 5
    # runs A (1, called 1), CC (2, called 1), TT (2, 2), G (1, 0), A (1, 1); the N is no run
    hp = np.array(prof["homopolymer"])
    assert hp[1][1] == 2 and hp[2][1] == 1 and hp[2][2] == 1 and hp[1][0] == 1 and hp.sum() == 5 and hp[0].sum() == 0
    # long runs and long calls collect in the last row and column; an insertion after the last reference base belongs to no run
    read, ref = "A" * 25 + "C" + "G" * 3, "A" * 12 + "C"
    ops = _ops("I" * 13 + "=" * 13 + "III")
    prof = assess.error_profile(read, ref, ops)
    assert prof == trace_ref.error_profile(read, ref, ops)
    assert prof["homopolymer"][10][20] == 1 and prof["homopolymer"][1][1] == 1 and np.sum(prof["homopolymer"]) == 2
    assert prof["insertion"] == [13, 0, 3, 0, 0]
    # lower case, U, and an alignment that does not cover the sequences
    assert assess.error_profile("acgu", "ACGT", _ops("====")) == trace_ref.error_profile("ACGT", "ACGT", _ops("===="))
    with pytest.raises(ValueError):
        assess.error_profile("ACG", "ACGT", _ops("===="))


def test_error_profile_and_merge_equal_the_reference_on_random_pairs():
    rng = np.random.default_rng(13)
    got, want = [], []
    for k in range(60):
        alphabet = "ACGTN" if k % 4 == 0 else "AC" if k % 3 == 0 else "ACGT"
        ref = assess_ref.random_seq(int(rng.integers(0, 120)), rng, alphabet)
        read = assess_ref.mutate(ref, 0.25, rng)
        ops = trace_ref.trace(read, ref)
        got.append(assess.error_profile(read, ref, ops))
        want.append(trace_ref.error_profile(read, ref, ops))
        assert got[-1] == want[-1], (read, ref)
        assert assess.cigar(ops) == trace_ref.cigar(ops)
    assert assess.merge(got) == trace_ref.merge(want)
    assert assess.merge([]) == trace_ref.merge([])
    total = assess.merge(got)
    assert np.sum(total["homopolymer"]) > 60 and np.sum(total["substitution"]) > 1000 and total["other_mismatch"] > 0


def _trace_call(lib, codes, read_off, ref_off, edit, match, ops_off):
    codes = np.asarray(codes, dtype=np.uint8)
    read_off, ref_off, ops_off = (np.asarray(v, dtype=np.int64) for v in (read_off, ref_off, ops_off))
    edit, match = np.asarray(edit, dtype=np.int32), np.asarray(match, dtype=np.int32)
    ops = np.full(max(int(ops_off[-1]), 1), 9, dtype=np.uint8)
    status = np.zeros(len(edit), dtype=np.int32)
    st = lib.chiron_align_trace(0, codes.ctypes.data, read_off.ctypes.data, ref_off.ctypes.data, len(edit), edit.ctypes.data,
                                match.ctypes.data, ops_off.ctypes.data, 0, ops.ctypes.data, status.ctypes.data, None, None)
    assert np.all(ops == 9)
    return st, lib.chiron_last_error().decode()


def test_trace_refuses_bad_arguments_before_it_looks_for_a_gpu(built):
    """Every refusal below is CHIRON_ERR_INVALID or CHIRON_ERR_OVERFLOW although the workspace is null and the machine may have
    no GPU: the checks come first.  A valid call then stops at the null workspace."""
    lib = _lib.load()
    codes = [0, 1, 2, 3, 0, 1, 2]                       # read ACGT, reference ACG: E = 1, M = 3, 4 columns
    ok = dict(codes=codes, read_off=[0, 4], ref_off=[4, 7], edit=[1], match=[3], ops_off=[0, 4])
    st, msg = _trace_call(lib, **ok)
    assert st == _lib.ERR_INVALID and "null workspace" in msg
    for change, word in ((dict(edit=[0], ops_off=[0, 3]), "edit distance"), (dict(edit=[5], match=[0], ops_off=[0, 5]), "edit distance"),
                         (dict(ops_off=[0, 5]), "columns"), (dict(ops_off=[0, 3]), "columns"), (dict(ops_off=[-1, 3]), "ops_off"),
                         (dict(match=[4], ops_off=[0, 5]), "matches"), (dict(match=[-1], ops_off=[0, 0]), "matches"),
                         (dict(codes=[0, 1, 5, 3, 0, 1, 2]), "code 5"), (dict(read_off=[4, 0]), "read_off"),
                         (dict(ref_off=[-3, 0], edit=[1], match=[3]), "ref_off")):
        st, msg = _trace_call(lib, **dict(ok, **change))
        assert st == _lib.ERR_INVALID and word in msg, (change, st, msg)
    # the second pair of two is the bad one
    st, msg = _trace_call(lib, codes=codes + codes, read_off=[0, 4, 11], ref_off=[4, 7, 14], edit=[1, 9], match=[3, 3], ops_off=[0, 4, 16])
    assert st == _lib.ERR_INVALID and "pair 1" in msg                     # 7 bases against 7 cannot cost 9
    long = assess.MAX_LEN + 1
    st, msg = _trace_call(lib, codes=np.zeros(long + 1, np.uint8), read_off=[0, long], ref_off=[long, long + 1], edit=[long - 1], match=[1],
                          ops_off=[0, long])
    assert st == _lib.ERR_OVERFLOW
    status = np.zeros(1, np.int32)
    assert lib.chiron_align_trace(0, None, None, None, 0, None, None, None, 0, None, None, None, None) == _lib.OK      # no pairs: a no-op
    assert lib.chiron_align_trace(0, None, None, None, 1, None, None, None, 1, None, status.ctypes.data, None, None) == _lib.ERR_INVALID
    with pytest.raises(ValueError):
        assess.align_ops(["A"], [])
    assert assess.align_ops([], []) == []


def test_trace_sizes(built):
    """One pair's back-pointers are (n + m + 1) rows of ceil(ceil(band / 2) / 4) bytes, the band being the diagonals
    [min(0, m-n) - w*, max(0, m-n) + w*] clipped to the table; the workspace holds them next to the codes and the columns, and a
    row of keys per workgroup only when a band is wider than LDS."""
    def want(n, m, E):
        w = (E - abs(m - n)) // 2
        band = min(max(0, m - n) + w, m) - max(min(0, m - n) - w, -n) + 1
        return (n + m + 1) * (((band + 1) // 2 + 3) // 4), band
    for n, m, E in ((0, 0, 0), (0, 5, 5), (4, 0, 4), (700, 700, 0), (900, 640, 260), (300, 300, 300), (513, 255, 400), (10000, 10100, 1040),
                    (4096, 4096, 4096), (4095, 100, 4095), (1 << 17, 1 << 17, 1 << 17)):
        assert assess.trace_pair_size(n, m, E) == want(n, m, E), (n, m, E)
    assert assess.trace_pair_size(10000, 10100, 1040)[0] == 20101 * 131       # 2.6 MB where the full table would take 25 MB
    for bad in ((5, 3, 1), (5, 3, 6), (-1, 3, 3)):
        with pytest.raises(_lib.ChironError) as ei:
            assess.trace_pair_size(*bad)
        assert ei.value.status == _lib.ERR_INVALID
    with pytest.raises(_lib.ChironError) as ei:
        assess.trace_pair_size(assess.MAX_LEN + 1, 5, assess.MAX_LEN + 1)
    assert ei.value.status == _lib.ERR_OVERFLOW
    size = assess.trace_workspace_size
    base = size(8, 0, 1000, 201)
    assert base >= 8 * 2 * 1000 * 2 and size(8, 1 << 20, 1000, 201) - base == 1 << 20
    assert size(8, 0, 1000, assess.LDS_SLOTS) == base                          # the widest band LDS holds: no rows
    rows = size(8, 0, 4096, assess.LDS_SLOTS + 1) - size(8, 0, 4096, assess.LDS_SLOTS)
    assert 0 <= rows - 8 * (assess.LDS_SLOTS + 2) * 8 < 256                      # one row of keys per workgroup, 8 workgroups
    assert size(0, 0, 0, 0) == 0 and size(5000, 0, 100, 1 << 20) - size(5000, 0, 100, 0) == 0      # a band no table of 100 bases has
    for args, status in (((-1, 0, 0, 0), _lib.ERR_INVALID), ((1, -1, 0, 0), _lib.ERR_INVALID), ((1, 0, assess.MAX_LEN + 1, 0), _lib.ERR_OVERFLOW),
                         (((1 << 24) + 1, 0, 10, 0), _lib.ERR_OVERFLOW), ((1, (1 << 46) + 1, 10, 0), _lib.ERR_OVERFLOW)):
        with pytest.raises(_lib.ChironError) as ei:
            size(*args)
        assert ei.value.status == status, args
    # the planner: consecutive pairs, every batch within the budget, a single pair always a batch
    lens = [400, 500, 450, 300, 480]
    edits = [60, 80, 40, 300, 70]
    one = [size(1, assess.trace_pair_size(n, n, e)[0], n, assess.trace_pair_size(n, n, e)[1]) for n, e in zip(lens, edits)]
    assert [b for b, _ in assess.plan_trace_batches(lens, lens, edits, 1)] == [[0], [1], [2], [3], [4]]
    assert [b for b, _ in assess.plan_trace_batches(lens, lens, edits, 1 << 30)] == [[0, 1, 2, 3, 4]]
    plan = assess.plan_trace_batches(lens, lens, edits, max(one) + min(one))
    assert sum((b for b, _ in plan), []) == [0, 1, 2, 3, 4] and 1 < len(plan) < 5 and all(nb <= max(one) + min(one) for _, nb in plan)


def _reference_aligner(rs, ws, band0):
    return map_ref.infix_rows(rs, ws, band0, cmap.INFIX_DTYPE)


def _reference_tracer(rs, fs):
    return [trace_ref.trace(map_ref.as_str(a), map_ref.as_str(b)) for a, b in zip(rs, fs)]


def test_sam_and_paf_lines_from_a_traced_mapping():
    """A two-contig genome, a forward and a reverse-strand read and one that does not map, through map_reads with the reference
    aligner and add_cigars with the reference tracer.  Each SAM line's CIGAR replayed over its SEQ and the genome from POS
    reproduces both and NM; the PAF's cg:Z: tag is the SAM CIGAR; without add_cigars the PAF has its twelve columns."""
    rng = np.random.default_rng(14)
    contigs = [("ctgA", assess_ref.random_seq(3000, rng)), ("ctgB", assess_ref.random_seq(2500, rng))]
    fwd = assess_ref.mutate(contigs[0][1][700:1100], 0.1, rng)
    rev = map_ref.revcomp(assess_ref.mutate(contigs[1][1][1200:1500], 0.1, rng))
    reads = {"fwd": fwd, "rev": rev, "noise": assess_ref.random_seq(300, rng)}
    genome = cmap.Genome(contigs)
    result = cmap.map_reads(reads, genome, aligner=_reference_aligner)
    plain = cmap.paf_lines(result, genome)
    assert len(plain) == 2 and all(len(ln.split("\t")) == 12 for ln in plain)
    assert cmap.sam_lines(result, reads, genome) == ["@HD\tVN:1.6\tSO:unknown", "@SQ\tSN:ctgA\tLN:3000", "@SQ\tSN:ctgB\tLN:2500"]
    assert cmap.add_cigars(result, reads, genome, tracer=_reference_tracer) is result
    by = {r["name"]: r for r in result["reads"]}
    assert by["noise"]["status"] == "unmapped" and "cigar" not in by["noise"]
    sam = cmap.sam_lines(result, reads, genome)
    assert sam[:3] == ["@HD\tVN:1.6\tSO:unknown", "@SQ\tSN:ctgA\tLN:3000", "@SQ\tSN:ctgB\tLN:2500"] and len(sam) == 5
    paf = cmap.paf_lines(result, genome)
    assert [ln.split("\t")[:12] for ln in paf] == [ln.split("\t") for ln in plain]
    seqs = dict(contigs)
    for line, pline in zip(sam[3:], paf):
        f = line.split("\t")
        assert len(f) == 12
        name, flag, contig, pos, mapq, cg, rnext, pnext, tlen, seq, qual, nm = f
        r = by[name]
        assert (int(flag), contig, int(pos), mapq, rnext, pnext, tlen, qual) == (0 if name == "fwd" else 16, r["contig"], r["start"] + 1, "255", "*", "0", "0", "*")
        assert seq == (reads[name] if name == "fwd" else map_ref.revcomp(reads[name]))
        used_read, used_ref, edits = trace_ref.replay(cg, seq, seqs[contig][int(pos) - 1:])
        assert used_read == len(seq) and used_ref == r["end"] - r["start"] and nm == "NM:i:%d" % edits == "NM:i:%d" % r["edit"]
        assert pline.split("\t")[12] == "cg:Z:" + cg and len(pline.split("\t")) == 13
        assert cg == r["cigar"] == trace_ref.cigar(trace_ref.trace(seq, seqs[contig][r["start"]:r["end"]]))
    assert by["fwd"]["contig"] == "ctgA" and by["rev"]["contig"] == "ctgB" and by["rev"]["strand"] == "reverse"
