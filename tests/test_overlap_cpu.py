"""The overlap stage without a GPU: the three statements of the definition held to each other (tests/overlap_ref.py), the host side
of chiron_amd.overlap on the reference as its aligner -- seeding, the band's edge rule, classification, PAF coordinates, the
planted case -- and every refusal of chiron_align_overlap, all of which come before a device is asked for."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import map_ref
import overlap_cases as cases
import overlap_ref as ref
from chiron_amd import _lib, assess, overlap


# ----------------------------------------------------------------------------------------------------------------------------
# the definition, three times
# ----------------------------------------------------------------------------------------------------------------------------
def test_three_statements_agree_on_every_small_pair():
    """Every pair of a two-letter alphabet with n <= 4 and m <= 5 at every band inside [-n, m]: the brute force over all paths, the
    plain recurrence and the numpy rows give the same (cost, M, s, e)."""
    checked = 0
    for n in range(5):
        for m in range(6):
            brute = ref.brute_force_all(n, m)
            keys = sorted(brute)
            reads, index = [], {}
            for a, b, _, _ in keys:
                for seq in (a, b):
                    if seq not in index:
                        index[seq] = len(reads)
                        reads.append(np.array(seq, dtype=np.uint8))
            got = ref.rows(reads, [(index[a], index[b], dlo, dhi) for a, b, dlo, dhi in keys])
            for key, row in zip(keys, got):
                want = brute[key]
                assert tuple(int(v) for v in row) == want, (key, row, want)
                assert ref.recurrence(*key) == want, key
                checked += 1
    assert checked == sum((2 ** n) * (2 ** m) * (n + m + 1) * (n + m + 2) // 2 for n in range(5) for m in range(6))


def test_recurrence_and_rows_agree_on_longer_reads():
    """Four letters and code 4, n and m up to 40, bands of every kind, clipped ones included; and the facts the definition states:
    cost <= 0 when the band holds diagonal -n or m, cost and M of one parity class (cost + M = 2 E), s and e inside the band."""
    rng = np.random.default_rng(5)
    reads, pairs = [], []
    for _ in range(120):
        n, m = int(rng.integers(0, 41)), int(rng.integers(0, 41))
        b = rng.integers(0, 5, m).astype(np.uint8)
        a = rng.integers(0, 5, n).astype(np.uint8)
        if n and m and rng.random() < 0.6:                                     # related reads: a piece of b, mutated
            lo = int(rng.integers(0, m))
            a = np.array(ref.codes_of(map_ref.mutate_counted("".join("ACGTN"[c] for c in b[lo:lo + n]), 0.12, rng)[0]), dtype=np.uint8)
        dlo = int(rng.integers(-len(a) - 3, m + 1))
        dhi = int(rng.integers(max(dlo, -len(a)), m + 4))
        reads += [a, b]
        pairs.append((len(reads) - 2, len(reads) - 1, dlo, dhi))
    got = ref.rows(reads, pairs)
    for (ia, ib, dlo, dhi), row in zip(pairs, got):
        a, b = reads[ia], reads[ib]
        want = ref.recurrence(a, b, dlo, dhi)
        assert tuple(int(v) for v in row) == want
        cost, M, s, e = want
        lo, hi = ref.clip(len(a), len(b), dlo, dhi)
        assert (cost + M) % 2 == 0 and M >= 0 and lo <= s - len(a) <= hi and lo <= e - len(a) <= hi
        if lo == -len(a) or hi == len(b):
            assert cost <= 0
    with pytest.raises(ValueError):
        ref.rows([np.zeros(3, np.uint8), np.zeros(4, np.uint8)], [(0, 1, 5, 9)])
    assert ref.recurrence("ACG", "ACGT", 5, 9) is None


def test_a_band_without_a_corner_can_cost_more_than_nothing():
    """The empty path exists only at the corners (0, m) and (n, 0): a band that holds neither diagonal has no path of cost 0."""
    assert ref.recurrence("AAAA", "CCCC", 0, 0) == (8, 0, 4, 4)
    assert ref.recurrence("AAAA", "CCCC", -4, 4) == (0, 0, 0, 0)
    assert ref.recurrence("AAAA", "AAAA", 0, 0) == (-4, 4, 4, 4)


# ----------------------------------------------------------------------------------------------------------------------------
# the host side
# ----------------------------------------------------------------------------------------------------------------------------
def test_classification_from_s_and_e():
    n, m = 10, 20
    assert overlap.classify(n, m, n + 3, 13) == ("contained", (0, 10), (3, 13))
    assert overlap.classify(n, m, n, m) == ("contained", (0, 10), (0, 20))                   # corner to corner: all of a
    assert overlap.classify(n, m, n + 15, m) == ("contained", (0, 10), (15, 20))             # row 0 to the corner (n, m): all of a
    assert overlap.classify(n, m, n - 6, m) == ("contains", (6, 10), (0, 20))                # column 0 to the corner (n, m): all of b
    assert overlap.classify(n, m, n, m + 4) == ("contains", (0, 6), (0, 20))                 # the corner (0, 0) to column m: all of b
    assert overlap.classify(20, 10, 20 - 4, 10 - 14 + 20) == ("contains", (4, 14), (0, 10))
    assert overlap.classify(n, m, n - 6, 4) == ("dovetail_ab", (6, 10), (0, 4))
    assert overlap.classify(n, m, n + 15, m - 5 + n) == ("dovetail_ba", (0, 5), (15, 20))
    assert overlap.touches_edge(n, m, -3, 5, n - 3, 2) and overlap.touches_edge(n, m, -3, 5, n, n + 5)
    assert not overlap.touches_edge(n, m, -10, 20, 0, 30) and not overlap.touches_edge(n, m, -3, 5, n - 2, n + 4)


@pytest.mark.parametrize("kind,strand", cases.TYPED)
def test_types_and_paf_coordinates_against_a_plain_walk(built, kind, strand):
    """One exact shared stretch of 300 bases in each arrangement, on both strands: the overlap's type, M and E, and the PAF line --
    the query's span on the query's strand as given -- are what searching the strings gives."""
    reads, want = cases.typed_case(kind, strand, 900 + cases.TYPED.index((kind, strand)))
    names, result = overlap.find_overlaps(reads, min_overlap=100, aligner=cases.reference_aligner)
    assert names == ["a", "b"] and result["candidate_pairs"] == 1 and len(result["overlaps"]) == 1
    o = result["overlaps"][0]
    assert (o["type"], o["strand"], o["match"], o["edit"], o["length"], o["identity"]) == (kind, strand, 300, 0, 300, 1.0)
    line = overlap.paf_lines(names, result)[0].split("\t")
    assert tuple(line[:12]) == tuple(str(v) for v in want["paf"])
    assert line[12:] == ["tp:A:" + overlap.TYPE_LETTER[kind], "ty:Z:" + kind, "ed:i:0"]


def test_edge_rule_needs_one_doubling(built):
    """tests/overlap_cases.edge_case: at w = 8 the result ends on the band's upper edge, at w = 16 it lies inside."""
    reads, cand, band = cases.edge_case()
    first = ref.rows(reads, [(0, 1, 50 - band, 50 + band)])[0]
    assert tuple(int(v) for v in first) == (-175, 197, 250, 258) and overlap.touches_edge(len(reads[0]), len(reads[1]), 42, 58, int(first["start"]), int(first["end"]))
    result = overlap.overlap_pairs(reads, [cand], band=band, min_overlap=100, aligner=cases.reference_aligner)
    assert (result["aligned"], result["realigned"], result["edge"], result["batches"]) == (1, 1, 0, 2)
    o = result["overlaps"][0]
    assert (o["type"], o["widenings"], o["band"]) == ("contained", 1, 16)
    assert (o["a_start"], o["a_end"], o["b_start"], o["b_end"], o["match"], o["edit"]) == (0, 200, 50, 262, 200, 12)
    stuck = overlap.overlap_pairs(reads, [dict(cand, delta=50)], band=0, min_overlap=100, aligner=cases.reference_aligner)    # 0 doubles to 0
    assert (stuck["realigned"], stuck["edge"], stuck["overlaps"]) == (overlap.MAX_WIDENINGS, 1, [])


def test_candidates_meet_every_pair_once():
    """The planted reads: a candidate's a is below its b, no (a, b, strand) twice, every candidate at min_votes or more, a read's
    candidates in the stated order, and max_overlaps cuts each read's list to its head."""
    reads, _ = cases.planted(cases.SEEDS[0])
    coded = [assess.encode(reads[name]) for name in sorted(reads)]
    index = overlap.build_index(coded)
    cands = overlap.candidates(index, coded)
    assert len(cands) > 500 and all(c["a"] < c["b"] and c["votes"] >= overlap.MIN_VOTES for c in cands)
    assert len({(c["a"], c["b"], c["strand"]) for c in cands}) == len(cands)
    keys = [(c["a"], -c["votes"], c["b"], c["strand"] != "forward") for c in cands]
    assert keys == sorted(keys)
    few = overlap.candidates(index, coded, max_overlaps=3)
    for q in range(len(coded)):
        assert [c for c in few if c["a"] == q] == [c for c in cands if c["a"] == q][:3]
    from chiron_amd import map as cmap
    for codes in (coded[3], assess.reverse_complement(coded[4])):                          # the sorted lookup finds map.hits' hits
        d1, g1 = cmap.hits(index, codes)
        d2, g2 = overlap._hits(index, codes)
        assert len(d1) > 100 and sorted(zip(d1.tolist(), g1.tolist())) == sorted(zip(d2.tolist(), g2.tolist()))
    starts = overlap.read_starts([len(c) for c in coded])
    assert starts[1] == len(coded[0]) + overlap.SEPARATOR


# what the reference attains on the planted case at the defaults, measured on the CPU: (true pairs, found, kept pairs that are not
# true pairs, type right, largest end error in bases); DESIGN holds the table
PLANTED = {11: (562, 559, 1, 559, 7), 12: (580, 575, 0, 575, 6), 13: (543, 543, 0, 543, 5)}
RECALL_FLOOR = 575 / 580


@pytest.mark.parametrize("seed", cases.SEEDS)
def test_planted_case_on_the_reference(built, seed):
    """tests/overlap_cases.planted through find_overlaps with the numpy reference as aligner: the figures of DESIGN's table, as
    measured; every kept pair shares bases on the genome, on the right strand."""
    reads, truth = cases.planted(seed)
    names, result = overlap.find_overlaps(reads, aligner=cases.reference_aligner)
    ev = cases.evaluate(names, result, truth)
    assert (ev["true_pairs"], ev["found"], ev["false_kept"], ev["type_right"], ev["max_end_error"]) == PLANTED[seed]
    assert ev["no_shared_bases"] == 0 and ev["strand_right"] == ev["found"]
    assert ev["found"] / ev["true_pairs"] >= RECALL_FLOOR
    assert result["kept"]["contained"] > 0 and result["kept"]["contains"] > 0 and result["edge"] == 0
    assert result["aligned"] == result["candidate_pairs"] == len(result["overlaps"]) + result["dropped"]["short"] + result["dropped"]["identity"]


def test_command_writes_paf_and_report(built, tmp_path):
    """`overlap_command` from a FASTQ folder, the reference as aligner: twelve columns and three tags a line, the report's counts."""
    reads, _ = cases.typed_case("dovetail_ab", "reverse", 31)
    for name, seq in reads.items():
        (tmp_path / (name + ".fastq")).write_text("@%s\n%s\n+\n%s\n" % (name, seq, "I" * len(seq)))
    report = overlap.overlap_command(str(tmp_path), str(tmp_path / "out"), min_overlap=100, aligner=cases.reference_aligner)
    lines = (tmp_path / "out" / "overlaps.paf").read_text().splitlines()
    assert len(lines) == 1 and len(lines[0].split("\t")) == 15 and lines[0].split("\t")[4] == "-"
    assert json.loads((tmp_path / "out" / "overlap_report.json").read_text()) == report
    assert report["reads"] == 2 and report["kept"] == {"contained": 0, "contains": 0, "dovetail_ab": 1, "dovetail_ba": 0, "total": 1}
    assert report["parameters"]["band"] == 256 and report["batches"] == 1 and report["dropped"] == {"short": 0, "identity": 0}


# ----------------------------------------------------------------------------------------------------------------------------
# the library, before any device
# ----------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_constants(built):
    names = {n for n, _, _ in _lib.SYMBOLS}
    assert {"chiron_align_overlap", "chiron_align_overlap_workspace_size"} <= names
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "chiron_amd.h")) as f:
        header = f.read()
    assert "#define CHIRON_OVERLAP_MAX_READ (1 << 17)" in header and _lib.OVERLAP_MAX_READ == 1 << 17 == overlap.MAX_READ
    assert _lib.load().chiron_abi_version() == 7


def test_workspace_size_formula(built):
    up = lambda v: (v + 255) & ~255
    size = overlap.workspace_size
    assert size(0, 0, 0, 0) == 0
    assert size(3, 1000, 10, 4096) == up(320) + up(200) + up(1000)                           # the band stays in LDS: no rows
    assert size(3, 1000, 10, 4097) == up(320) + up(200) + up(1000) + up(10 * 4097 * 8)
    assert size(3, 1000, 5000, 5000) == up(5000 * 32) + up(5000 * 20) + up(1000) + up(2048 * 5000 * 8)
    lib = _lib.load()
    n = C.c_size_t(77)
    for args, status, text in (((-1, 0, 0, 0), _lib.ERR_INVALID, "negative reads / total_bases / pairs / max_band"),
                               ((1, 10, (1 << 24) + 1, 0), _lib.ERR_OVERFLOW, "16777217 pairs in one call, at most 2^24"),
                               (((1 << 24) + 1, 10, 1, 0), _lib.ERR_OVERFLOW, "16777217 reads in one call, at most 2^24"),
                               ((1, (1 << 17) + 1, 1, 0), _lib.ERR_OVERFLOW, "131073 bases in 1 reads, a read has at most 131072"),
                               ((2, 100, 1, (1 << 18) + 2), _lib.ERR_OVERFLOW, "a band of 262146 diagonals, the largest table has 262145")):
        assert lib.chiron_align_overlap_workspace_size(*args, C.byref(n)) == status
        assert text in lib.chiron_last_error().decode() and n.value == 77
    assert lib.chiron_align_overlap_workspace_size(1, 1, 1, 1, None) == _lib.ERR_INVALID


def _call(lib, codes=(0, 1, 2, 3, 4, 0, 1), read_off=(0, 3, 7), reads=2, a=(0,), b=(1,), dlo=(-3,), dhi=(4,), pairs=1, out=True, ws=0,
          ws_bytes=1 << 20, flags=0):
    arr = lambda v, t: None if v is None else np.ascontiguousarray(v, dtype=t)
    codes, read_off = arr(codes, np.uint8), arr(read_off, np.int64)
    cols = [arr(v, np.int32) for v in (a, b, dlo, dhi)]
    o = np.full((max(pairs, 1), 5), 77, dtype=np.int32)
    ptr = lambda v: None if v is None else v.ctypes.data
    st = lib.chiron_align_overlap(0, ptr(codes), ptr(read_off), reads, *[ptr(c) for c in cols], pairs, ptr(o) if out else None, ws, ws_bytes, flags, None)
    return st, lib.chiron_last_error().decode(), o


def test_every_refusal_comes_before_a_device(built):
    lib = _lib.load()
    INVALID, OVERFLOW = _lib.ERR_INVALID, _lib.ERR_OVERFLOW
    st, msg, o = _call(lib)
    assert st == INVALID and "chiron_align_overlap: null workspace" in msg              # everything else passed: the last check before the device
    assert (o == 77).all()
    long_off = (0, 3, 3 + (1 << 17) + 1)
    for kw, status, text in (
            (dict(flags=2), INVALID, "unknown flags 0x2"),
            (dict(pairs=-1), INVALID, "negative count (reads 2, pairs -1)"),
            (dict(reads=-2), INVALID, "negative count (reads -2, pairs 1)"),
            (dict(pairs=(1 << 24) + 1), OVERFLOW, "16777217 pairs in one call, at most 2^24"),
            (dict(read_off=None), INVALID, "null read_off"),
            (dict(a=None), INVALID, "null pair_a / pair_b / dlo / dhi"),
            (dict(dhi=None), INVALID, "null pair_a / pair_b / dlo / dhi"),
            (dict(out=False), INVALID, "null out"),
            (dict(codes=None), INVALID, "null codes"),
            (dict(read_off=(-1, 3, 7)), INVALID, "read_off[0] = -1 is negative"),
            (dict(read_off=(0, 3, 2)), INVALID, "read_off[2] = 2 below its predecessor 3"),
            (dict(codes=(0, 1, 2, 3, 5, 0, 1)), INVALID, "code 5 at 1 of read 1 outside 0..4"),
            (dict(codes=(9, 9, 0, 1, 255, 0, 0, 0, 0), read_off=(2, 5, 9)), INVALID, "code 255 at 2 of read 0 outside 0..4"),
            (dict(read_off=long_off, codes=np.zeros(long_off[-1], np.uint8)), OVERFLOW, "read 1 has 131073 bases, at most 131072"),
            (dict(b=(2,)), INVALID, "pair 0 names reads 0 and 2, the call has 2"),
            (dict(a=(-1,)), INVALID, "pair 0 names reads -1 and 1, the call has 2"),
            (dict(dlo=(5,), dhi=(9,)), INVALID, "pair 0: the band 5 .. 9 holds no diagonal of the table's -3 .. 4"),
            (dict(dlo=(-9,), dhi=(-4,)), INVALID, "pair 0: the band -9 .. -4 holds no diagonal of the table's -3 .. 4"),
            (dict(dlo=(2,), dhi=(1,)), INVALID, "pair 0: the band 2 .. 1 holds no diagonal"),
            (dict(ws_bytes=767), INVALID, "a workspace of 767 bytes, 768 are needed")):
        st, msg, o = _call(lib, **kw)
        assert st == status and text in msg and msg.startswith("chiron_align_overlap: "), (kw, st, msg)
        assert (o == 77).all(), kw
    st, msg, o = _call(lib, pairs=0, read_off=None, a=None, out=False)                      # zero pairs: nothing is looked at
    assert st == _lib.OK
    assert overlap.workspace_size(2, 7, 1, 8) == 768
