"""CPU: the read mapper without a GPU.  The reference of tests/map_ref.py against brute force; the band-doubling rule (nothing
E <= w accepts differs from the full table); the host side of chiron_amd.map (index, votes, tie rules, writers); the argument
checks of chiron_align_infix, which happen before a device is looked for."""
import ctypes as C
import os

import numpy as np
import pytest

import assess_ref
import map_ref

E2E_SEED = 11                           # shared with test_gpu_map.py: the two unrelated reads get fewer than min_votes seeds


def test_full_table_equals_brute_force_on_every_small_pair():
    """All pairs over {A, C} with n <= 4, m <= 6."""
    words = lambda k: ["".join("AC"[(v >> t) & 1] for t in range(k)) for v in range(1 << k)]
    checked = 0
    for n in range(5):
        for m in range(7):
            for a in words(n):
                for b in words(m):
                    assert map_ref.full_table(a, b) == map_ref.brute_force(a, b), (a, b)
                    checked += 1
    assert checked == sum(2 ** n for n in range(5)) * sum(2 ** m for m in range(7))
    assert map_ref.full_table("", "") == (0, 0, 0, 0) and map_ref.full_table("", "ACG") == (0, 0, 0, 0)
    assert map_ref.full_table("ACG", "") == (3, 0, 0, 0)
    assert map_ref.full_table("N", "N") == (1, 0, 0, 0)               # code 4 matches nothing: delete it against the empty substring
    assert map_ref.full_table("ACGT", "TTACGTACGT") == (0, 4, 2, 6)   # two exact copies: the smaller s


def test_band_rule_accepts_nothing_that_differs_from_the_full_table():
    """About 1000 random pairs, related and unrelated, m < n, m = n and m > n, at w = 0, 1, 2, 4: whatever E <= w (or a band that
    covers the table) accepts equals the full table in all four values; and the doubling loop ends on the full-table result at
    the band expected_band() derives from the true E."""
    rng = np.random.default_rng(21)
    accepted = {0: 0, 1: 0, 2: 0, 4: 0}
    pairs = 0
    for k in range(1000):
        n = int(rng.integers(0, 25))
        kind = k % 4
        if kind == 0:                                                   # unrelated
            a, b = assess_ref.random_seq(n, rng), assess_ref.random_seq(int(rng.integers(0, 40)), rng)
        else:                                                           # the read lies in the window, with flanks of 0 .. 8
            core = assess_ref.random_seq(n, rng, "ACGT" if kind < 3 else "AC")
            a = assess_ref.mutate(core, (0.0, 0.1, 0.3, 0.2)[kind], rng)
            b = assess_ref.random_seq(int(rng.integers(0, 9)), rng) + core + assess_ref.random_seq(int(rng.integers(0, 9)), rng)
            if k % 16 == 1:
                b = core[:n // 2]                                       # m < n
            elif k % 16 == 2:
                b = core                                                # m = n
        want = map_ref.full_table(a, b)
        for w in accepted:
            E, M, s, e, ok = map_ref.banded(a, b, w)
            assert E >= want[0], (a, b, w)
            if ok:
                accepted[w] += 1
                assert (E, M, s, e) == want, (a, b, w)
        for band0 in (0, 1, 4):
            got = map_ref.doubling(a, b, band0)
            assert got[:4] == want and got[4] == map_ref.expected_band(len(a), len(b), want[0], band0), (a, b, band0)
        pairs += 1
    assert pairs == 1000 and all(v > 100 for v in accepted.values()), accepted


# ------------------------------------------------------------------------------------------------------------------------------
# host side
# ------------------------------------------------------------------------------------------------------------------------------
def _genome(records):
    from chiron_amd import map as cmap
    return cmap.Genome(records)


def test_no_indexed_kmer_spans_two_contigs_or_holds_an_n():
    from chiron_amd import map as cmap
    rng = np.random.default_rng(31)
    a, b = assess_ref.random_seq(300, rng), assess_ref.random_seq(200, rng)
    b = b[:100] + "N" + b[101:]
    g = _genome([("a", a), ("b", b)])
    assert len(g.codes) == 500 + cmap.SEPARATOR and g.starts.tolist() == [0, 300 + cmap.SEPARATOR]
    val, pos = cmap.build_index(g.codes)
    assert len(val) == (300 - cmap.K + 1) + (200 - cmap.K + 1) - cmap.K          # every k-mer over the N is gone
    text = a + "N" * cmap.SEPARATOR + b
    for v, p in zip(val.tolist(), pos.tolist()):
        kmer = text[p:p + cmap.K]
        assert "N" not in kmer and (p + cmap.K <= 300 or p >= g.starts[1])
        assert v == int("".join(str("ACGT".index(ch)) for ch in kmer), 4)
    assert np.all(np.diff(val) >= 0)
    # the junction's k-mer exists nowhere: a read made of it finds nothing
    junction = assess_ref_encode(a[-8:] + b[:7])
    assert cmap.vote((val, pos), junction)["votes"] == 0
    assert g.contig_of(0) == 0 and g.contig_of(299) == 0 and g.contig_of(int(g.starts[1])) == 1


def assess_ref_encode(seq):
    from chiron_amd import assess
    return assess.encode(seq)


def test_max_occ_drops_the_over_frequent_kmers():
    from chiron_amd import map as cmap
    rng = np.random.default_rng(32)
    unit = assess_ref.random_seq(cmap.K, rng)
    filler = [assess_ref.random_seq(40, rng) for _ in range(6)]
    text = "".join(f + unit for f in filler)                       # the unit occurs 6 times
    codes = assess_ref_encode(text)
    unit_val = int("".join(str("ACGT".index(ch)) for ch in unit), 4)
    val, _ = cmap.build_index(codes, max_occ=6)
    assert int((val == unit_val).sum()) == 6
    val, pos = cmap.build_index(codes, max_occ=5)
    assert int((val == unit_val).sum()) == 0 and len(val) == len(codes) - cmap.K + 1 - 6
    # equal k-mers keep their positions in rising order
    val, pos = cmap.build_index(codes, max_occ=6)
    assert np.all(np.diff(pos[val == unit_val]) > 0)


def test_tie_rules_and_floor_division():
    from chiron_amd import map as cmap
    rng = np.random.default_rng(33)
    plant = assess_ref.random_seq(300, rng)
    flank = [assess_ref.random_seq(n, rng) for n in (5000, 7000, 3000)]
    text = flank[0] + plant + flank[1] + plant + flank[2]
    g = _genome([("one", text)])
    index = cmap.build_index(g.codes)
    v = cmap.vote(index, assess_ref_encode(plant))
    assert v["strand"] == "forward" and v["delta"] == 5000                       # two identical copies: the smaller position
    assert v["votes"] == 300 - cmap.K + 1 and v["votes_second"] == v["votes"]
    # a palindromic plant (its own reverse complement): both strands score alike, forward wins
    half = assess_ref.random_seq(150, rng)
    pal = half + map_ref.revcomp(half)
    g2 = _genome([("one", flank[0] + pal + flank[2])])
    v = cmap.vote(cmap.build_index(g2.codes), assess_ref_encode(pal))
    assert v["strand"] == "forward" and v["delta"] == 5000 and v["votes_second"] == v["votes"]
    # the reverse strand is found when that is where the read lies
    v = cmap.vote(index, assess_ref_encode(map_ref.revcomp(flank[1][1000:1400])))
    assert v["strand"] == "reverse" and v["delta"] == 5300 + 1000
    # negative diagonals: a read that hangs over the genome's start by 300 bases has delta = -300, which floors into bin -2
    bins, score = cmap.bin_scores(np.array([-300, -300, -1, 0, 255, 256], dtype=np.int64))
    assert bins.tolist() == [-2, -1, 0, 1] and score.tolist() == [3, 3, 3, 1]
    over = assess_ref.random_seq(300, rng) + text[:400]
    v = cmap.vote(index, assess_ref_encode(over))
    assert v["delta"] == -300 and v["votes"] == 400 - cmap.K + 1
    lo, hi = cmap.window_of(g, 0, v["delta"], len(over), 256)
    assert (lo, hi) == (0, 700 - 300 + 256)


def test_writers_round_trip_through_load_references(tmp_path):
    from chiron_amd import assess, map as cmap
    rng = np.random.default_rng(34)
    contigs = [("c1", assess_ref.random_seq(4000, rng)), ("c2", assess_ref.random_seq(3000, rng))]
    g = _genome(contigs)
    reads = {"fwd": assess_ref.mutate(contigs[0][1][1000:1600], 0.05, rng),
             "rev": map_ref.revcomp(assess_ref.mutate(contigs[1][1][500:1200], 0.05, rng)),
             "junk": assess_ref.random_seq(500, rng)}
    aligner = lambda rs, ws, band0: map_ref.infix_rows(rs, ws, band0, cmap.INFIX_DTYPE)
    res = cmap.map_reads(reads, g, aligner=aligner)
    by = {r["name"]: r for r in res["reads"]}
    assert [by[k]["status"] for k in ("fwd", "rev", "junk")] == ["mapped", "mapped", "unmapped"] and res["unmapped"] == ["junk"]
    assert (by["fwd"]["contig"], by["fwd"]["strand"]) == ("c1", "forward") and (by["rev"]["contig"], by["rev"]["strand"]) == ("c2", "reverse")
    assert abs(by["fwd"]["start"] - 1000) < 10 and abs(by["fwd"]["end"] - 1600) < 10
    assert abs(by["rev"]["start"] - 500) < 10 and abs(by["rev"]["end"] - 1200) < 10
    report = cmap.write_outputs(str(tmp_path), res, g, {"genome": "x"})
    assert report["totals"]["mapped"] == 2 and report["totals"]["unmapped"] == 1 and report["totals"]["edge"] == 0
    refs = assess.load_references(str(tmp_path / "reference"))
    assert set(refs) == {"fwd", "rev"}
    assert refs["fwd"] == contigs[0][1][by["fwd"]["start"]:by["fwd"]["end"]]
    assert refs["rev"] == map_ref.revcomp(contigs[1][1][by["rev"]["start"]:by["rev"]["end"]])
    for name in refs:                      # the cut-out, in the read's orientation, aligns globally at the mapping's (E, M)
        assert assess_ref.full_table(reads[name], refs[name]) == (by[name]["edit"], by[name]["match"])
    paf = [ln.split("\t") for ln in (tmp_path / "mapped.paf").read_text().splitlines()]
    assert len(paf) == 2 and all(len(c) == 12 for c in paf)
    for c in paf:
        r = by[c[0]]
        assert c[1:4] == [str(r["read_len"]), "0", str(r["read_len"])] and c[4] == ("+" if r["strand"] == "forward" else "-")
        assert c[5] == r["contig"] and int(c[6]) == len(dict(contigs)[r["contig"]]) and (int(c[7]), int(c[8])) == (r["start"], r["end"])
        assert int(c[9]) == r["match"] and int(c[10]) == r["match"] + r["mismatch"] + r["insertion"] + r["deletion"] and c[11] == "255"


def test_end_to_end_seed_leaves_the_unrelated_reads_below_min_votes():
    """What test_gpu_map.py's end-to-end case relies on, from the host-side voting alone."""
    from chiron_amd import map as cmap
    contigs, reads, truth = map_ref.planted_case(E2E_SEED)
    g = _genome(contigs)
    index = cmap.build_index(g.codes)
    for name, seq in reads.items():
        v = cmap.vote(index, assess_ref_encode(seq))
        if name.startswith("noise"):
            assert v["votes"] < cmap.MIN_VOTES, (name, v)
        else:
            assert v["votes"] >= cmap.MIN_VOTES and v["strand"] == truth[name][3], (name, v)
            assert g.names[g.contig_of(v["g"])] == truth[name][0]


def test_abi_sizes_and_argument_errors(built):
    from chiron_amd import _lib, map as cmap
    lib = _lib.load()
    n = C.c_size_t()
    assert lib.chiron_align_infix_workspace_size(0, 0, 0, C.byref(n)) == _lib.OK
    # a table that fits LDS needs no rows; one diagonal more needs a row per workgroup
    fits = cmap.workspace_size(3, 1000, cmap.LDS_SLOTS - 1001)
    over = cmap.workspace_size(3, 1000, cmap.LDS_SLOTS - 1000)
    assert over - fits >= 3 * (cmap.LDS_SLOTS + 1) * 8 and fits >= 3 * (cmap.LDS_SLOTS - 1) + 3 * 16 + 3 * 20
    many = cmap.workspace_size(5000, 1000, cmap.LDS_SLOTS)
    assert many - cmap.workspace_size(5000, 1000, cmap.LDS_SLOTS - 1001) < (_lib.INFIX_MAX_GROUPS + 1) * (cmap.LDS_SLOTS + 1002) * 8 + 5000 * 1001 + 256
    assert lib.chiron_align_infix_workspace_size(1, cmap.MAX_READ, cmap.MAX_WINDOW, C.byref(n)) == _lib.OK
    for args in ((1, cmap.MAX_READ + 1, 10), (1, 10, cmap.MAX_WINDOW + 1), ((1 << 24) + 1, 10, 10)):
        assert lib.chiron_align_infix_workspace_size(*args, C.byref(n)) == _lib.ERR_OVERFLOW, args
    for args in ((-1, 1, 1), (1, -1, 1), (1, 1, -1)):
        assert lib.chiron_align_infix_workspace_size(*args, C.byref(n)) == _lib.ERR_INVALID, args
    assert lib.chiron_align_infix_workspace_size(1, 1, 1, None) == _lib.ERR_INVALID

    codes = np.array([0, 1, 2, 3, 4, 0, 1, 2], dtype=np.uint8)
    out = [np.zeros(2, np.int32) for _ in range(5)]

    def call(codes, read_off, win_off, pairs=2, band0=256, flags=0, ws=1):
        ro, wo = np.asarray(read_off, np.int64), np.asarray(win_off, np.int64)
        return lib.chiron_align_infix(0, codes.ctypes.data if codes is not None else None, ro.ctypes.data, wo.ctypes.data, pairs, band0,
                                      flags, *[o.ctypes.data for o in out], C.c_void_p(ws), None)

    assert call(codes, [0, 2, 4], [4, 6, 8], pairs=0) == _lib.OK                       # a no-op, before anything is looked at
    assert call(codes, [0, 2, 4], [4, 6, 8], band0=-1) == _lib.ERR_INVALID and b"band0" in lib.chiron_last_error()
    assert call(codes, [0, 2, 4], [4, 6, 8], flags=1) == _lib.ERR_INVALID
    assert call(codes, [0, 2, 4], [4, 6, 8], pairs=-1) == _lib.ERR_INVALID
    assert call(codes, [0, 2, 1], [4, 6, 8]) == _lib.ERR_INVALID and b"predecessor" in lib.chiron_last_error()
    assert call(codes, [-1, 2, 4], [4, 6, 8]) == _lib.ERR_INVALID
    assert call(codes, [0, 2, 4], [4, 3, 8]) == _lib.ERR_INVALID
    bad = codes.copy()
    bad[5] = 5
    assert call(bad, [0, 2, 4], [4, 6, 8]) == _lib.ERR_INVALID and b"outside 0..4" in lib.chiron_last_error()
    assert call(None, [0, 2, 4], [4, 6, 8]) == _lib.ERR_INVALID
    assert call(codes, [0, 2, 4], [4, 6, 8], ws=0) == _lib.ERR_INVALID and b"workspace" in lib.chiron_last_error()
    # lengths past the limits: refused from the offsets alone, before a code is read
    assert call(codes, [0, cmap.MAX_READ + 1, cmap.MAX_READ + 1], [0, 1, 2]) == _lib.ERR_OVERFLOW
    assert call(codes, [0, 1, 2], [0, cmap.MAX_WINDOW + 1, cmap.MAX_WINDOW + 1]) == _lib.ERR_OVERFLOW
    with pytest.raises(_lib.ChironError) as ei:
        cmap.workspace_size(1, cmap.MAX_READ + 1, 5)
    assert ei.value.status == _lib.ERR_OVERFLOW
    assert (cmap.THREADS, cmap.LDS_SLOTS, cmap.BAND0) == (256, 4096, 256)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "chiron_amd.h")).read()
    for name, value in (("MAX_READ", "(1 << 17)"), ("MAX_WINDOW", "((1 << 20) - 1)"), ("BAND0", "256"), ("THREADS", "256"),
                        ("LDS_SLOTS", "4096"), ("MAX_GROUPS", "2048")):
        assert "#define CHIRON_INFIX_%s %s" % (name, value) in header and getattr(_lib, "INFIX_" + name) == eval(value)
