"""CPU: modcall without a GPU -- the three restatements of chiron_signal_score's definition (tests/site_ref.py) against each other,
the brute force included; the refusals of the two entry points and the calls that need no device; the host walk under a sanitizer;
the host rules of chiron_amd.modcall (sites, groups, windows, rows, segments, planner, files, command line); and the planted case
of tests/modcall_cases.py, scored by the reference alone."""
import argparse
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import modcall_cases as cases
import refine_ref
import site_ref as ref
import squiggle_cases
from chiron_amd import _lib, modcall, squiggle
from test_weight_pack_cpu import rocm_prefix

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ----------------------------------------------------------------------------------------------------------------------------
# the references
# ----------------------------------------------------------------------------------------------------------------------------
def test_reference_against_brute_force():
    """Every path enumerated for S <= 7 and L <= 5: the recurrence in plain Python and the numpy rows give the brute force's cost.
    Both sample ranges, few values so that ties occur, S = L, S = L - 1 and S = 0."""
    rng = np.random.default_rng(5000)
    seen, feasible, infeasible = set(), 0, 0
    for n in range(1500):
        x, e = cases.small_case(rng)
        want = ref.brute_item(x, e)
        assert ref.score_item(x, e) == want and ref.score_item_numpy(x, e) == want, (n, x, e, want)
        S, L = len(x), len(e)
        seen |= {"S=0"} if S == 0 else set()
        seen |= {"S=L"} if S == L else set()
        seen |= {"S=L-1"} if S == L - 1 else set()
        seen |= {"L=1"} if L == 1 else set()
        seen |= {"tie"} if ref.brute_paths(x, e).count(want) > 1 else set()              # several paths attain the minimum
        feasible, infeasible = feasible + (want != ref.INFEASIBLE), infeasible + (want == ref.INFEASIBLE)
        assert (want == ref.INFEASIBLE) == (S < L)
    print("brute force: %d feasible, %d infeasible" % (feasible, infeasible))
    assert seen == {"S=0", "S=L", "S=L-1", "L=1", "tie"} and feasible > 500 and infeasible > 200


def test_reference_formulations_agree():
    """The plain-Python recurrence against the numpy rows on calls of the GPU tests' kind, the fixed cases among them."""
    rng = np.random.default_rng(5001)
    segments, candidates = cases.random_call(rng, 12, 80, max_samples=60)
    segments += [np.zeros(0, np.int16), np.full(40, -32768, np.int16), np.full(3, 7, np.int16)]
    n = len(segments)
    candidates += [(n - 3, np.array([5], np.int32)),                                   # S = 0
                   (n - 2, np.full(16, 32767, np.int32)), (n - 2, np.array([32767], np.int32)),                # the extreme values
                   (n - 1, np.array([7, 7, 7], np.int32)), (n - 1, np.array([7, 7, 7, 7], np.int32)),          # S = L, S = L - 1
                   (n - 1, np.array([7, 3], np.int32)), (n - 1, np.array([3, 7], np.int32))]                   # one sample on the level 3, either way round
    got, plain = ref.score(segments, candidates), ref.score_plain(segments, candidates)
    assert got.dtype == np.int32 and np.array_equal(got, plain)
    assert got[-7:].tolist() == [ref.INFEASIBLE, 40 * 65535, 40 * 65535, 0, ref.INFEASIBLE, 4, 4]
    assert (got == ref.INFEASIBLE).sum() > 5 and (got != ref.INFEASIBLE).sum() > 40
    assert ref.INFEASIBLE == modcall.INFEASIBLE == (1 << 31) - 1 and (ref.MAX_SAMPLES, ref.MAX_COLUMNS) == (modcall.MAX_SAMPLES, modcall.MAX_COLUMNS)
    assert ref.score([], []).shape == (0,)


# ----------------------------------------------------------------------------------------------------------------------------
# the entry points without a device
# ----------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_limits_are_bound(built):
    lib = _lib.load()
    names = {n for n, _, _ in _lib.SYMBOLS}
    assert {"chiron_signal_score_workspace_size", "chiron_signal_score"} <= names and hasattr(lib, "chiron_signal_score")
    header = open(os.path.join(ROOT, "include", "chiron_amd.h")).read()
    INT32_MAX = (1 << 31) - 1  # noqa: F841  the header's word for INFEASIBLE
    for name in ("MAX_SAMPLES", "MAX_COLUMNS", "INFEASIBLE", "THREADS", "MAX_GROUPS"):
        text = header.split("#define CHIRON_SITE_%s " % name)[1].split("\n")[0].split("/*")[0].strip()
        assert eval(text) == getattr(_lib, "SITE_" + name), name
    assert lib.chiron_abi_version() == 7
    assert _lib.SITE_MAX_SAMPLES * 65535 < 1 << 30 and (1 << 30) + _lib.SITE_MAX_SAMPLES * 65535 < 1 << 31
    assert (modcall.THREADS, modcall.MAX_GROUPS, modcall.MAX_COLUMNS) == (256, 2048, 16)


def test_workspace_size_rules(built):
    """The header's sentence: each part rounded up to 256 bytes -- the segment offsets (8 bytes a segment + 8), the samples (2 bytes
    a sample + 16), the level offsets (8 bytes a candidate + 8), 4 bytes a level, 4 bytes a candidate of segment indices and 4 bytes a
    candidate of costs."""
    lib = _lib.load()
    up = lambda v: (v + 255) // 256 * 256
    want = lambda g, s, c, n: up(8 * g + 8) + up(2 * s + 16) + up(8 * c + 8) + up(4 * n) + 2 * up(4 * c)
    for args in ((3, 1000, 6, 60), (0, 0, 0, 0), (1, 0, 1, 1), (31, 120, 31, 64), (32, 121, 64, 1024), (1000, 1000, 524289, 524289)):
        assert modcall.score_workspace_size(*args) == want(*args), args
    assert modcall.score_workspace_size(1, 121, 0, 0) == modcall.score_workspace_size(1, 120, 0, 0) + 256      # the pad: 2 * 120 + 16 = 256
    n = C.c_size_t()
    for k in range(4):
        args = [1, 1, 1, 1]
        args[k] = -1
        assert lib.chiron_signal_score_workspace_size(*args, C.byref(n)) == _lib.ERR_INVALID and b"negative" in lib.chiron_last_error()
    assert lib.chiron_signal_score_workspace_size(1, 1, 1, 1, None) == _lib.ERR_INVALID and b"null bytes" in lib.chiron_last_error()
    for args, word in (((1 << 31, 1, 1, 1), "segments"), ((1, _lib.SIGNAL_MAX_SAMPLES + 1, 1, 1), "samples"), ((1, 1, 1 << 31, 1), "candidates"),
                       ((1, 1, 1, 1 << 31), "levels")):
        with pytest.raises(_lib.ChironError) as ei:
            modcall.score_workspace_size(*args)
        assert ei.value.status == _lib.ERR_OVERFLOW and word in str(ei.value), args
    top = ((1 << 31) - 1, _lib.SIGNAL_MAX_SAMPLES, (1 << 31) - 1, (1 << 31) - 1)
    assert modcall.score_workspace_size(*top) == want(*top)
    # monotone in every argument: what the planner's bisection rests on
    base = modcall.score_workspace_size(5, 5000, 10, 100)
    assert all(modcall.score_workspace_size(5 + 70 * a, 5000 + 300 * b, 10 + 70 * c, 100 + 70 * d) > base
               for a, b, c, d in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)))


def _call(lib, samples=(1, 2, 3, 4, 5, 6), sample_off=(0, 4, 6), segments=2, level=(10, -10, 0, 5), level_off=(0, 2, 3, 4), seg=(0, 1, 0), candidates=3,
          flags=0, cost=True, ws=0, ws_bytes=1 << 20):
    """Two segments of 4 and 2 samples; three candidates of 2, 1 and 1 levels on segments 0, 1, 0.  With ws = 0 a call that passes
    every check ends at the null workspace."""
    arr = lambda v, t: None if v is None else np.ascontiguousarray(np.asarray(v, dtype=t))
    a = [arr(samples, np.int16), arr(sample_off, np.int64), arr(level, np.int32), arr(level_off, np.int64), arr(seg, np.int32)]
    c = np.full(8, 77, np.int32)                 # a refused call writes nothing, whatever it was promised
    p = [None if x is None else x.ctypes.data for x in a]
    st = lib.chiron_signal_score(0, p[0], p[1], segments, p[2], p[3], p[4], candidates, c.ctypes.data if cost else None, ws, ws_bytes, flags, None)
    return st, lib.chiron_last_error().decode(), c


def test_every_refusal_comes_before_a_device(built):
    lib = _lib.load()
    INVALID, OVERFLOW = _lib.ERR_INVALID, _lib.ERR_OVERFLOW
    st, msg, c = _call(lib)
    assert st == INVALID and "chiron_signal_score: null workspace" in msg             # everything else passed: the last check but one
    assert (c == 77).all()
    host = np.zeros(1 << 12, np.uint8)                                                 # a workspace that is too small is refused before its memory is looked at
    need = modcall.score_workspace_size(2, 6, 3, 4)
    st, msg, c = _call(lib, ws=host.ctypes.data, ws_bytes=need - 1)
    assert st == INVALID and "a workspace of %d bytes, %d are needed" % (need - 1, need) in msg and (c == 77).all()
    for kw, status, text in (
            (dict(flags=4), INVALID, "unknown flags 0x4"),
            (dict(candidates=-1), INVALID, "negative size"),
            (dict(segments=-1), INVALID, "negative size"),
            (dict(candidates=1 << 31), OVERFLOW, "candidates in one call"),
            (dict(segments=1 << 31), OVERFLOW, "segments in one call"),
            (dict(level=None), INVALID, "null level / level_off / seg"),
            (dict(level_off=None), INVALID, "null level / level_off / seg"),
            (dict(seg=None), INVALID, "null level / level_off / seg"),
            (dict(cost=False), INVALID, "null cost_out"),
            (dict(sample_off=None), INVALID, "null sample_off"),
            (dict(samples=None), INVALID, "null samples"),
            (dict(sample_off=(-1, 4, 6)), INVALID, "sample_off[0] = -1 is negative"),
            (dict(sample_off=(0, 4, 3)), INVALID, "sample_off[2] = 3 below its predecessor 4"),
            (dict(sample_off=(0, 4, 4 + 4097)), INVALID, "segment 1 has 4097 samples, at most 4096"),
            (dict(sample_off=(0, 4097, 4098)), INVALID, "segment 0 has 4097 samples, at most 4096"),
            (dict(level_off=(-2, 2, 3, 4)), INVALID, "level_off[0] = -2 is negative"),
            (dict(level_off=(0, 2, 1, 4)), INVALID, "level_off[2] = 1 below its predecessor 2"),
            (dict(level_off=(0, 2, 2, 4)), INVALID, "candidate 1 has 0 levels, 1..16 are allowed"),
            (dict(level_off=(0, 2, 3, 20)), INVALID, "candidate 2 has 17 levels, 1..16 are allowed"),
            (dict(seg=(0, 2, 0)), INVALID, "seg[1] = 2 outside 0..1"),
            (dict(seg=(0, 1, -1)), INVALID, "seg[2] = -1 outside 0..1"),
            (dict(segments=0), INVALID, "seg[0] = 0 outside 0..-1"),
            (dict(level=(10, 32768, 0, 5)), INVALID, "level 32768 of column 1 of candidate 0 outside -32767..32767"),
            (dict(level=(10, -10, 0, -32768)), INVALID, "level -32768 of column 0 of candidate 2 outside -32767..32767"),
            (dict(level=(10, -10, squiggle.UNKNOWN, 5)), INVALID, "level -2147483648 of column 0 of candidate 1 outside -32767..32767")):
        st, msg, c = _call(lib, **kw)
        assert st == status and text in msg and msg.startswith("chiron_signal_score: "), (kw, st, msg)
        assert (c == 77).all(), kw
    # what is legal: the extreme levels, an empty segment, a segment nobody names, sixteen levels; each ends at the workspace check
    for kw in (dict(level=(32767, -32767, 0, 5)), dict(sample_off=(0, 0, 6)), dict(seg=(0, 0, 0)), dict(sample_off=(3, 4, 4100), samples=np.zeros(4100)),
               dict(level=np.zeros(18), level_off=(0, 16, 17, 18))):
        st, msg, _ = _call(lib, **kw)
        assert st == INVALID and "null workspace" in msg, (kw, msg)


def test_calls_that_need_no_device(built):
    lib = _lib.load()
    st, _, c = _call(lib, candidates=0)
    assert st == _lib.OK and (c == 77).all()                                           # no candidate: nothing is written
    st, _, c = _call(lib, candidates=0, level=None, level_off=None, seg=None, sample_off=None, samples=None, segments=0, cost=False)
    assert st == _lib.OK
    got = modcall.score_call([], [])
    assert got.shape == (0,) and got.dtype == np.int32
    assert modcall.score_call([np.arange(5)], []).shape == (0,)
    assert modcall.modcall([], squiggle_cases.PlainGenome(np.zeros(10, np.uint8)), (np.zeros(4, np.int32),) * 2, 1, scorer=ref.score)["rows"] == []


def test_host_walk_under_sanitizers(tmp_path):
    """tests/native/site_pack_check.cpp, built with the ROCm host compiler under AddressSanitizer + UndefinedBehaviorSanitizer:
    csrc/site_pack.h on 0, 1, 2, 63, 64, 65, 257 and random numbers of segments and of candidates in buffers of exactly the stated
    size, each kind of fault at the last place it can sit."""
    exe = str(tmp_path / "site_pack_check")
    cmd = [os.path.join(rocm_prefix(), "llvm", "bin", "clang++"), "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", os.path.join(HERE, "native", "site_pack_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "site pack OK" in r.stdout


# ----------------------------------------------------------------------------------------------------------------------------
# the host side
# ----------------------------------------------------------------------------------------------------------------------------
def _revcomp(text):
    return "".join("TGCA"["ACGT".index(c)] if c in "ACGT" else "N" for c in reversed(text))


def _genome_of(text):
    return squiggle_cases.PlainGenome(np.array(["ACGTN".index(c) for c in text], dtype=np.uint8))


def test_motif_sites_against_a_walk_of_both_strands():
    rng = np.random.default_rng(5002)
    text = "".join("ACGT"[v] for v in rng.integers(0, 4, 500))
    text = text[:100] + "N" + text[101:250] + "CGCGACGGATC" + text[261:]
    genome = _genome_of(text)
    rc = _revcomp(text)
    n = len(text)
    for motif, offset in (("CG", 0), ("CG", 1), ("GATC", 1), ("CAG", 1), ("A", 0), ("ACG", 2)):
        fwd, rev = modcall.motif_sites(genome, motif, offset)
        want_f = [p + offset for p in range(n) if text.startswith(motif, p)]
        want_r = sorted(n - 1 - (p + offset) for p in range(n) if rc.startswith(motif, p))
        assert fwd.tolist() == want_f and rev.tolist() == want_r, motif
        assert len(want_f) > 0 and len(want_r) > 0
    fwd, rev = modcall.motif_sites(genome)                                             # the defaults: CG, its C
    assert np.array_equal(rev, fwd + 1)                                                # a palindrome: the same occurrences, the C of the other strand
    f2, r2 = modcall.motif_sites(genome, "ACG", 2)
    assert set(f2.tolist()) <= set((fwd + 1).tolist()) and not np.array_equal(r2, f2)
    for bad in (("", 0), ("CN", 0), ("cg", 0), ("CG", 2), ("CG", -1)):
        with pytest.raises(ValueError):
            modcall.motif_sites(genome, *bad)
    assert modcall.motif_sites(_genome_of("A"))[0].shape == (0,)


def test_grouping_at_gaps_of_k_minus_1_and_k():
    assert modcall.site_groups([], 5) == []
    assert modcall.site_groups([7], 5) == [(0, 1)]
    occ = [10, 14, 19, 23, 27, 40, 45, 49]                                             # gaps 4 5 4 4 13 5 4
    assert modcall.site_groups(occ, 5) == [(0, 2), (2, 5), (5, 6), (6, 8)]
    assert modcall.site_groups(occ, 6) == [(0, 5), (5, 8)] and modcall.site_groups(occ, 4) == [(k, k + 1) for k in range(8)]
    text = "A" * 10 + "CG" + "AA" + "CG" + "AAA" + "CG" + "A" * 10                      # CG at 10, 14 (gap 4) and 19 (gap 5)
    groups = modcall.strand_groups(_genome_of(text), 5)
    assert [g["sites"] for g in groups[0]] == [(10, 14), (19,)] and [g["sites"] for g in groups[1]] == [(11, 15), (20,)]
    assert [g["occurrences"].tolist() for g in groups[1]] == [[10, 14], [19]]
    # the window: 9 positions for one site at k = 5 and flank 2, mirrored on the reverse strand for an even k
    assert modcall.group_window(19, 19, False, 5, 2) == (15, 24) and modcall.group_window(20, 20, True, 5, 2) == (16, 25)
    assert modcall.group_window(10, 14, False, 5, 2) == (6, 19) and modcall.group_window(10, 14, False, 5, 0) == (8, 17)
    assert modcall.group_window(30, 30, False, 6, 1) == (26, 34) and modcall.group_window(30, 30, True, 6, 1) == (27, 35)


def _walk_rows(read, genome, g0, g1, k, occurrences, motif_len, table, alt):
    """The window's rows by a per-base walk of squiggle.kmer_bins on a read that matches the genome over the window."""
    bins = squiggle.kmer_bins(read, genome, k)
    g, idx = squiggle._columns(read)
    order = range(g1 - 1, g0 - 1, -1) if read["reverse"] else range(g0, g1)
    h = k // 2
    row0, row1 = [], []
    for q in order:
        code = int(bins[idx[np.flatnonzero(g == q)[0]]])
        lo = q - (k - 1 - h if read["reverse"] else h)
        whole = any(lo <= a and a + motif_len <= lo + k for a in occurrences)
        row0.append(squiggle.UNKNOWN if code < 0 else int(table[code]))
        row1.append(squiggle.UNKNOWN if code < 0 else int(alt[code] if whole else table[code]))
    return row0, row1


def test_window_rows_against_a_walk_of_kmer_bins():
    rng = np.random.default_rng(5003)
    codes = rng.integers(0, 4, 300).astype(np.uint8)
    codes[150] = 4
    genome = squiggle_cases.PlainGenome(codes)
    took_alt = unknown = 0
    for k in (3, 4, 5, 6):
        table, alt = rng.integers(-3000, 3000, 4 ** k).astype(np.int32), rng.integers(-3000, 3000, 4 ** k).astype(np.int32)
        alt[rng.random(4 ** k) < 0.05] = squiggle.UNKNOWN
        for motif in ("CG", "GAT"):
            for reverse, groups in enumerate(modcall.strand_groups(genome, k, motif, 0)):
                read = {"pos": 0, "ops": np.zeros(300, np.uint8), "reverse": bool(reverse), "lead": 0, "called": np.zeros(300, np.uint8)}
                for grp in groups:
                    for flank in (0, 2):
                        g0, g1 = modcall.group_window(grp["sites"][0], grp["sites"][-1], bool(reverse), k, flank)
                        if g0 < 0 or g1 > 300:
                            continue
                        row0, row1 = modcall.window_rows(genome, g0, g1, bool(reverse), k, grp["occurrences"], len(motif), table, alt)
                        want0, want1 = _walk_rows(read, genome, g0, g1, k, grp["occurrences"], len(motif), table, alt)
                        assert row0.dtype == row1.dtype == np.int32 and row0.tolist() == want0 and row1.tolist() == want1, (k, motif, reverse, grp["sites"])
                        took_alt += int((row0 != row1).sum())
                        unknown += int((row1 == squiggle.UNKNOWN).sum())
                        # the k-mers that hold the group's first occurrence whole are k - len(motif) + 1 consecutive bases inside the window
                        assert len(row0) == grp["sites"][-1] - grp["sites"][0] + k + 2 * flank
    assert took_alt > 500 and unknown > 10
    # by hand: AACGTT.., k = 3, forward; the 3-mers ACG and CGT hold the CG whole, AAC and GTT do not
    g = _genome_of("AAACGTTT")
    table, alt = np.arange(64, dtype=np.int32), 1000 + np.arange(64, dtype=np.int32)
    row0, row1 = modcall.window_rows(g, 1, 7, False, 3, [3], 2, table, alt)
    assert row0.tolist() == [0, 1, 6, 27, 47, 63] and row1.tolist() == [0, 1, 1006, 1027, 47, 63]
    row0, row1 = modcall.window_rows(g, 1, 7, True, 3, [3], 2, table, alt)               # AAACGT: the same k-mers read from the other end
    assert row0.tolist() == [0, 1, 6, 27, 47, 63] and row1.tolist() == [0, 1, 1006, 1027, 47, 63]


def _read_on(genome_len, pos, ops, reverse, rng, lead=0):
    ops = np.asarray(ops, dtype=np.uint8)
    n = lead + int((ops != 3).sum())
    starts = np.concatenate([[0], np.cumsum(rng.integers(3, 9, n))]).astype(np.int32) + 5
    return {"name": "r", "pos": pos, "ops": ops, "reverse": reverse, "lead": lead, "called": rng.integers(0, 4, n).astype(np.uint8),
            "starts": starts, "signal": rng.integers(-3000, 3000, int(starts[-1])).astype(np.int16)}


def test_segments_with_indels_and_the_drops():
    """One CG at 50 in a genome without another: the window is 46 .. 54.  The segment runs from the first sample of the read base on
    the window's first position to the last sample of the one on its last, whatever lies between; an end in a deletion drops the
    group, and so do the other reasons."""
    rng = np.random.default_rng(5004)
    text = list("".join("AT"[v] for v in rng.integers(0, 2, 120)))
    text[50:52] = "CG"
    genome = _genome_of("".join(text))
    table = rng.integers(-3000, 3000, 4 ** 5).astype(np.int32)
    alt = table + 500
    groups = modcall.strand_groups(genome, 5)
    assert [g["sites"] for g in groups[0]] == [(50,)] and [g["sites"] for g in groups[1]] == [(51,)]
    M, X, I, D = 0, 1, 2, 3
    plain = [M] * 100
    inside = [M] * 38 + [I, I] + [M] * 2 + [D] + [X] + [M] * 57                          # from 10: an insertion before 48, 50 deleted, 51 a mismatch
    for reverse in (False, True):
        g0, g1 = (46, 55) if not reverse else (47, 56)
        for ops, lead in ((plain, 0), (inside, 3)):
            read = _read_on(120, 10, ops, reverse, rng, lead)
            kept, drops = modcall.read_candidates(read, genome, groups[int(reverse)], (table, alt), 5, 2)
            assert not any(drops.values()) and len(kept) == 1
            g, idx = squiggle._columns(read)
            first, last = (g1 - 1, g0) if reverse else (g0, g1 - 1)
            a, b = int(idx[g == first][0]), int(idx[g == last][0])
            assert a < b and (kept[0]["s0"], kept[0]["s1"]) == (int(read["starts"][a]), int(read["starts"][b + 1]))
            assert b - a + 1 == 9 + (ops is inside)                                      # two inserted bases more, one deleted base fewer
            want0, want1 = modcall.window_rows(genome, g0, g1, reverse, 5, [50], 2, table, alt)
            assert np.array_equal(kept[0]["row0"], want0) and np.array_equal(kept[0]["row1"], want1) and len(want0) == 9
            assert (want1 - want0).tolist() == [0, 0, 0, 500, 500, 500, 500, 0, 0]             # the four 5-mers that hold the CG whole
        # an end of the window in a deletion: the first position, then the last
        for at in (g0, g1 - 1):
            ops = [M] * (at - 10) + [D] + [M] * (99 - (at - 10))
            kept, drops = modcall.read_candidates(_read_on(120, 10, ops, reverse, rng), genome, groups[int(reverse)], (table, alt), 5, 2)
            assert kept == [] and drops["end_unaligned"] == 1 and sum(drops.values()) == 1
        # the window leaves the aligned stretch on either side; a read that does not reach the site does not see the group
        for pos, n, seen in ((g0 + 1, 60, 1), (g0, 60, 0), (0, g1 - 1, 1), (0, g1, 0), (60, 50, None), (0, 40, None)):
            kept, drops = modcall.read_candidates(_read_on(120, pos, [M] * n, reverse, rng), genome, groups[int(reverse)], (table, alt), 5, 2)
            assert drops["window_off_read"] == (seen or 0) and len(kept) == (1 if seen == 0 else 0) and sum(drops.values()) == (seen or 0), (pos, n)
        # a 5-mer without a level in either table
        for which in (0, 1):
            t = [table.copy(), alt.copy()]
            code = int(modcall.window_codes(genome, g0, g1, reverse, 5)[4])              # the middle base: it takes the alternative level
            t[which][code] = squiggle.UNKNOWN
            kept, drops = modcall.read_candidates(_read_on(120, 10, plain, reverse, rng), genome, groups[int(reverse)], tuple(t), 5, 2)
            assert kept == [] and drops["unknown_level"] == 1
        # flank 4 makes the window 13 wide, flank 6 makes it 17: too wide
        assert len(modcall.read_candidates(_read_on(120, 10, plain, reverse, rng), genome, groups[int(reverse)], (table, alt), 5, 2, 4)[0][0]["row0"]) == 13
        assert modcall.read_candidates(_read_on(120, 10, plain, reverse, rng), genome, groups[int(reverse)], (table, alt), 5, 2, 6)[1]["too_wide"] == 1
    # above 4096 samples: too long
    read = _read_on(120, 10, plain, False, rng)
    read["starts"] = (np.asarray(read["starts"], dtype=np.int64) * 200).astype(np.int32)     # at least 9 * 600 samples
    read["signal"] = np.zeros(int(read["starts"][-1]), np.int16)
    assert modcall.read_candidates(read, genome, groups[0], (table, alt), 5, 2)[1]["too_long"] == 1
    # fewer samples than columns: infeasible, counted after the scorer has said so
    read = _read_on(120, 10, plain, False, rng)
    read["starts"] = np.minimum(read["starts"], read["starts"][37]).astype(np.int32)     # bases 37 .. have no sample: 3 to 8 samples for 9 columns
    got = modcall.modcall([read], genome, (table, alt), 5, scorer=ref.score)
    assert got["rows"] == [] and got["groups"] == {"seen": 1, "scored": 0, "dropped": {**dict.fromkeys(modcall.GROUP_DROPS, 0), "infeasible": 1}}


def _random_reads(rng, genome_len, count):
    reads = []
    for n in range(count):
        r = squiggle_cases.random_read(rng, genome_len, name="r%d" % n, columns=int(rng.integers(60, 200)))
        r["starts"] = (int(rng.integers(0, 30)) + np.concatenate([[0], np.cumsum(rng.integers(1, 20, len(r["called"])))])).astype(np.int32)
        r["signal"] = rng.integers(-3000, 3000, int(r["starts"][-1]) + 5).astype(np.int16)
        reads.append(r)
    return reads


def test_planning_and_batching_give_the_same_rows(built):
    rng = np.random.default_rng(5005)
    genome = squiggle_cases.PlainGenome(rng.integers(0, 4, 600))
    table, alt = rng.integers(-3000, 3000, 4 ** 5).astype(np.int32), rng.integers(-3000, 3000, 4 ** 5).astype(np.int32)
    reads = _random_reads(rng, 600, 40)
    calls = []

    def scorer(segments, candidates):
        calls.append((len(segments), sum(len(s) for s in segments), len(candidates), sum(len(e) for _, e in candidates)))
        assert all(candidates[2 * n][0] == candidates[2 * n + 1][0] == n for n in range(len(segments))) and len(candidates) == 2 * len(segments)
        return ref.score(segments, candidates)
    one = modcall.modcall(reads, genome, (table, alt), 5, scorer=scorer)
    assert one["batches"] == len(calls) == 1 and one["groups"]["scored"] == len(one["rows"]) > 60
    assert one["groups"]["seen"] == one["groups"]["scored"] + sum(one["groups"]["dropped"].values()) and sum(one["calls"].values()) == len(one["rows"])
    assert one["groups"]["dropped"]["end_unaligned"] > 0 and one["groups"]["dropped"]["window_off_read"] > 0
    whole = calls[0]
    assert whole[0] == len(one["rows"]) + one["groups"]["dropped"]["infeasible"]
    for row in one["rows"]:
        assert row["delta"] == (row["c0"] - row["c1"]) / row["samples"] and row["call"] == modcall.call_of(row["delta"]) and row["columns"] <= 16
    budget = modcall.score_workspace_size(whole[0] // 6, whole[1] // 6, whole[2] // 6, whole[3] // 6)
    del calls[:]
    many = modcall.modcall(reads, genome, (table, alt), 5, workspace_mb=budget / (1 << 20), scorer=scorer)
    assert many["batches"] == len(calls) >= 4 and all(modcall.score_workspace_size(*c) <= budget for c in calls)
    assert tuple(np.sum(calls, axis=0).tolist()) == whole
    assert dict(many, batches=1) == one
    runs = modcall.plan_score_batches([(5, 700, 10, 90)] * 10, modcall.score_workspace_size(15, 2100, 30, 270))
    assert runs == [(0, 3), (3, 6), (6, 9), (9, 10)]
    assert modcall.plan_score_batches([(5, 700, 10, 90)] * 3, 1) == [(0, 1), (1, 2), (2, 3)]      # a read that alone exceeds the budget
    # the thresholds
    assert [modcall.call_of(d) for d in (8.0, 7.99, 0.0, -7.99, -8.0)] == ["modified", "ambiguous", "ambiguous", "ambiguous", "canonical"]
    assert modcall.call_of(3.0, 2.5) == "modified" and modcall.MIN_DELTA == 8.0 and modcall.FLANK == 2
    with pytest.raises(ValueError):
        modcall.modcall(reads, genome, (table, alt[:-1]), 5, scorer=scorer)


def test_the_command_line_and_the_files(tmp_path):
    from chiron_amd import entry
    base = ["modcall", "-i", "m", "-s", "c", "-g", "g.fa", "--table", "a.tsv", "--alt-table", "b.tsv", "-o", "out"]
    args = entry.build_parser().parse_args(base)
    assert (args.motif, args.motif_offset, args.flank, args.min_delta, args.table_min_events, args.min_mapq, args.normalize) == ("CG", 0, 2, 8.0, 5, 0, "mad")
    assert (args.segment_len, args.batch_size, args.band, args.max_band, args.workspace_mb) == (400, 1100, 256, 8192, 4096) and args.func is entry.modcall
    args = entry.build_parser().parse_args(base + ["--motif", "GATC", "--motif-offset", "1", "--flank", "1", "--min-delta", "3.5", "--table-min-events", "2",
                                                   "--min-mapq", "20", "--normalize", "none", "-l", "300", "-b", "8", "--band", "0", "--max-band", "64",
                                                   "--workspace-mb", "16"])
    assert (args.motif, args.motif_offset, args.flank, args.min_delta, args.table_min_events, args.min_mapq, args.normalize) == ("GATC", 1, 1, 3.5, 2, 20, "none")
    for missing in ("--table", "--alt-table"):
        argv = list(base)
        del argv[argv.index(missing):argv.index(missing) + 2]
        with pytest.raises(SystemExit):
            entry.build_parser().parse_args(argv)
    sub = [a for a in entry.build_parser()._actions if isinstance(a, argparse._SubParsersAction)][0].choices["modcall"]
    assert "not tuned on real reads" in " ".join(sub.format_help().split())
    # two tables of different k are refused, and so is a file that is no table
    planes = np.zeros((4, 64), dtype=np.int64)
    planes[:, 6] = [9, 80, 9 * 300, 9 * 300 * 300]
    (tmp_path / "k3.tsv").write_text("".join(squiggle.kmer_lines(planes, 3)))
    (tmp_path / "k2.tsv").write_text("".join(squiggle.kmer_lines(planes[:, :16], 2)))
    k, canonical, alternative = modcall.load_tables(str(tmp_path / "k3.tsv"), str(tmp_path / "k3.tsv"))
    assert k == 3 and canonical[6] == 300 and np.array_equal(canonical, alternative)
    with pytest.raises(ValueError) as ei:
        modcall.load_tables(str(tmp_path / "k3.tsv"), str(tmp_path / "k2.tsv"))
    assert "the same k" in str(ei.value)
    # the three files
    genome = _genome_of("A" * 20 + "CG" + "AA" + "CG" + "A" * 20)
    rows = [{"read": "r1", "strand": 0, "group": 0, "sites": (20, 24), "samples": 100, "columns": 13, "c0": 900, "c1": 100, "delta": 8.0, "call": "modified"},
            {"read": "r2", "strand": 0, "group": 0, "sites": (20, 24), "samples": 50, "columns": 13, "c0": 100, "c1": 600, "delta": -10.0, "call": "canonical"},
            {"read": "r3", "strand": 1, "group": 0, "sites": (21, 25), "samples": 64, "columns": 13, "c0": 100, "c1": 132, "delta": -0.5, "call": "ambiguous"}]
    result = {"rows": rows, "groups": {"seen": 4, "scored": 3, "dropped": {**dict.fromkeys(modcall.GROUP_DROPS, 0), "too_wide": 1}},
              "calls": {"modified": 1, "canonical": 1, "ambiguous": 1}, "batches": 1}
    report = modcall.write_outputs(str(tmp_path / "out"), result, genome, {"min_delta": 8.0, "reads": {"total": 3, "used": 3, "dropped": {}}})
    lines = (tmp_path / "out" / "mod_calls.tsv").read_text().splitlines()
    assert lines[0].split("\t") == list(modcall.CALL_COLUMNS) == ["read", "contig", "pos", "sites", "strand", "samples", "columns", "c0", "c1", "delta", "call"]
    assert lines[1:] == ["r1\tctg\t21\t2\t+\t100\t13\t900\t100\t8.0000\tmodified", "r2\tctg\t21\t2\t+\t50\t13\t100\t600\t-10.0000\tcanonical",
                         "r3\tctg\t22\t2\t-\t64\t13\t100\t132\t-0.5000\tambiguous"]
    lines = (tmp_path / "out" / "mod_sites.tsv").read_text().splitlines()
    assert lines[0].split("\t") == list(modcall.SITE_COLUMNS) == ["contig", "pos", "strand", "groups", "modified", "canonical", "ambiguous", "fraction", "mean_delta"]
    assert lines[1:] == ["ctg\t21\t+\t2\t1\t1\t0\t0.5000\t-1.0000", "ctg\t22\t-\t1\t0\t0\t1\tnan\t-0.5000", "ctg\t25\t+\t2\t1\t1\t0\t0.5000\t-1.0000",
                         "ctg\t26\t-\t1\t0\t0\t1\tnan\t-0.5000"]
    saved = json.loads((tmp_path / "out" / "modcall_report.json").read_text())
    assert saved == report and saved["groups"]["dropped"]["too_wide"] == 1 and saved["calls"]["modified"] == 1 and saved["batches"] == 1
    assert saved["sites"] == 4 and saved["files"] == ["mod_calls.tsv", "mod_sites.tsv"] and saved["reads"]["used"] == 3 and saved["min_delta"] == 8.0


# ----------------------------------------------------------------------------------------------------------------------------
# the planted case, on the reference alone
# ----------------------------------------------------------------------------------------------------------------------------
MARGIN = 0.02           # about two standard errors of a share near 0.97 on 300 pairs
# the worst seed's attained value of each share, measured with the numpy reference on the committed case (seeds 1 .. 5)
WORST = {"sign": 0.9811, "sign_sure": 0.9923, "modified_b": 0.0031, "sign_refined": 0.9779, "sign_sure_refined": 0.9922}
_planted = {}


def planted_results(seed):
    """Computed once a seed and shared: the case, its two tables, and modcall's result with the numpy reference as the scorer for
    sample a (jittered borders), for sample b, and for sample a after squiggle.refine with the canonical table (numpy refiner)."""
    if seed not in _planted:
        case = cases.planted(seed)
        tables = cases.tables_of(case)
        out = {"case": case, "tables": tables}
        for name in ("a_jit", "b_jit"):
            kept = cases.prepared(case[name])
            out[name] = modcall.modcall(kept, case["genome"], tables, cases.K, scorer=ref.score)
            if name == "a_jit":
                refined = squiggle.refine(kept, case["genome"], tables[0], cases.K, refiner=refine_ref.refine)
                assert refined["moved"] > 2000
                out["a_refined"] = modcall.modcall(kept, case["genome"], tables, cases.K, scorer=ref.score)
        _planted[seed] = out
    return _planted[seed]


def _pairs_of(reads):
    """(read, group) pairs of a sample by the case's own walk: the groups of the read's strand with a site on the read."""
    return sum(1 for r in reads for sites in r["truth"] if any(r["pos"] <= s < r["pos"] + len(r["called"]) for s in sites))


@pytest.mark.parametrize("seed", cases.SEEDS)
def test_planted_states_are_called(seed):
    """tests/modcall_cases.py at seeds 1 .. 5, the numpy reference as the scorer, default flank and min_delta.  Sample a, every (read,
    group) modified with probability 1/2: the sign of delta names the truth in at least WORST - 0.02 of the scored pairs, and in at
    least WORST - 0.02 of those with |delta| >= 8; sample b, nothing modified: at most WORST + 0.02 of its pairs are called modified.
    Measured, seeds 1 .. 5: sign 0.9811 .. 0.9892 of 271 .. 380 scored pairs; 0.853 .. 0.956 of them above the threshold and 0.9923 ..
    1.0000 of those right; b called modified 0.0000 .. 0.0031."""
    got = planted_results(seed)
    a = cases.judge(got["a_jit"]["rows"], got["case"]["a"], modcall.MIN_DELTA)
    b = cases.judge(got["b_jit"]["rows"], got["case"]["b"], modcall.MIN_DELTA)
    print("planted seed %d: a scored %d, sign right %.4f, above the threshold %.4f and right among them %.4f; b scored %d, called modified %.4f; a calls %s"
          % (seed, a["scored"], a["sign"], a["sure"], a["sign_sure"], b["scored"], b["modified"], got["a_jit"]["calls"]))
    assert a["scored"] >= 250 and b["scored"] >= 250
    assert a["sign"] >= WORST["sign"] - MARGIN
    assert a["sign_sure"] >= WORST["sign_sure"] - MARGIN and a["sure"] > 0.8
    assert b["modified"] <= WORST["modified_b"] + MARGIN
    truth = [st for r in got["case"]["a"] for st in r["truth"].values()]
    assert 0.4 < np.mean(truth) < 0.6 and not any(st for r in got["case"]["b"] for st in r["truth"].values())


@pytest.mark.parametrize("seed", cases.SEEDS)
def test_planted_case_scores_nine_tenths_of_its_pairs(seed):
    """A condition on the case, not a measurement: the reference scores at least 0.9 of the (read, group) pairs of both samples at
    every seed, so that dropped pairs cannot hide failures.  The pairs are counted by the case's own walk and agree with modcall's.
    Measured, seeds 1 .. 5: a 0.9633, 0.9377, 0.9500, 0.9755, 0.9463; b 0.9527, 0.9615, 0.9725, 0.9492, 0.9615.  The case keeps its
    genome inside the stage's stated scope (modcall_cases.within_scope): §19's genome at seed 1 holds three CG chains of 17 and 18
    columns, which the stage drops as `too_wide` for every read; left as they were they alone are 41 of 355 pairs, and the case would
    score 0.8535 and 0.8496.  The G of the last CG of each (positions 69, 195, 364) is an A here; no other seed is touched."""
    got = planted_results(seed)
    for name in ("a", "b"):
        groups = got[name + "_jit"]["groups"]
        assert groups["seen"] == _pairs_of(got["case"][name]) and groups["dropped"]["infeasible"] == groups["dropped"]["too_long"] == 0
        assert groups["dropped"]["too_wide"] == 0 and got["case"]["cut"] == ([68, 194, 363] if seed == 1 else [])
        print("planted seed %d sample %s: %d of %d pairs scored (%.4f), dropped %s" % (seed, name, groups["scored"], groups["seen"],
                                                                                      groups["scored"] / groups["seen"], groups["dropped"]))
    for name in ("a", "b"):
        groups = got[name + "_jit"]["groups"]
        assert groups["scored"] >= 0.9 * groups["seen"], (name, groups)


@pytest.mark.parametrize("seed", cases.SEEDS)
def test_planted_states_after_refinement(seed):
    """DESIGN 20's limitation: `squiggle --refine` with the canonical table pulls the borders wrong at a modified site.  Sample a
    again, after squiggle.refine with the canonical table and the numpy refiner: the same pairs are scored and the shares get their
    own floors by the same rule.  Measured, seeds 1 .. 5: sign 0.9779 .. 0.9901 (jittered borders: 0.9811 .. 0.9892), right among those
    above the threshold 0.9922 .. 1.0000: refinement does not lower them materially -- inside the window the borders are free under
    either hypothesis, and only the window's two ends come from the read's borders."""
    got = planted_results(seed)
    a = cases.judge(got["a_refined"]["rows"], got["case"]["a"], modcall.MIN_DELTA)
    print("planted seed %d after refinement: a scored %d, sign right %.4f, above the threshold %.4f and right among them %.4f"
          % (seed, a["scored"], a["sign"], a["sure"], a["sign_sure"]))
    assert got["a_refined"]["groups"]["seen"] == got["a_jit"]["groups"]["seen"] and a["scored"] >= got["a_jit"]["groups"]["scored"] - 3
    assert a["sign"] >= WORST["sign_refined"] - MARGIN
    assert a["sign_sure"] >= WORST["sign_sure_refined"] - MARGIN and a["sure"] > 0.8
