"""CPU: locate without a GPU -- the three restatements of chiron_signal_locate's definition (tests/locate_ref.py) against each
other, the brute force included; the refusals of the two entry points and the calls that need no device; the host walk under a
sanitizer; the host rules of chiron_amd.locate (reference row, column map, query, summary, planner, files); and the planted case,
located by the reference alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import locate_cases as cases
import locate_ref as ref
import squiggle_cases
from chiron_amd import _lib, locate, map as map_mod, squiggle
from test_weight_pack_cpu import rocm_prefix

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ----------------------------------------------------------------------------------------------------------------------------
# the references
# ----------------------------------------------------------------------------------------------------------------------------
def test_reference_against_brute_force():
    """Every path enumerated for Q <= 6 and R <= 7: cost and start per end column equal in all three, breaks and ties included."""
    rng = np.random.default_rng(5000)
    with_break = tied = empty = 0
    for k in range(600):
        Q, R = int(rng.integers(1, 7)), int(rng.integers(1, 8))
        x = rng.integers(-6, 7, Q)
        e = rng.integers(-6, 7, R).astype(np.int64)
        e[rng.random(R) < (0.25 if k % 2 else 0.0)] = ref.BREAK
        if k % 5 == 0:                                   # a constant signal on a constant reference: the tie rule alone decides
            x[:] = 3
            e[e != ref.BREAK] = 3
        want = ref.columns_brute(x, e)
        assert ref.columns_plain(x, e) == want, (k, x, e)
        assert ref.columns_numpy(x, e) == want, (k, x, e)
        assert np.array_equal(ref.blocks_of(want), ref.blocks_numpy(x, e))
        assert np.array_equal(ref.blocks_of(want, 2), ref.blocks_numpy(x, e, 2))
        with_break += int((e == ref.BREAK).any())
        empty += int((e == ref.BREAK).all())
        for j, (d, s) in enumerate(want):
            assert (d == ref.NONE) == (e[j] == ref.BREAK) and (d == ref.NONE or j - (Q - 1) <= s <= j)
        if k % 5 == 0 and not (e == ref.BREAK).any():
            tied += 1                                    # all paths cost 0: the smallest start is the furthest one a path can come from
            assert want == [(0, max(j - (Q - 1), 0)) for j in range(R)]
            assert ref.blocks_of(want)[0].tolist() == [0, 0, 0]             # smallest end, smallest start
    assert with_break > 100 and tied > 50 and empty > 3


def test_reference_formulations_at_the_library_block():
    """The plain-Python recurrence against the numpy rows across a block edge, with breaks, and at the extreme values."""
    rng = np.random.default_rng(5001)
    for R, Q, breaks, wide in ((1030, 9, 0.0, False), (1025, 40, 0.05, False), (2049, 5, 0.3, True), (70, 300, 0.02, True)):
        e, x = cases.random_reference(rng, R, breaks, wide), cases.random_query(rng, Q, wide)
        assert ref.columns_plain(x, e) == ref.columns_numpy(x, e)
        assert np.array_equal(ref.locate([x], e), ref.locate_plain([x], e))
    got = ref.locate([np.full(16384, 32767, np.int16), np.full(16384, -32767, np.int16)], np.array([-32767, 32767, ref.BREAK], np.int32))
    assert got.tolist() == [[[0, 1, 1]], [[0, 0, 0]]]
    got = ref.locate([np.full(16384, 32767, np.int16)], np.array([-32767, ref.BREAK], np.int32))
    assert got.tolist() == [[[16384 * 65534, 0, 0]]] and 16384 * 65534 < 1 << 30
    assert ref.locate([np.zeros(3, np.int16)], np.full(5, ref.BREAK, np.int32)).tolist() == [[[ref.NONE] * 3]]
    assert ref.locate([], np.zeros(1500, np.int32)).shape == (0, 2, 3) and ref.locate([np.zeros(2, np.int16)], np.zeros(0, np.int32)).shape == (1, 0, 3)
    assert ref.BREAK == locate.BREAK == -(1 << 31) and ref.NONE == locate.NONE == (1 << 31) - 1 and ref.BLOCK == locate.BLOCK == 1024


# ----------------------------------------------------------------------------------------------------------------------------
# the entry points without a device
# ----------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_limits_are_bound(built):
    lib = _lib.load()
    names = {n for n, _, _ in _lib.SYMBOLS}
    assert {"chiron_signal_locate_workspace_size", "chiron_signal_locate"} <= names and hasattr(lib, "chiron_signal_locate")
    header = open(os.path.join(ROOT, "include", "chiron_amd.h")).read()
    INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1  # noqa: F841  the header's words for BREAK and NONE
    for name in ("BREAK", "NONE", "MAX_QUERY", "BLOCK", "MAX_REF", "MAX_CELLS", "CHUNK", "THREADS", "MAX_GROUPS"):
        text = header.split("#define CHIRON_LOCATE_%s " % name)[1].split("\n")[0].split("/*")[0].strip().replace("ll", "")
        assert eval(text) == getattr(_lib, "LOCATE_" + name), name
    assert lib.chiron_abi_version() == 7


def test_workspace_size_rules(built):
    lib = _lib.load()
    up = lambda v: (v + 255) // 256 * 256
    assert locate.workspace_size(3, 1000, 2049) == up(32) + up(2000) + up(4 * 2049) + up(3 * 3 * 12) + 2 * up(3 * 3072 * 8)
    assert locate.workspace_size(0, 0, 0) == 0
    assert locate.workspace_size(7, 70, 0) == up(64) + up(140)
    assert locate.workspace_size(1, 1, 1) == 3 * 256 + up(12) + 2 * 8192
    n = C.c_size_t()
    for k in range(3):
        args = [1, 1, 1]
        args[k] = -1
        assert lib.chiron_signal_locate_workspace_size(*args, C.byref(n)) == _lib.ERR_INVALID and b"negative" in lib.chiron_last_error()
    assert lib.chiron_signal_locate_workspace_size(1, 1, 1, None) == _lib.ERR_INVALID and b"null bytes" in lib.chiron_last_error()
    for args, word in (((1 << 31, 1, 1), "items in one call"), ((1, _lib.SIGNAL_MAX_SAMPLES + 1, 1), "samples in one call"),
                       ((1, 1, _lib.LOCATE_MAX_REF + 1), "ref_len"), ((1 << 20, 1, 1 << 21), "row cells")):
        with pytest.raises(_lib.ChironError) as ei:
            locate.workspace_size(*args)
        assert ei.value.status == _lib.ERR_OVERFLOW and word in str(ei.value), args
    assert locate.workspace_size(1 << 12, _lib.SIGNAL_MAX_SAMPLES, _lib.LOCATE_MAX_REF) > 1 << 43
    # it depends on the counts only and grows with each: what the planner's bisection rests on
    base = locate.workspace_size(5, 5000, 3000)
    assert all(locate.workspace_size(5 + a, 5000 + 300 * b, 3000 + 100 * c) > base for a, b, c in ((1, 0, 0), (0, 1, 0), (0, 0, 1)))


def _call(lib, samples=(1, 2, 3, 4, 5, 6), sample_off=(0, 4, 6), items=2, level=(10, -10, 0), ref_len=3, out=True, ws=0, ws_bytes=0, flags=0):
    """Two queries of 4 and 2 samples on three columns.  With ws = 0 a call that passes every check ends at the null workspace."""
    arr = lambda v, t: None if v is None else np.ascontiguousarray(np.asarray(v, dtype=t))
    a = [arr(samples, np.int16), arr(sample_off, np.int64), arr(level, np.int32)]
    o = np.full(24, 77, np.int32)                # a refused call writes nothing, whatever it was promised
    p = [None if x is None else x.ctypes.data for x in a]
    st = lib.chiron_signal_locate(0, p[0], p[1], items, p[2], ref_len, o.ctypes.data if out else None, ws, ws_bytes, flags, None)
    return st, lib.chiron_last_error().decode(), o


def test_every_refusal_comes_before_a_device(built):
    lib = _lib.load()
    INVALID, OVERFLOW = _lib.ERR_INVALID, _lib.ERR_OVERFLOW
    st, msg, o = _call(lib)
    assert st == INVALID and "chiron_signal_locate: null workspace" in msg            # everything else passed: the last check before the device
    assert (o == 77).all()
    long_off = (0, 4, 4 + _lib.LOCATE_MAX_QUERY + 1)
    for kw, status, text in (
            (dict(flags=4), INVALID, "unknown flags 0x4"),
            (dict(items=-1), INVALID, "negative size"),
            (dict(ref_len=-1), INVALID, "negative size"),
            (dict(items=1 << 31), OVERFLOW, "items in one call"),
            (dict(ref_len=_lib.LOCATE_MAX_REF + 1), OVERFLOW, "ref_len 268435457, at most 268435456"),
            (dict(sample_off=None), INVALID, "null samples / sample_off"),
            (dict(samples=None), INVALID, "null samples / sample_off"),
            (dict(level=None), INVALID, "null ref_level"),
            (dict(out=False), INVALID, "null block_out"),
            (dict(sample_off=(-1, 4, 6)), INVALID, "sample_off[0] = -1 is negative"),
            (dict(sample_off=(0, 4, 3)), INVALID, "sample_off[2] = 3 below its predecessor 4"),
            (dict(sample_off=(0, 4, 4)), INVALID, "query 1 is empty"),
            (dict(sample_off=(2, 2, 6)), INVALID, "query 0 is empty"),
            (dict(sample_off=long_off, samples=np.zeros(long_off[-1], np.int16)), OVERFLOW, "query 1 has 16385 samples, at most 16384"),
            (dict(level=(10, 32768, 0)), INVALID, "level 32768 of column 1 outside -32767..32767 and not the break value"),
            (dict(level=(10, -10, -32768)), INVALID, "level -32768 of column 2 outside -32767..32767 and not the break value"),
            (dict(level=(-(1 << 31) + 1, 0, 0)), INVALID, "level -2147483647 of column 0 outside")):
        st, msg, o = _call(lib, **kw)
        assert st == status and text in msg and msg.startswith("chiron_signal_locate: "), (kw, st, msg)
        assert (o == 77).all(), kw
    # what is legal: the extreme levels, break columns, a query at the cap, offsets that start above 0; each ends at the workspace check
    cap = (3, 3 + _lib.LOCATE_MAX_QUERY, 4 + _lib.LOCATE_MAX_QUERY)
    for kw in (dict(level=(32767, -32767, locate.BREAK)), dict(level=(locate.BREAK,) * 3), dict(sample_off=cap, samples=np.zeros(cap[-1], np.int16))):
        st, msg, _ = _call(lib, **kw)
        assert st == INVALID and "null workspace" in msg, (kw, msg)


def test_calls_that_need_no_device(built):
    lib = _lib.load()
    st, _, o = _call(lib, items=0)
    assert st == _lib.OK and (o == 77).all()                                            # no item: nothing is written
    st, _, o = _call(lib, items=0, samples=None, sample_off=None, level=None, out=False)
    assert st == _lib.OK
    st, _, o = _call(lib, ref_len=0, level=None, out=False)
    assert st == _lib.OK                                                                # no column: no block to fill
    st, msg, _ = _call(lib, ref_len=0, level=None, sample_off=(0, 4, 4))
    assert st == _lib.ERR_INVALID and "query 1 is empty" in msg                         # the queries are still checked
    assert locate.locate_call([], np.zeros(1500, np.int32)).shape == (0, 2, 3)
    got = locate.locate_call([np.zeros(3, np.int16)], np.zeros(0, np.int32))
    assert got.shape == (1, 0, 3) and got.dtype == np.int32


def test_host_walk_under_sanitizers(tmp_path):
    """tests/native/locate_pack_check.cpp, built with the ROCm host compiler under AddressSanitizer + UndefinedBehaviorSanitizer:
    csrc/locate_pack.h on offset and level arrays of exactly the stated size, each kind of fault at the last place it can sit."""
    exe = str(tmp_path / "locate_pack_check")
    cmd = [os.path.join(rocm_prefix(), "llvm", "bin", "clang++"), "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", os.path.join(HERE, "native", "locate_pack_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "locate pack OK" in r.stdout


# ----------------------------------------------------------------------------------------------------------------------------
# the host side
# ----------------------------------------------------------------------------------------------------------------------------
def _genome(rng, lengths, unknown=0.03):
    seqs = []
    for n in lengths:
        codes = rng.integers(0, 4, n)
        codes[rng.random(n) < unknown] = 4
        seqs.append("".join("ACGTN"[v] for v in codes))
    return map_mod.Genome([("ctg%d" % c, s) for c, s in enumerate(seqs)])


def test_reference_levels_against_a_walk_of_kmer_bins():
    """Every contig and strand as one error-free read over the whole contig: squiggle.kmer_bins' code per base, in signal order,
    through the table is the row's stretch; breaks between the stretches; the column map finds every column again."""
    rng = np.random.default_rng(5002)
    kinds = set()
    for k in range(1, 7):
        genome = _genome(rng, [int(rng.integers(1, 90)) for _ in range(int(rng.integers(1, 4)))] + [k - 1 if k > 1 else 1, 60])
        table = rng.integers(-3000, 3000, 4 ** k).astype(np.int32)
        table[rng.random(4 ** k) < 0.2] = squiggle.UNKNOWN
        row, cmap = locate.reference_levels(genome, table, k)
        assert row.dtype == np.int32 and len(row) == cmap.columns == int(2 * genome.lengths.sum() + 2 * len(genome.lengths) - 1)
        seen = np.zeros(len(row), bool)
        for c, n in enumerate(genome.lengths.tolist()):
            for strand in (0, 1):
                read = {"pos": int(genome.starts[c]), "ops": np.zeros(n, np.uint8), "reverse": bool(strand), "lead": 0, "called": np.zeros(n, np.uint8)}
                code = squiggle.kmer_bins(read, genome, k)
                want = np.where(code >= 0, table[np.maximum(code, 0)], squiggle.UNKNOWN)
                want = np.where(want == squiggle.UNKNOWN, locate.BREAK, want)
                a = int(cmap.first[2 * c + strand])
                assert np.array_equal(row[a:a + n], want), (k, c, strand)
                seen[a:a + n] = True
                kinds |= {(bool(v >= 0), bool(w != locate.BREAK)) for v, w in zip(code, want)}
                for i in (0, n // 2, n - 1):
                    pos = n - 1 - i if strand else i
                    assert cmap.column_to_locus(a + i) == (c, pos, strand) == locate.column_to_locus(cmap, a + i)
                    assert cmap.locus_to_column(c, pos, strand) == a + i
        assert (row[~seen] == locate.BREAK).all() and (~seen).sum() == 2 * len(genome.lengths) - 1
        assert all(cmap.column_to_locus(j) is None for j in np.flatnonzero(~seen)) and cmap.column_to_locus(len(row)) is None and cmap.column_to_locus(-1) is None
        with pytest.raises(ValueError):
            cmap.locus_to_column(0, int(genome.lengths[0]), 0)
    assert kinds == {(True, True), (True, False), (False, False)}
    # ACGTA under a table that is its own index: the 3-mers ACG, CGT, GTA forward, and TAC, ACG, CGT on the reverse complement TACGT
    row, cmap = locate.reference_levels(squiggle_cases.PlainGenome(np.array([0, 1, 2, 3, 0], np.uint8)), np.arange(64, dtype=np.int32), 3)
    B = locate.BREAK
    assert row.tolist() == [B, 6, 27, 44, B, B, B, 49, 6, 27, B] and cmap.column_to_locus(7) == (0, 3, 1)
    for table, k in ((np.zeros(63, np.int32), 3), (np.zeros(64, np.int32), 2), (np.full(4, 40000, np.int32), 1)):
        with pytest.raises(ValueError):
            locate.reference_levels(squiggle_cases.PlainGenome(np.zeros(5, np.uint8)), table, k)


def test_query_of():
    rng = np.random.default_rng(5003)
    sig = rng.normal(500, 40, 3000).astype(np.float32)
    q, why = locate.query_of(sig, 100, 1000)
    assert why is None and q.dtype == np.int16 and np.array_equal(q, squiggle.normalise(sig[100:1100], "mad"))     # on that prefix only
    assert not np.array_equal(q, squiggle.normalise(sig, "mad")[100:1100])
    q, _ = locate.query_of(sig, 2500, 1000)
    assert len(q) == 500
    assert np.array_equal(locate.query_of(sig, 0, 50, "none", 10)[0], np.rint(sig[:50]).astype(np.int16))
    assert locate.query_of(sig, 2900, 1000) == (None, "too_short") and locate.query_of(sig, 5000, 1000) == (None, "too_short")
    assert locate.query_of(np.full(900, 7.0), 0, 1000) == (None, "flat_signal")
    assert locate.query_of(sig, 0, 1000, min_samples=1001) == (None, "too_short")
    for prefix in (0, locate.MAX_QUERY + 1):
        with pytest.raises(ValueError):
            locate.query_of(sig, 0, prefix)
    assert len(locate.query_of(np.arange(20000.0), 0, locate.MAX_QUERY)[0]) == locate.MAX_QUERY


def test_summarise():
    N = locate.NONE
    none = {"best": None, "second": None, "per_sample": None, "margin": None}
    assert locate.summarise(np.zeros((0, 3), np.int32), 10) == none and locate.summarise([[N, N, N]] * 3, 10) == none
    s = locate.summarise([[500, 100, 60], [N, N, N], [300, 2100, 2050], [300, 3100, 3040], [700, 4200, 4100]], 100)
    assert s == {"best": (300, 2100, 2050), "second": 300, "per_sample": 3.0, "margin": 0.0}      # least cost at the smallest column
    s = locate.summarise([[500, 100, 60], [300, 2100, 2050], [300, 2150, 2140], [700, 2200, 2100]], 100)
    assert s["best"] == (300, 2100, 2050) and s["second"] == 500 and s["margin"] == 2.0          # 2150 and 2200 lie within a query of the best
    s = locate.summarise([[500, 2000, 1990], [300, 2100, 2050], [400, 2201, 2190]], 100)
    assert s["second"] == 400 and s["margin"] == 1.0                                               # exactly q_len away does not count
    s = locate.summarise([[500, 2000, 1990], [300, 2100, 2050], [400, 2200, 2190]], 100)
    assert s["second"] is None and s["margin"] is None and s["per_sample"] == 3.0


def test_locate_plans_its_calls_and_words_its_rows():
    """locate() with the reference as locator=: drops by reason, calls planned against the budget, rows equal however they are
    batched, the stretch and strand from the column map, the status rules, targets and the file's lines."""
    rng = np.random.default_rng(5004)
    genome = _genome(rng, [700, 500], 0.0)              # no N: a walk of consecutive columns meets no break
    table = rng.integers(-600, 600, 64).astype(np.int32)
    row, cmap = locate.reference_levels(genome, table, 3)
    reads, ends = [], []
    for k in range(12):
        contig, strand = k % 2, (k // 2) % 2
        first = int(cmap.first[2 * contig + strand]) + int(rng.integers(5, 200))
        x, end = cases.walk_query(rng, np.where(row == locate.BREAK, 0, row), first, int(rng.integers(300, 500)))
        reads.append(("r%d" % k, x.astype(np.float32)))
        ends.append((first, end))
    reads += [("short", np.zeros(50, np.float32)), ("flat", np.full(400, 3.0, np.float32))]
    calls = []

    def locator(queries, level):
        calls.append((len(queries), sum(len(q) for q in queries)))
        assert level is not None and all(q.dtype == np.int16 for q in queries)
        return ref.locate(queries, level)
    kw = dict(prefix=500, mode="none", min_samples=100, locator=locator)
    one = locate.locate(reads, row, cmap, **kw)
    assert one["dropped"] == {"too_short": 1, "flat_signal": 1} and one["batches"] == len(calls) == 1 and calls[0][0] == 12
    assert sum(one["status"].values()) == len(one["rows"]) == 12
    for r, (first, end), (name, x) in zip(one["rows"], ends, reads):
        blocks = ref.locate([np.rint(x).astype(np.int16)], row)[0]
        s = locate.summarise(blocks, len(x))
        assert r["read"] == name and r["samples"] == len(x) and (r["end_column"], r["start_column"]) == s["best"][1:]
        assert r["cost_per_sample"] == s["per_sample"] and r["margin"] == s["margin"]
        c, at_end, strand = cmap.column_to_locus(r["end_column"])
        at_start = cmap.column_to_locus(r["start_column"])[1]
        assert r["contig"] == cmap.names[c] and r["strand"] == "+-"[strand] and (r["start"], r["end"]) == (min(at_start, at_end), max(at_start, at_end) + 1)
        assert abs(r["end_column"] - end) <= 8 and abs(r["start_column"] - first) <= 8             # noise of 20 on levels 600 apart
    del calls[:]
    budget = locate.workspace_size(5, 2500, len(row))
    many = locate.locate(reads, row, cmap, workspace_mb=budget / (1 << 20), **kw)
    assert many["batches"] == len(calls) >= 3 and all(locate.workspace_size(n, s, len(row)) <= budget for n, s in calls)
    assert many["rows"] == one["rows"] and sum(n for n, _ in calls) == 12
    assert locate.plan_batches([400] * 10, 3000, locate.workspace_size(3, 1200, 3000)) == [(0, 3), (3, 6), (6, 9), (9, 10)]
    assert locate.plan_batches([400] * 3, 3000, 1) == [(0, 1), (1, 2), (2, 3)]                      # a query that alone exceeds the budget
    # the status rules
    costly = locate.locate(reads, row, cmap, max_cost=0.0, **kw)
    assert costly["status"] == {"placed": 0, "ambiguous": 0, "unplaced": 12} and costly["rows"][0]["contig"] is not None
    strict = locate.locate(reads, row, cmap, min_margin=1e9, **kw)
    with_margin = sum(1 for r in one["rows"] if r["margin"] is not None)
    assert strict["status"] == {"placed": 12 - with_margin, "ambiguous": with_margin, "unplaced": 0} and with_margin >= 6
    blank = locate.locate(reads[:3], np.full(40, locate.BREAK, np.int32), locate.ColumnMap(["x"], [40]), **kw)
    assert blank["status"]["unplaced"] == 3 and blank["rows"][0]["contig"] is None and blank["rows"][0]["cost_per_sample"] is None
    assert locate.locate([], row, cmap, **kw) == {"rows": [], "dropped": {"too_short": 0, "flat_signal": 0}, "status": dict.fromkeys(locate.STATUSES, 0), "batches": 0}
    # targets and lines
    targets = locate.parse_targets("ctg0:1-700", cmap)
    assert targets == [(0, 0, 700)] and locate.parse_targets("ctg1", cmap) == [(1, 0, 500)]
    assert locate.parse_targets("ctg0:10-20, ctg1:5-5", cmap) == [(0, 9, 20), (1, 4, 5)]
    for bad in ("nope:1-5", "ctg0:0-5", "ctg0:5-701", "ctg0:9-3", "ctg0:a-b"):
        with pytest.raises(ValueError):
            locate.parse_targets(bad, cmap)
    lines = locate.located_lines(one["rows"], targets, cmap)
    assert lines[0] == "\t".join(locate.LOCATED_COLUMNS + ("target",)) + "\n" and len(lines) == 13
    for ln, r in zip(lines[1:], one["rows"]):
        f = ln.rstrip("\n").split("\t")
        assert f[0] == r["read"] and f[2] == r["contig"] and int(f[3]) == r["start"] and int(f[4]) == r["end"] and f[5] == r["strand"] and f[8] == r["status"]
        assert f[9] == ("on_target" if r["contig"] == "ctg0" and r["status"] == "placed" else "off_target")
    assert locate.located_lines(blank["rows"])[1].split("\t")[2:] == [".", ".", ".", ".", ".", ".", "unplaced\n"]


def test_the_command_line():
    from chiron_amd import entry
    base = ["locate", "-s", "sig", "-g", "g.fa", "--table", "kmer_levels.tsv", "-o", "out"]
    args = entry.build_parser().parse_args(base)
    assert (args.table_min_events, args.skip, args.prefix, args.normalize, args.max_cost, args.min_margin, args.targets, args.workspace_mb) == (
        5, 0, 2000, "mad", None, 1.0, None, 4096) and args.func is entry.locate
    assert args.prefix == locate.DEFAULT_PREFIX and args.min_samples == locate.DEFAULT_MIN_SAMPLES and args.min_margin == locate.DEFAULT_MIN_MARGIN
    args = entry.build_parser().parse_args(base + ["--prefix", "1000", "--skip", "50", "--max-cost", "80", "--min-margin", "2.5", "--targets", "c:1-9",
                                                   "--normalize", "none", "--table-min-events", "8"])
    assert (args.prefix, args.skip, args.max_cost, args.min_margin, args.targets, args.normalize, args.table_min_events) == (1000, 50, 80.0, 2.5, "c:1-9", "none", 8)


# ----------------------------------------------------------------------------------------------------------------------------
# the planted case, on the reference alone
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", cases.SEEDS)
def test_planted_reads_are_found_again(seed):
    """locate_cases.planted(seed): 30 control reads, the first 1000 samples of each, against both strands of the 600-base genome
    (1201 columns) under the planted table; the DP is the numpy reference.  Every read ends on its true strand within 32 bases of
    the true position of its last used sample, and every margin there is is positive.
    Measured with the reference, seeds 1 .. 5: 150 of 150 reads on the true strand within 32 bases (the largest error 19, 16, 12,
    7, 2 bases), 141 within 3 (29, 26, 27, 29, 30 of 30); cost per sample 46 to 55 in the median.  A margin needs a block minimum
    whose end lies more than 1000 columns from the best end, and the row has 1201 columns in two blocks: 6 of the 150 reads have
    one (0, 1, 1, 2, 2 a seed), 28.4 at least and 32.7 in the median; the other 144 have none and are placed without one.  So the
    margin's bar here is the one the reference attains: no margin at or below 0."""
    case = cases.planted(seed)
    level, cmap = locate.reference_levels(case["genome"], case["table"], case["k"])
    assert len(level) == 1201 and (level == locate.BREAK).sum() == 9
    got = locate.locate(case["reads"], level, cmap, skip=cases.SKIP, prefix=cases.PREFIX, locator=ref.locate)
    assert len(got["rows"]) == 30 and got["status"] == {"placed": 30, "ambiguous": 0, "unplaced": 0}
    errors, margins = [], []
    for row, truth in zip(got["rows"], case["truth"]):
        pos, strand = cases.true_locus(truth, row["samples"] - 1)
        _, at, s = cmap.column_to_locus(row["end_column"])
        assert s == strand and row["strand"] == "+-"[strand], row
        errors.append(abs(at - pos))
        assert row["start"] <= at < row["end"] and row["contig"] == "ctg"
        if row["margin"] is not None:
            margins.append(row["margin"])
    print("planted seed %d: %d of 30 within 3 bases, %d within 32, largest error %d; %d margins %s; median cost per sample %.1f"
          % (seed, sum(e <= 3 for e in errors), sum(e <= 32 for e in errors), max(errors), len(margins), ["%.1f" % m for m in margins],
             float(np.median([r["cost_per_sample"] for r in got["rows"]]))))
    assert all(e <= 32 for e in errors)
    assert all(m > 0 for m in margins)
