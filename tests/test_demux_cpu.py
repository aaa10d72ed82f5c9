"""CPU: demux without a GPU -- the numpy restatements of chiron_demux_windows (tests/demux_ref.py) against brute force and against
each other, the host rules of chiron_amd.demux (windows, classify, trim, readers and writers, the planner), the refusals of the two
entry points that are decided before a device is needed, and the planted multiplexed run on the references alone."""
import ctypes as C
import functools
import itertools
import json
import os

import numpy as np
import pytest

import assess_ref
import demux_cases as cases
import demux_ref as ref
import map_ref
from chiron_amd import _lib, assess, demux

NONE = demux.NONE


def letters(codes):
    return "".join("ACGTN"[int(c)] for c in codes)


# ----------------------------------------------------------------------------------------------------------------------------
# the references
# ----------------------------------------------------------------------------------------------------------------------------
def test_reference_against_every_substring():
    """Every pattern of 1..4 and window of 0..5 bases over three letters: (E, e) of the column DP and of the bit-vector form are
    the smallest global distance (assess_ref.full_table) over every substring, then the smallest end."""
    glob = functools.lru_cache(maxsize=None)(lambda p, t: assess_ref.full_table(p, t)[0])
    pairs = 0
    for n in range(1, 5):
        for m in range(0, 6):
            for p in itertools.product(range(3), repeat=n):
                ps = letters(p)
                for t in itertools.product(range(3), repeat=m):
                    ts = letters(t)
                    D = [min(glob(ps, ts[s:e]) for s in range(e + 1)) for e in range(m + 1)]
                    want = (min(D), D.index(min(D)))
                    assert D[0] == n
                    assert ref.pair_dp(p, t) == want and ref.pair_bitvector(p, t) == want, (ps, ts)
                    pairs += 1
    assert pairs == 120 * 364


def test_reference_distance_is_the_infix_distance():
    rng = np.random.default_rng(5)
    for k in range(60):
        p = cases.random_codes(int(rng.integers(1, 65)), rng, with_n=k % 4 == 0)
        t = cases.random_codes(int(rng.integers(0, 200)), rng, with_n=k % 4 == 1)
        if k % 2 and len(t) > len(p):
            at = int(rng.integers(0, len(t) - len(p)))
            t[at:at + len(p)] = p
            t = assess.encode(assess_ref.mutate(letters(t), 0.1, rng))
        assert ref.pair_dp(p, t)[0] == map_ref.full_table(letters(p), letters(t))[0]


@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 63, 64])
def test_bitvector_form_equals_the_column_dp(n):
    """The kernel's 64-bit arithmetic in Python ints against the DP, with the first minimum: random and planted pairs, code 4 on
    either side, m = 0, and the 64-base pattern whose add wraps."""
    rng = np.random.default_rng(100 + n)
    assert ref.pair_bitvector(cases.random_codes(n, rng), []) == (n, 0) == ref.pair_dp(cases.random_codes(n, rng), [])
    for k in range(80):
        p = cases.random_codes(n, rng, with_n=k % 5 == 0)
        m = int(rng.integers(0, 160))
        t = cases.random_codes(m, rng, with_n=k % 5 == 1)
        if k % 2 and m >= n:
            at = int(rng.integers(0, m - n + 1))
            t[at:at + n] = p
            if k % 4 == 1 and n > 2:
                t = np.delete(t, at + int(rng.integers(0, n)))
        assert ref.pair_bitvector(p, t) == ref.pair_dp(p, t), (k, letters(p), letters(t))
    p = cases.random_codes(n, rng)
    t = np.concatenate([cases.random_codes(5, rng), p, cases.random_codes(5, rng)])
    E, e = ref.pair_bitvector(p, t)
    assert E == 0 and e <= 5 + n                     # an exact copy costs nothing; a shorter prefix copy may end it earlier
    assert ref.pair_dp(p, np.concatenate([p, t]))[1] <= n


def test_batched_reference_equals_the_scalar_one():
    rng = np.random.default_rng(9)
    for n, m in ((1, 0), (1, 7), (24, 40), (33, 150), (64, 64), (64, 200)):
        p = cases.random_codes(n, rng, with_n=True)
        wins = np.array([cases.random_codes(m, rng, with_n=w % 3 == 0) for w in range(9)], dtype=np.uint8).reshape(9, m)
        if m >= n:
            wins[4, m - n:] = p
            wins[5, :n] = p
        E, e = ref.pairs_batch(p, wins)
        assert [(int(a), int(b)) for a, b in zip(E, e)] == [ref.pair_dp(p, w) for w in wins]
    windows = [cases.random_codes(m, rng) for m in (0, 3, 3, 17, 0, 17, 40)]
    patterns = [cases.random_codes(n, rng) for n in (1, 5, 24)]
    E, e = ref.matrix(windows, patterns)
    for w, t in enumerate(windows):
        for q, p in enumerate(patterns):
            assert (E[w, q], e[w, q]) == ref.pair_dp(p, t)


def test_window_reduction_hand_cases():
    assert ref.reduce_window([3, 5, 4], [10, 11, 12], [7, 7, 7]) == (0, 3, 10, NONE)          # one group: no second
    assert ref.reduce_window([4, 2, 2], [1, 9, 5], [0, 1, 2]) == (1, 2, 9, 2)                 # equal E: the smaller index; margin 0
    assert ref.reduce_window([4, 2, 2], [1, 9, 5], [0, 1, 1]) == (1, 2, 9, 4)                 # a second spelling does not compete
    assert ref.reduce_window([2, 2, 6], [1, 9, 5], [3, 3, 0]) == (0, 2, 1, 6)
    assert ref.reduce_window([9], [0], [0]) == (0, 9, 0, NONE)
    rng = np.random.default_rng(2)
    E, e, groups = rng.integers(0, 4, (40, 7)), rng.integers(0, 30, (40, 7)), rng.integers(0, 3, 7)
    many = ref.reduce_windows(E, e, groups)
    assert [tuple(int(v[w]) for v in many) for w in range(40)] == [ref.reduce_window(E[w], e[w], groups) for w in range(40)]
    got = ref.match([assess.encode("ACGTACGT"), assess.encode("")], [assess.encode("ACGT"), assess.encode("ACGA"), assess.encode("TTTT")],
                    [0, 0, 1], want_matrix=True)
    assert got["best"].tolist() == [0, 0] and got["dist"].tolist() == [0, 4] and got["end"].tolist() == [4, 0]
    assert got["second"].tolist() == [3, 4] and got["pair_dist"].tolist() == [[0, 1, 3], [4, 4, 4]]
    assert got["pair_end"].tolist() == [[4, 3, 4], [0, 0, 0]]


# ----------------------------------------------------------------------------------------------------------------------------
# host rules
# ----------------------------------------------------------------------------------------------------------------------------
def test_end_windows_and_complement():
    heads, tails = demux.end_windows(["ACGTTGCA", "ACG", "", "AANNCCGGTT"], window=4)
    assert [letters(h) for h in heads] == ["ACGT", "ACG", "", "AANN"]
    assert [letters(t) for t in tails] == ["ACGT", "GCA", "", "TTGG"]        # the last 4 bases reversed, not complemented
    assert letters(demux.complement(assess.encode("AACGTN"))) == "TTGCAN"
    # a barcode B at the head reads as B; ligated to the other strand it ends the read as revcomp(B), which the reversed tail window
    # shows as complement(B): both ends report the barcode's inner boundary
    B = "AACCGTTGAC"
    read = "GG" + B + "ACGTACGTAAACCCGGGTTT" + map_ref.revcomp(B) + "TTT"
    heads, tails = demux.end_windows([read], window=20)
    assert ref.pair_dp(assess.encode(B), heads[0]) == (0, 2 + len(B))
    assert ref.pair_dp(demux.complement(assess.encode(B)), tails[0]) == (0, 3 + len(B))
    for bad in (0, demux.MAX_WINDOW + 1):
        with pytest.raises(ValueError):
            demux.end_windows(["ACGT"], window=bad)


def _end(best, dist, end, second):
    return {"best": np.array(best, np.int32), "dist": np.array(dist, np.int32), "end": np.array(end, np.int32),
            "second": np.array(second, np.int32)}


def test_classify_every_branch():
    lens = [24, 24, 25, 10]
    assert demux.allowed_errors([24, 25, 10, 64, 1]).tolist() == [4, 5, 2, 12, 0]          # 0.2 * 25 allows 5, not 4
    # the thresholds are inclusive: a dist of exactly the allowed errors hits, a margin of exactly min_margin hits
    h = _end([0, 0, 0, 0, 2, 2, 0], [4, 5, 4, 4, 5, 6, 0], [30] * 7, [6, 9, 5, NONE, 7, 9, 1])
    assert demux.hits(h, lens).tolist() == [True, False, False, True, True, False, False]
    assert demux.hits(h, lens, max_err=0.25, min_margin=1).tolist() == [True] * 7
    hit, miss = (1, 2, 40, 9), (1, 9, 40, 10)
    other, same_group = (0, 1, 35, 8), (3, 1, 20, 8)
    rows = [(hit, hit), (hit, miss), (miss, hit), (miss, miss), (hit, other), (hit, same_group)]
    head = _end(*zip(*[r[0] for r in rows]))
    tail = _end(*zip(*[r[1] for r in rows]))
    either = demux.classify(head, tail, lens, groups=[0, 1, 2, 1])
    assert either["status"] == ["classified", "classified", "classified", "unclassified", "conflict", "classified"]
    assert either["group"].tolist() == [1, 1, 1, -1, -1, 1]
    assert either["head_hit"].tolist() == [True, True, False, False, True, True]
    both = demux.classify(head, tail, lens, require="both", groups=[0, 1, 2, 1])
    assert both["status"] == ["classified", "unclassified", "unclassified", "unclassified", "conflict", "classified"]
    assert both["group"].tolist() == [1, -1, -1, -1, -1, 1]
    # without groups every pattern is its own barcode: patterns 1 and 3 disagree
    assert demux.classify(head, tail, lens)["status"][5] == "conflict"
    with pytest.raises(ValueError):
        demux.classify(head, tail, lens, require="all")
    empty = demux.classify(_end([], [], [], []), _end([], [], [], []), lens)
    assert empty["status"] == [] and len(empty["group"]) == 0


def test_trim_and_crossing_cuts():
    seq, qual = "ACGTACGTAC", "0123456789"
    assert demux.trim(seq, qual, 3, 2) == ("TACGT", "34567", 3, 8)
    assert demux.trim(seq, qual, None, 2) == ("ACGTACGT", "01234567", 0, 8)
    assert demux.trim(seq, None, 3, None) == ("TACGTAC", None, 3, 10)
    assert demux.trim(seq, qual, None, None) == (seq, qual, 0, 10)
    assert demux.trim(seq, qual, 4, 5) == ("A", "4", 4, 5)
    assert demux.trim(seq, qual, 5, 5) is None and demux.trim(seq, qual, 8, 6) is None       # the cuts meet; the cuts cross
    assert demux.trim("", None, None, None) is None and demux.trim(seq, qual, 10, None) is None


def test_readers_keep_the_quality(tmp_path):
    fq = tmp_path / "two.fastq"
    fq.write_text("@r1 extra words\nACGT\n+\n!!#$\n\n@r2\nGG\n+r2\n@@\n")
    assert demux.read_records(str(fq)) == [("r1", "ACGT", "!!#$"), ("r2", "GG", "@@")]       # a quality line may start with '@'
    assert assess.read_records(str(fq)) == [("r1", "ACGT"), ("r2", "GG")]
    fa = tmp_path / "one.fasta"
    fa.write_text(">only\nAC\nGT\n")
    assert demux.read_records(str(fa)) == [("only", "ACGT", None)]
    assert demux.load_reads(str(fa)) == [("one", "ACGT", None)]                              # a single record is named after its file
    assert demux.load_reads(str(fq)) == [("r1", "ACGT", "!!#$"), ("r2", "GG", "@@")]
    folder = tmp_path / "run" / "result"
    folder.mkdir(parents=True)
    (folder / "a.fastq").write_text("@x\nAC\n+\n!!\n")
    (folder / "merged.fastq").write_text("@x\nAC\n+\n!!\n")
    assert demux.load_reads(str(tmp_path / "run")) == [("a", "AC", "!!")]
    assert [n for n, _, _ in demux.load_reads(str(tmp_path / "run"))] == list(assess.load_reads(str(tmp_path / "run")))
    for bad in ("@r\nACGT\n+\n!!\n", "@r\nACGT\n+\n", "@r\nACGT\nACGT\n!!!!\n"):
        fq.write_text(bad)
        with pytest.raises(ValueError):
            demux.read_records(str(fq))


def test_load_patterns_and_groups(tmp_path):
    fa = tmp_path / "bc.fasta"
    fa.write_text(">bcA first\nACGTAC\n>bcB\nTTTTGG\n>bcA\nACGTAG\n")
    names, codes = demux.load_patterns(str(fa))
    assert names == ["bcA", "bcB", "bcA"] and [letters(c) for c in codes] == ["ACGTAC", "TTTTGG", "ACGTAG"]
    groups, bins = demux.groups_of(names)
    assert groups.tolist() == [0, 1, 0] and bins == ["bcA", "bcB"]
    for text in ("", ">long\n" + "A" * 65 + "\n", ">none\n\n", ">unclassified\nACGT\n", ">a/b\nACGT\n"):
        fa.write_text(text)
        with pytest.raises(ValueError):
            demux.load_patterns(str(fa))


def _hand_matcher(windows, patterns, groups):
    return ref.match(windows, patterns, groups)


def test_command_writes_bins_table_and_report(tmp_path):
    """Two barcodes of 8 bases and an adapter-free hand case: every status, the untrimmed unclassified bin, the FASTA form."""
    A, B = "AACCGGTT", "GTGTCACA"
    ins = "ACGATCGATTAGCCGATAGCTAGGATCCA"
    reads = [("both", "C" + A + ins + map_ref.revcomp(A), None), ("headB", B + ins, None), ("none", ins, None),
             ("two", A + ins + map_ref.revcomp(B) + "GG", None), ("gone", A + map_ref.revcomp(A), None)]
    fa, bc = tmp_path / "reads.fasta", tmp_path / "bc.fasta"
    fa.write_text("".join(">%s\n%s\n" % (n, s) for n, s, _ in reads))
    bc.write_text(">bcA\n%s\n>bcB\n%s\n" % (A, B))
    out = tmp_path / "out"
    report = demux.demux_command(str(fa), str(bc), str(out), window=12, max_err=0.2, min_margin=2, matcher=_hand_matcher)
    assert sorted(os.listdir(out)) == ["bcA.fasta", "bcB.fasta", "demux.tsv", "demux_report.json", "unclassified.fasta"]
    assert (out / "bcA.fasta").read_text() == ">both\n%s\n" % ins
    assert (out / "bcB.fasta").read_text() == ">headB\n%s\n" % ins
    assert (out / "unclassified.fasta").read_text() == ">none\n%s\n>two\n%s\n" % (ins, reads[3][1])            # untrimmed
    assert report["status"] == {"classified": 2, "unclassified": 1, "conflict": 1, "empty": 1}
    assert report["bins"] == {"bcA": 1, "bcB": 1} and report["reads"] == 5 and report["calls"] == {"head": 1, "tail": 1}
    assert json.load(open(out / "demux_report.json")) == report
    table = [ln.split("\t") for ln in (out / "demux.tsv").read_text().splitlines()]
    assert tuple(table[0]) == demux.TSV_COLUMNS and len(table) == 6
    row = dict(zip(table[0], table[1]))
    assert (row["read"], row["status"], row["barcode"], row["kept_start"], row["kept_end"]) == ("both", "classified", "bcA", "9", str(9 + len(ins)))
    assert (row["head_best"], row["head_dist"], row["head_end"], row["head_hit"], row["tail_end"]) == ("0", "0", "9", "1", "8")
    assert dict(zip(table[0], table[5]))["status"] == "empty" and dict(zip(table[0], table[3]))["barcode"] == "-"
    assert assess.load_reads(str(out / "unclassified.fasta")) == {"none": ins, "two": reads[3][1]}
    # --no-trim keeps the classified reads whole; nothing is empty then
    whole = demux.demux_command(str(fa), str(bc), str(tmp_path / "whole"), window=12, do_trim=False, matcher=_hand_matcher)
    assert whole["status"]["empty"] == 0 and whole["bases"]["written"] == whole["bases"]["in"]
    assert (tmp_path / "whole" / "bcA.fasta").read_text() == ">both\n%s\n>gone\n%s\n" % (reads[0][1], reads[4][1])
    # one adapter: plain trimming into one bin, and a second of NONE passes the margin
    bc.write_text(">adapter\n%s\n" % A)
    one = demux.demux_command(str(fa), str(bc), str(tmp_path / "one"), window=12, matcher=_hand_matcher)
    assert one["bins"] == {"adapter": 2} and one["status"]["empty"] == 1
    assert "\t-\t" in (tmp_path / "one" / "demux.tsv").read_text().splitlines()[1]


# ----------------------------------------------------------------------------------------------------------------------------
# the entry points' refusals
# ----------------------------------------------------------------------------------------------------------------------------
def test_size_function_and_planner(built):
    lib = _lib.load()
    n = C.c_size_t()
    size = lambda *a: (lib.chiron_demux_workspace_size(*a, C.byref(n)), n.value)
    assert size(0, 0, 12, 0) == (_lib.OK, 0) and size(0, 0, 12, 1) == (_lib.OK, 0)
    st, nbytes = size(1000, 150000, 96, 0)
    parts = 96 * 40 + 1000 * 16 + 150000 + 8 * 1000 + 1000 * 16
    assert st == _lib.OK and parts <= nbytes <= parts + 4 * 256 and nbytes % 256 == 0
    assert demux.workspace_size(1000, 150000, 96) == nbytes
    assert size(1000, 150000, 96, 1)[1] - nbytes in range(2 * 2 * 96 * 1000, 2 * 2 * 96 * 1000 + 2 * 256 + 1)
    for k in range(3):                                                      # monotone in every argument
        prev = 0
        for step in (0, 1, 300):
            args = [1000, 150000, 96, 1]
            args[k] += step
            st, got = size(*args)
            assert st == _lib.OK and got >= prev
            prev = got
    for bad in ((-1, 0, 1, 0), (1, -1, 1, 0), (1, 1, -1, 0)):
        assert size(*bad)[0] == _lib.ERR_INVALID and b"negative size" in lib.chiron_last_error()
    assert size(1, 1, 0, 0)[0] == _lib.ERR_INVALID and lib.chiron_last_error() == b"chiron_demux_workspace_size: no patterns"
    for bad, text in ((((1 << 24) + 1, 0, 1, 0), b"16777217 windows in one call, at most 2^24"),
                      ((1, 1, 65537, 0), b"65537 patterns in one call, at most 65536"),
                      ((2, 8193, 1, 0), b"8193 window bytes for 2 windows of at most 4096 bases")):
        assert size(*bad)[0] == _lib.ERR_OVERFLOW and text in lib.chiron_last_error(), bad
    assert lib.chiron_demux_workspace_size(1, 1, 1, 0, None) == _lib.ERR_INVALID
    # the planner: as few consecutive runs as the budget allows, a window alone always goes
    lens = [150] * 10 + [0] * 3 + [40] * 7
    assert demux.plan_batches([], 12, 1 << 20) == [] and demux.plan_batches(lens, 12, 1 << 30) == [(0, 20)]
    runs = demux.plan_batches(lens, 12, demux.workspace_size(4, 600, 12))
    assert runs[0] == (0, 4) and runs[-1][1] == 20 and all(a[1] == b[0] for a, b in zip(runs, runs[1:]))
    for first, last in runs:
        assert demux.workspace_size(last - first, sum(lens[first:last]), 12) <= demux.workspace_size(4, 600, 12)
        if last < 20:
            assert demux.workspace_size(last + 1 - first, sum(lens[first:last + 1]), 12) > demux.workspace_size(4, 600, 12)
    assert demux.plan_batches(lens, 12, 1) == [(k, k + 1) for k in range(20)]
    assert len(demux.plan_batches(lens, 12, demux.workspace_size(4, 600, 12, True), True)) >= len(runs)


def _good():
    """A good call of three windows and two patterns, as a dict in the prototype's order."""
    return {"device_id": 0, "win_codes": np.array([0, 1, 2, 3, 0, 1, 4, 3, 2], np.uint8), "win_off": [0, 4, 4, 9], "windows": 3,
            "pat_codes": np.array([0, 1, 2, 3, 3], np.uint8), "pat_off": [0, 3, 5], "pat_group": np.array([0, 1], np.int32), "patterns": 2,
            "flags": 0, "best_out": np.zeros(3, np.int32), "dist_out": np.zeros(3, np.int32), "end_out": np.zeros(3, np.int32),
            "second_out": np.zeros(3, np.int32), "pair_dist_out": np.zeros(6, np.int16), "pair_end_out": np.zeros(6, np.int16),
            "workspace": np.zeros(64, np.uint8), "stream": None}


REFUSALS = {
    "unknown_flags": ({"flags": 2}, 1, "chiron_demux_windows: unknown flags 0x2"),
    "negative_windows": ({"windows": -1}, 1, "chiron_demux_windows: negative size (windows -1, window bytes 0, patterns 2)"),
    "negative_patterns": ({"patterns": -2}, 1, "chiron_demux_windows: negative size (windows 3, window bytes 0, patterns -2)"),
    "no_patterns": ({"patterns": 0}, 1, "chiron_demux_windows: no patterns"),
    "too_many_windows": ({"windows": (1 << 24) + 1}, 4, "chiron_demux_windows: 16777217 windows in one call, at most 2^24"),
    "too_many_patterns": ({"patterns": 65537}, 4, "chiron_demux_windows: 65537 patterns in one call, at most 65536"),
    "null_window_offsets": ({"win_off": None}, 1, "chiron_demux_windows: null offsets"),
    "null_pattern_offsets": ({"pat_off": None}, 1, "chiron_demux_windows: null offsets"),
    "null_pattern_codes": ({"pat_codes": None}, 1, "chiron_demux_windows: null patterns"),
    "null_groups": ({"pat_group": None}, 1, "chiron_demux_windows: null patterns"),
    "null_output": ({"end_out": None}, 1, "chiron_demux_windows: null output"),
    "half_a_matrix": ({"pair_end_out": None}, 1, "chiron_demux_windows: pair_dist_out and pair_end_out go together, both or neither"),
    "null_windows": ({"win_codes": None}, 1, "chiron_demux_windows: null windows"),
    "negative_first_window_offset": ({"win_off": [-1, 4, 4, 9]}, 1, "chiron_demux_windows: win_off[0] = -1 is negative"),
    "decreasing_window_offset": ({"win_off": [0, 4, 3, 9]}, 1, "chiron_demux_windows: win_off[2] = 3 below its predecessor 4"),
    "negative_first_pattern_offset": ({"pat_off": [-1, 3, 5]}, 1, "chiron_demux_windows: pat_off[0] = -1 is negative"),
    "decreasing_pattern_offset": ({"pat_off": [0, 3, 2]}, 1, "chiron_demux_windows: pat_off[2] = 2 below its predecessor 3"),
    "window_code": ({"win_codes": np.array([0, 1, 2, 3, 0, 1, 5, 3, 2], np.uint8)}, 1, "chiron_demux_windows: code 5 at 2 of window 2 outside 0..4"),
    "pattern_code": ({"pat_codes": np.array([0, 1, 2, 3, 9], np.uint8)}, 1, "chiron_demux_windows: code 9 at 1 of pattern 1 outside 0..4"),
    "empty_pattern": ({"pat_off": [0, 3, 3]}, 1, "chiron_demux_windows: pattern 1 has no bases"),
    "negative_group": ({"pat_group": np.array([0, -1], np.int32)}, 1, "chiron_demux_windows: pat_group[1] = -1 is negative"),
    "pattern_too_long": ({"pat_codes": np.zeros(70, np.uint8), "pat_off": [0, 3, 68]}, 4, "chiron_demux_windows: pattern 1 has 65 bases, at most 64"),
    "window_too_long": ({"win_codes": np.zeros(5000, np.uint8), "win_off": [0, 4, 4, 4101]}, 4,
                        "chiron_demux_windows: window 2 has 4097 bases, at most 4096"),
    "null_workspace": ({"workspace": None}, 1, "chiron_demux_windows: null workspace"),
    "no_device": ({"device_id": -1}, 2, "no HIP device -1: libchiron_amd has no CPU fallback"),
}


def _call(lib, args):
    keep = [np.asarray(v, dtype=np.int64) if isinstance(v, list) else v for v in args.values()]
    return lib.chiron_demux_windows(*[v.ctypes.data if isinstance(v, np.ndarray) else v for v in keep])


@pytest.mark.parametrize("check", sorted(REFUSALS))
def test_refusal_status_and_text(built, check):
    lib = _lib.load()
    change, status, text = REFUSALS[check]
    args = _good()
    args.update(change)
    assert (_call(lib, args), lib.chiron_last_error().decode()) == (status, text)
    assert not args["best_out"].any() and not args["pair_dist_out"].any()


def test_no_windows_touch_no_device(built):
    lib = _lib.load()
    args = dict(_good(), windows=0, device_id=-1, workspace=None, win_off=None, win_codes=None, best_out=None, pair_end_out=None)
    assert _call(lib, args) == _lib.OK
    got = demux.match_call([], [np.zeros(4, np.uint8)], [0], want_matrix=True)
    assert got["best"].shape == (0,) and got["pair_dist"].shape == (0, 1)
    assert demux.match_windows([], [np.zeros(4, np.uint8)], [0])["calls"] == 0


# ----------------------------------------------------------------------------------------------------------------------------
# the planted run on the references
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    case = cases.planted()
    names = [n for n, _ in case["barcodes"]]
    patterns = [assess.encode(s) for _, s in case["barcodes"]]
    groups, bins = demux.groups_of(names)
    result = demux.demux(case["reads"], patterns, groups, matcher=_hand_matcher)
    return case, bins, result


def test_planted_run_on_the_reference(planted):
    """The conditions the reference has to meet before any GPU run (seed demux_cases.SEED, the command's defaults).  Both
    thresholds are inclusive (test_classify_every_branch pins that a dist of exactly the allowed errors and a margin of exactly
    min_margin hit), so a read that sits on one is decided, not left to a tie."""
    case, bins, result = planted
    rows = {row["read"]: row for row in result["rows"]}
    carrying = binned = 0
    for name, (kind, head, tail) in case["truth"].items():
        row = rows[name]
        got = bins[row["barcode"]] if row["status"] == "classified" else None
        if kind in ("both", "head", "tail"):
            carrying += 1
            assert got in (None, head or tail), (name, kind, got)                  # never another barcode's bin
            binned += got is not None
        elif kind == "two" and row["head_hit"] and row["tail_hit"]:
            assert row["status"] == "conflict", name
        if row["status"] == "classified":
            assert 0 <= row["kept_start"] < row["kept_end"] <= row["length"]
            assert len(row["seq"]) == len(row["qual"]) == row["kept_end"] - row["kept_start"]
    assert carrying == 180 and binned >= 0.9 * carrying
    assert sum(1 for row in rows.values() if row["status"] == "conflict") >= 40     # most of the 60 two-barcode reads hit twice
    none = [rows[n] for n, t in case["truth"].items() if t[0] == "none"]
    assert sum(1 for row in none if row["status"] == "classified") <= 1             # random inserts almost never hold a barcode


def test_planted_trimming_recovers_the_insert(planted):
    """A read with the same barcode planted at both ends that hit at both: the kept range is the insert, give or take the few bases
    by which an edit-distance end can slide at a mutated barcode's inner edge."""
    case, bins, result = planted
    seqs = {n: s for n, s, _ in case["reads"]}
    checked = 0
    for row in result["rows"]:
        if case["truth"][row["read"]][0] == "both" and row["head_hit"] and row["tail_hit"] and row["status"] == "classified":
            kept = row["kept_end"] - row["kept_start"]
            assert 200 - 6 <= kept <= 400 + 6
            assert row["seq"] == seqs[row["read"]][row["kept_start"]:row["kept_end"]]
            assert row["kept_start"] >= 24 - 6 and row["length"] - row["kept_end"] >= 24 - 6
            checked += 1
    assert checked >= 40
