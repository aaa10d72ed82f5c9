"""CPU: the assessment's reference (tests/assess_ref.py) against exhaustive enumeration and an explicit traceback, the banded DP
with its exactness certificate against the full table, and the host side of chiron_amd.assess: readers, base coding, pairing,
report arithmetic, chiron_align_workspace_size and the argument errors chiron_align_pairs reports before it needs a GPU."""
import ctypes as C
import itertools
import json

import numpy as np
import pytest

from chiron_amd import _lib, assess

import assess_ref


def test_oracle_matches_exhaustive_enumeration():
    """Every pair over a 2-letter alphabet up to length 5 (63 x 63 pairs): the key DP finds the minimum cost and, among the
    alignments of that cost, the most matches."""
    seqs = ["".join(t) for L in range(6) for t in itertools.product("AC", repeat=L)]
    for a in seqs:
        for b in seqs:
            want = assess_ref.exhaustive(a, b) if a and b else (max(len(a), len(b)), 0)
            assert assess_ref.full_table(a, b) == want, (a, b)


def test_oracle_special_characters():
    assert assess_ref.full_table("acgu", "ACGT") == (0, 4)
    assert assess_ref.full_table("NNNN", "NNNN") == (4, 0)
    assert assess_ref.full_table("ANA", "ANA") == (1, 2)
    assert assess_ref.full_table("", "") == (0, 0)
    assert assess_ref.full_table("", "ACG") == (3, 0)
    assert assess_ref.full_table("ACG", "") == (3, 0)
    assert assess_ref.exhaustive("AnA", "aNa") == (1, 2)


def test_batched_oracle_equals_the_single_pair_oracle():
    rng = np.random.default_rng(3)
    reads = [assess_ref.random_seq(int(rng.integers(0, 60)), rng, "ACGTN") for _ in range(64)]
    refs = [assess_ref.mutate(r, 0.2, rng) if k % 2 else assess_ref.random_seq(int(rng.integers(0, 60)), rng) for k, r in enumerate(reads)]
    assert assess_ref.full_table_batch(reads, refs) == [assess_ref.full_table(a, b) for a, b in zip(reads, refs)]


def test_counts_follow_from_edit_and_match():
    """X, I, D from (n, m, E, M) equal the operation counts of an explicit traceback."""
    rng = np.random.default_rng(11)
    for t in range(300):
        a = assess_ref.random_seq(int(rng.integers(0, 40)), rng, "ACGTN" if t % 3 == 0 else "ACGT")
        b = assess_ref.mutate(a, 0.3, rng) if t % 2 else assess_ref.random_seq(int(rng.integers(0, 40)), rng)
        E, M = assess_ref.full_table(a, b)
        m_, x_, i_, d_ = assess_ref.traceback_counts(a, b)
        assert (m_, x_ + i_ + d_) == (M, E)
        assert assess_ref.counts(len(a), len(b), E, M) == (x_, i_, d_)
        assert assess.counts(len(a), len(b), E, M) == (x_, i_, d_)


def test_band_certificate_never_accepts_a_wrong_result():
    """The banded DP (the kernel's scheme: one array, anti-diagonal by anti-diagonal) at half-widths 0, 1, 2 and 4 on 1200
    random pairs: whatever the certificate E <= 2w + 1 + |m-n| accepts equals the full table, in E and in M."""
    rng = np.random.default_rng(5)
    certified = rejected = 0
    for t in range(1200):
        n, m = int(rng.integers(0, 16)), int(rng.integers(0, 16))
        alphabet = "AC" if t % 2 else "ACGT"
        a = assess_ref.random_seq(n, rng, alphabet)
        b = assess_ref.mutate(a, 0.4, rng) if t % 3 == 0 else assess_ref.random_seq(m, rng, alphabet)
        want = assess_ref.full_table(a, b)
        for w in (0, 1, 2, 4):
            E, M, ok = assess_ref.banded(a, b, w)
            assert E >= want[0]                      # a band only removes paths
            if ok:
                certified += 1
                assert (E, M) == want, (a, b, w)
            else:
                rejected += 1
        assert assess_ref.banded(a, b, 16)[:2] == want      # the whole table
    assert certified > 1000 and rejected > 200       # both sides of the rule were exercised


def test_encode_and_reverse_complement():
    assert assess.encode("ACGTacgtUuNn-*").tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 3, 3, 4, 4, 4, 4]
    assert assess.encode(b"AC").tolist() == [0, 1]
    assert assess.encode("").tolist() == []
    assert assess.reverse_complement(assess.encode("AACGN")).tolist() == assess.encode("NCGTT").tolist()


def test_readers(tmp_path):
    fq = tmp_path / "one.fastq"
    fq.write_text("@read7 extra words\nACGTN\n+\n!!!!!\n")
    assert assess.read_records(str(fq)) == [("read7", "ACGTN")]
    multi = tmp_path / "merged.fastq"
    multi.write_text("@a\nACGT\n+\n@@@@\n@b\nacgu\n+\n!!!!\n")         # a quality line that starts with '@'
    assert assess.read_records(str(multi)) == [("a", "ACGT"), ("b", "acgu")]
    fa = tmp_path / "refs.fasta"
    fa.write_text(">a desc\nACG\nTAC\n>b\nGG\n\n")
    assert assess.read_records(str(fa)) == [("a", "ACGTAC"), ("b", "GG")]
    empty = tmp_path / "empty.fasta"
    empty.write_text(">e\n")
    assert assess.read_records(str(empty)) == [("e", "")]
    bad = tmp_path / "bad.fastq"
    bad.write_text("ACGT\n")
    with pytest.raises(ValueError):
        assess.read_records(str(bad))


def _tree(tmp_path):
    (tmp_path / "result").mkdir()
    (tmp_path / "reference").mkdir()
    for name, seq in (("r1", "ACGT"), ("r2", "GGCC"), ("r3", "TTTT")):
        (tmp_path / "result" / (name + ".fastq")).write_text("@%s\n%s\n+\n%s\n" % (name, seq, "!" * len(seq)))
    (tmp_path / "result" / "merged.fastq").write_text("@r1\nACGT\n+\n!!!!\n@r2\nGGCC\n+\n!!!!\n@r3\nTTTT\n+\n!!!!\n")
    (tmp_path / "reference" / "r1_ref.fastq").write_text("@r1\nACGA\n+\n!!!!\n")
    (tmp_path / "reference" / "r2.fasta").write_text(">whatever\nGGC\n")
    return tmp_path


def test_pairing_and_unpaired(tmp_path):
    tree = _tree(tmp_path)
    reads = assess.load_reads(str(tree))
    assert reads == {"r1": "ACGT", "r2": "GGCC", "r3": "TTTT"}          # merged.fastq does not double the reads
    assert assess.load_reads(str(tree / "result" / "merged.fastq")) == reads
    refs = assess.load_references(str(tree / "reference"))
    paired, unpaired = assess.pair_reads(reads, refs)
    assert paired == [("r1", "ACGT", "ACGA"), ("r2", "GGCC", "GGC")] and unpaired == ["r3"]
    multi = tree / "refs.fasta"
    multi.write_text(">r3\nTTT\n>r1\nAC\n")
    paired, unpaired = assess.pair_reads(reads, assess.load_references(str(multi)))
    assert [p[0] for p in paired] == ["r1", "r3"] and unpaired == ["r2"]


def test_report_arithmetic():
    pairs = [("x", "ACGTACGT", "ACGAACT"), ("y", "GGGG", "GGGGCC"), ("z", "", "")]
    rows = np.zeros(len(pairs), dtype=assess.RESULT_DTYPE)
    for r, (_, a, b) in zip(rows, pairs):
        E, M = assess_ref.full_table(a, b)
        X, I, D = assess_ref.counts(len(a), len(b), E, M)
        r["read_len"], r["ref_len"], r["edit"], r["match"], r["mismatch"], r["insertion"], r["deletion"] = len(a), len(b), E, M, X, I, D
    rep = assess.build_report([p[0] for p in pairs], rows, ["forward", "reverse", "forward"], ["lost"])
    assert rep["paired"] == 3 and rep["unpaired_count"] == 1 and rep["unpaired"] == ["lost"]
    x, y, z = rep["reads"]
    assert (x["edit"], x["match"], x["mismatch"], x["insertion"], x["deletion"]) == (2, 6, 1, 1, 0)
    assert x["identity"] == 6 / 8 and x["mismatch_rate"] == 1 / 8 and x["insertion_rate"] == 1 / 8 and x["deletion_rate"] == 0
    assert (y["match"], y["deletion"], y["strand"]) == (4, 2, "reverse") and y["identity"] == 4 / 6
    assert z["identity"] == 0.0 and z["mismatch_rate"] == 0.0 and z["insertion_rate"] == 0.0 and z["deletion_rate"] == 0.0
    assert rep["pooled"]["match"] == 10 and rep["pooled"]["identity"] == 10 / 14 and rep["pooled"]["deletion_rate"] == 2 / 14
    assert rep["identity_mean"] == pytest.approx((6 / 8 + 4 / 6 + 0) / 3) and rep["identity_median"] == 4 / 6
    json.dumps(rep)
    empty = assess.build_report([], rows[:0], [], ["a", "b"])
    assert empty["paired"] == 0 and empty["identity_mean"] is None and empty["pooled"]["identity"] == 0.0


def test_choose_strand_prefers_forward_on_ties():
    f = np.zeros(3, dtype=assess.RESULT_DTYPE)
    r = np.zeros(3, dtype=assess.RESULT_DTYPE)
    f["edit"], f["match"] = [5, 5, 5], [3, 3, 3]
    r["edit"], r["match"] = [5, 4, 5], [3, 0, 4]
    rows, strands = assess.choose_strand(f, r)
    assert strands == ["forward", "reverse", "reverse"] and rows["edit"].tolist() == [5, 4, 5] and rows["match"].tolist() == [3, 0, 4]


def test_workspace_size(built):
    lib = _lib.load()
    n = C.c_size_t()
    assert lib.chiron_align_workspace_size(0, 0, C.byref(n)) == _lib.OK
    small = assess.workspace_size(8, 500)                  # 1001 diagonals fit LDS: no rows
    assert 8 * 2 * 500 <= small < 8 * 2 * 500 + 4096
    big = assess.workspace_size(8, 13000)
    assert big >= 8 * 2 * 13000 + 8 * (2 * 13000 + 2) * 8
    # the rows are per workgroup, not per pair
    many = assess.workspace_size(10 * _lib.ALIGN_MAX_GROUPS, 13000) - 10 * assess.workspace_size(_lib.ALIGN_MAX_GROUPS, 13000)
    assert many < 0
    edge = (_lib.ALIGN_LDS_SLOTS - 1) // 2                 # 2 * len + 1 diagonals: the longest pair that never leaves LDS
    assert assess.workspace_size(1, edge + 1) - assess.workspace_size(1, edge) >= (2 * edge + 4) * 8
    assert lib.chiron_align_workspace_size(1, _lib.ALIGN_MAX_LEN, C.byref(n)) == _lib.OK
    assert lib.chiron_align_workspace_size(1, _lib.ALIGN_MAX_LEN + 1, C.byref(n)) == _lib.ERR_OVERFLOW
    assert lib.chiron_align_workspace_size((1 << 24) + 1, 10, C.byref(n)) == _lib.ERR_OVERFLOW
    assert lib.chiron_align_workspace_size(-1, 10, C.byref(n)) == _lib.ERR_INVALID
    assert lib.chiron_align_workspace_size(1, -1, C.byref(n)) == _lib.ERR_INVALID
    assert lib.chiron_align_workspace_size(1, 1, None) == _lib.ERR_INVALID
    assert (assess.THREADS, assess.LDS_SLOTS, assess.BAND0, assess.MAX_LEN) == (256, 4096, 256, 1 << 17)


def _call(lib, codes, read_off, ref_off, pairs, flags=0, workspace=None):
    codes = np.asarray(codes, dtype=np.uint8)
    read_off = np.asarray(read_off, dtype=np.int64)
    ref_off = np.asarray(ref_off, dtype=np.int64)
    out = [np.zeros(max(pairs, 1), dtype=np.int32) for _ in range(3)]
    return lib.chiron_align_pairs(0, codes.ctypes.data, read_off.ctypes.data, ref_off.ctypes.data, pairs, flags,
                                  out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, workspace, None)


def test_align_pairs_argument_errors_need_no_gpu(built):
    """Everything chiron_align_pairs rejects, it rejects before it copies or launches: these return without a device."""
    lib = _lib.load()
    good = [0, 1, 2, 3, 4, 0, 1, 2]
    assert _call(lib, good, [0, 4], [4, 8], 0) == _lib.OK                                  # pairs == 0: a no-op
    assert _call(lib, good, [0, 4], [4, 8], -1) == _lib.ERR_INVALID
    assert _call(lib, good, [0, 4], [4, 8], 1, flags=1) == _lib.ERR_INVALID
    assert _call(lib, good, [-1, 4], [4, 8], 1) == _lib.ERR_INVALID
    assert _call(lib, good, [0, 4], [6, 5], 1) == _lib.ERR_INVALID                         # a decreasing offset
    assert b"ref_off" in lib.chiron_last_error()
    assert _call(lib, [0, 1, 2, 5, 0, 0, 0, 0], [0, 4], [4, 8], 1) == _lib.ERR_INVALID     # a code above 4
    assert b"code 5" in lib.chiron_last_error()
    assert _call(lib, good, [0, _lib.ALIGN_MAX_LEN + 1], [0, 4], 1) == _lib.ERR_OVERFLOW   # lengths are checked before codes are read
    assert _call(lib, good, [0, 4], [4, 8], 1, workspace=None) == _lib.ERR_INVALID         # null workspace
    with pytest.raises(ValueError):
        assess.align_pairs(["A"], [])
    assert len(assess.align_pairs([], [])) == 0
