"""GPU: chiron_align_pairs (csrc/assess.hip) through chiron_amd.assess against the full-table reference of tests/assess_ref.py.
Every case asserts (E, M) equal to the reference exactly: there is no tolerance.  Edge cases, lengths around the kernel's
boundaries (64, the cells a workgroup updates per pass, the LDS-to-workspace threshold), the divergence regimes on the golden
consensus reads, a 2048-pair batch (run to run and against one-at-a-time calls in reverse order), both strands, and the
`assess` command end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from chiron_amd import assess

import assess_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _expected_band(n, m, E):
    """The half-width the kernel must stop at: the first of BAND0 * 2^k that certifies E or covers the table."""
    w = assess.BAND0
    while not (E <= 2 * w + 1 + abs(m - n) or (min(0, m - n) - w <= -n and max(0, m - n) + w >= m)):
        w *= 2
    return w


def _check(reads, refs, want=None):
    got = assess.align_pairs(reads, refs)
    want = want or [assess_ref.full_table(a, b) for a, b in zip(reads, refs)]
    for k, (a, b, (E, M)) in enumerate(zip(reads, refs, want)):
        n, m = len(a), len(b)
        assert (int(got["edit"][k]), int(got["match"][k])) == (E, M), (k, n, m)
        X, I, D = assess_ref.counts(n, m, E, M)
        assert (int(got["mismatch"][k]), int(got["insertion"][k]), int(got["deletion"][k])) == (X, I, D)
        assert got["identity"][k] == (M / (M + X + I + D) if n + m else 0.0)
        assert int(got["band"][k]) == _expected_band(n, m, E), (k, n, m, E, int(got["band"][k]))
    return got


def _slots(n, m, w):
    return min(max(0, m - n) + w, m) - max(min(0, m - n) - w, -n) + 1


def test_edge_cases(built):
    rng = np.random.default_rng(1)
    s = assess_ref.random_seq(700, rng)
    reads = ["", "", "ACGT", "A", "A", "N", s, "N" * 300, "NNNN", "A" * 900, "A" * 900, "acgu" * 50, "ACNGT"]
    refs = ["", "ACGTA", "", "A", "C", "N", s, "N" * 300, "ACGT", "A" * 640, "C" * 640, "ACGT" * 50, "ACNGT"]
    got = _check(reads, refs)
    assert (int(got["edit"][0]), int(got["match"][0]), got["identity"][0]) == (0, 0, 0.0)
    assert (int(got["edit"][1]), int(got["match"][1])) == (5, 0)
    assert (int(got["edit"][6]), int(got["match"][6]), got["identity"][6]) == (0, 700, 1.0)
    assert (int(got["edit"][7]), int(got["match"][7])) == (300, 0)
    assert (int(got["edit"][9]), int(got["match"][9])) == (260, 640)
    assert (int(got["edit"][11]), int(got["match"][11])) == (0, 200)


def test_lengths_around_every_boundary(built):
    """63 / 64 / 65 (a wave), THREADS and 2 * THREADS +- 1 (the diagonals one pass of the workgroup covers), in equal and
    unequal combinations, related and unrelated content."""
    rng = np.random.default_rng(2)
    T = assess.THREADS
    lens = [63, 64, 65, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1]
    reads, refs = [], []
    for n in lens:
        base = assess_ref.random_seq(n, rng)
        reads += [base, base, base]
        refs += [assess_ref.mutate(base, 0.15, rng), assess_ref.random_seq(n, rng), assess_ref.random_seq(lens[(lens.index(n) + 4) % len(lens)], rng)]
    _check(reads, refs)


def test_lds_to_workspace_threshold(built):
    """Bands of LDS_SLOTS - 1, LDS_SLOTS and LDS_SLOTS + 1 diagonals: the last one LDS holds and the first in the workspace row.
    A read that matches nothing has E = n, so the certificate accepts exactly when m <= 2w + 1: with m = 2000 the kernel stops at
    w = 1024, where the band has |m-n| + 2049 diagonals."""
    rng = np.random.default_rng(3)
    L, m = assess.LDS_SLOTS, 2000
    reads, refs, want_slots = [], [], []
    for slots in (L - 1, L, L + 1):
        gap = slots - 2049
        ref = assess_ref.random_seq(m, rng)
        for read, rf in (("N" * (m + gap), ref), (ref + "N" * gap, "N" * m), (assess_ref.random_seq(m + gap, rng, "AN"), assess_ref.random_seq(m, rng, "CG"))):
            reads.append(read)
            refs.append(rf)
            want_slots.append(slots)
    got = _check(reads, refs)
    assert [_slots(len(a), len(b), int(w)) for a, b, w in zip(reads, refs, got["band"])] == want_slots
    # the same with the roles swapped (the band hangs on the other side of diagonal 0), and a table that is wider than LDS in full
    _check(refs, reads)
    a, b = "N" * 2050, assess_ref.random_seq(2050, rng)
    got = _check([a, b], [b, a])
    assert _slots(2050, 2050, int(got["band"][0])) == L + 1


def test_divergence_regimes_on_the_golden_reads(built):
    """Seeded substitutions, insertions and deletions on the golden consensus reads (2.6 k to 13 k bases) at 12 % and 30 %,
    unrelated sequences, and a read three times its reference.  Some pair finishes in the first band, some needs >= 3 doublings."""
    rng = np.random.default_rng(4)
    gold = [assess_ref.golden_read(ROOT, k) for k in range(1, 6)]
    reads, refs = [], []
    for g in gold:                                              # 12 %: E / m near 0.10
        reads.append(g)
        refs.append(assess_ref.mutate(g, 0.12, rng))
    longest = max(gold, key=len)
    shortest = min(gold, key=len)
    for g in (shortest, longest):                               # 30 %: E / m near 0.24
        reads.append(g)
        refs.append(assess_ref.mutate(g, 0.30, rng))
    reads.append(assess_ref.random_seq(6000, rng))              # unrelated
    refs.append(assess_ref.random_seq(6000, rng))
    reads.append(assess_ref.mutate(shortest, 0.02, rng))        # a near-perfect read
    refs.append(shortest)
    third = gold[1][:len(gold[1]) // 3 * 3]
    reads.append(third)                                         # n = 3m
    refs.append(assess_ref.mutate(third[len(third) // 3:2 * len(third) // 3], 0.12, rng))
    got = _check(reads, refs)
    ratio = got["edit"][:5] / got["ref_len"][:5]
    assert np.all((ratio > 0.07) & (ratio < 0.13)), ratio
    bands = got["band"].tolist()
    assert min(bands) == assess.BAND0 and max(bands) >= 8 * assess.BAND0, bands


def test_batch_of_2048_is_deterministic_and_order_independent(built):
    """One pair per workgroup.  The batch with more pairs than workgroups is tests/test_gpu_reuse.py's."""
    rng = np.random.default_rng(5)
    reads = [assess_ref.random_seq(int(rng.integers(300, 501)), rng) for _ in range(2048)]
    refs = [assess_ref.mutate(r, (0.05, 0.15, 0.4)[k % 3], rng) if k % 7 else assess_ref.random_seq(int(rng.integers(300, 501)), rng)
            for k, r in enumerate(reads)]
    first = _check(reads, refs, assess_ref.full_table_batch(reads, refs))
    second = assess.align_pairs(reads, refs)
    assert first.tobytes() == second.tobytes()
    for k in reversed(range(2048)):
        one = assess.align_pairs([reads[k]], [refs[k]])
        assert one[0].tobytes() == first[k].tobytes(), k


def _revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTN", "TGCAN"))


def test_reverse_strand_is_found(built, tmp_path):
    rng = np.random.default_rng(6)
    read = assess_ref.golden_read(ROOT, 1)
    ref = assess_ref.mutate(read, 0.1, rng)
    (tmp_path / "reads").mkdir()
    (tmp_path / "refs").mkdir()
    (tmp_path / "reads" / "fwd.fastq").write_text("@fwd\n%s\n+\n%s\n" % (read, "!" * len(read)))
    (tmp_path / "reads" / "rev.fastq").write_text("@rev\n%s\n+\n%s\n" % (read, "!" * len(read)))
    (tmp_path / "refs" / "fwd.fasta").write_text(">fwd\n%s\n" % ref)
    (tmp_path / "refs" / "rev.fasta").write_text(">rev\n%s\n" % _revcomp(ref))
    E, M = assess_ref.full_table(read, ref)
    rep = assess.assess(str(tmp_path / "reads"), str(tmp_path / "refs"), strand="both")
    by = {r["name"]: r for r in rep["reads"]}
    assert by["fwd"]["strand"] == "forward" and by["rev"]["strand"] == "reverse"
    for r in by.values():
        assert (r["edit"], r["match"]) == (E, M)
    only = assess.assess(str(tmp_path / "reads"), str(tmp_path / "refs"), strand="forward")
    rev = {r["name"]: r for r in only["reads"]}["rev"]
    assert rev["strand"] == "forward" and (rev["edit"], rev["match"]) == assess_ref.full_table(read, _revcomp(ref))


def test_assess_command_end_to_end(built, tmp_path):
    """A `call` output tree from the golden FASTQs and mutated references, one read without a reference: the report's numbers
    are the reference's, and the unpaired read is listed."""
    rng = np.random.default_rng(7)
    out = tmp_path / "out"
    (out / "result").mkdir(parents=True)
    (out / "reference").mkdir()
    want = {}
    for k in range(1, 6):
        src = os.path.join(ROOT, "tests", "golden", "example_dna", "result", "read%d.fastq" % k)
        with open(src) as f:
            text = f.read()
        (out / "result" / ("read%d.fastq" % k)).write_text(text)
        if k == 3:
            continue
        read = text.split("\n")[1].strip()
        ref = assess_ref.mutate(read, 0.12, rng)
        (out / "reference" / ("read%d_ref.fastq" % k)).write_text("@read%d\n%s\n+\n%s\n" % (k, ref, "!" * len(ref)))
        E, M = assess_ref.full_table(read, ref)
        want["read%d" % k] = (len(read), len(ref), E, M) + assess_ref.counts(len(read), len(ref), E, M)
    report = tmp_path / "report.json"
    r = subprocess.run([sys.executable, "-m", "chiron_amd.entry", "assess", "-i", str(out), "-o", str(report)], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rep = json.loads(report.read_text())
    assert rep["paired"] == 4 and rep["unpaired_count"] == 1 and rep["unpaired"] == ["read3"]
    assert "read3" in r.stderr
    tot = np.zeros(4, dtype=np.int64)
    idents = []
    for rec in rep["reads"]:
        n, m, E, M, X, I, D = want[rec["name"]]
        assert (rec["read_len"], rec["ref_len"], rec["edit"], rec["match"], rec["mismatch"], rec["insertion"], rec["deletion"]) == (n, m, E, M, X, I, D)
        den = M + X + I + D
        assert (rec["identity"], rec["mismatch_rate"], rec["insertion_rate"], rec["deletion_rate"]) == (M / den, X / den, I / den, D / den)
        assert rec["strand"] == "forward"
        tot += (M, X, I, D)
        idents.append(M / den)
    pooled = rep["pooled"]
    assert (pooled["match"], pooled["mismatch"], pooled["insertion"], pooled["deletion"]) == tuple(int(v) for v in tot)
    assert pooled["identity"] == tot[0] / tot.sum() and pooled["insertion_rate"] == tot[2] / tot.sum()
    assert rep["identity_mean"] == pytest.approx(np.mean(idents), abs=1e-15) and rep["identity_median"] == pytest.approx(np.median(idents), abs=1e-15)
    # no pair at all: a non-zero exit status
    (tmp_path / "none").mkdir()
    r = subprocess.run([sys.executable, "-m", "chiron_amd.entry", "assess", "-i", str(out), "-r", str(tmp_path / "none"), "-o",
                        str(tmp_path / "r2.json")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert json.loads((tmp_path / "r2.json").read_text())["unpaired_count"] == 5
