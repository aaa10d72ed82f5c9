"""GPU: chiron_align_trace (csrc/trace.hip) through chiron_amd.assess.align_ops against the full-table reference walk of
tests/trace_ref.py.  Every case asserts the op array equal to the reference exactly, its = X I D counts equal to the counts
(E, M) give, and that it consumes exactly the read and exactly the reference.  Edge cases, lengths around the kernel's
boundaries with band widths of every residue mod 8 (the back-pointer packing), the LDS-to-workspace threshold, the divergence
regimes on the golden reads, determinism across batches, calls and workspace budgets, a wrong (E, M) handed to the raw call, and
`assess --profile` and `map --cigar` end to end."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from chiron_amd import _lib, assess

import assess_ref
import trace_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _band(n, m, E):
    w = trace_ref.tight_band(n, m, E)
    return min(max(0, m - n) + w, m) - max(min(0, m - n) - w, -n) + 1


def _check(reads, refs, want=None, **kw):
    """-> (op arrays, [(E, M)]).  want: the reference's (E, M, ops) per pair when the caller already has it."""
    got = assess.align_ops(reads, refs, **kw)
    want = want or [trace_ref.full_trace(a, b) for a, b in zip(reads, refs)]
    assert len(got) == len(reads)
    for k, (a, b, ops, (E, M, ref_ops)) in enumerate(zip(reads, refs, got, want)):
        assert ops.dtype == np.uint8 and ops.tobytes() == ref_ops.tobytes(), (k, len(a), len(b), assess.cigar(ops)[:80], assess.cigar(ref_ops)[:80])
        X, I, D = assess.counts(len(a), len(b), E, M)
        cnt = np.bincount(ops, minlength=4)
        assert tuple(int(v) for v in cnt) == (M, X, I, D), (k, len(a), len(b))
        assert cnt[0] + cnt[1] + cnt[2] == len(a) and cnt[0] + cnt[1] + cnt[3] == len(b)
    return got, [(E, M) for E, M, _ in want]


def test_edge_cases(built):
    rng = np.random.default_rng(1)
    s = assess_ref.random_seq(700, rng)
    reads = ["", "", "ACGT", "A", "A", "N", s, "N" * 300, "NNNN", "A" * 900, "A" * 900, "acgu" * 50, "ACNGT", "AAAA", "AAAAA"]
    refs = ["", "ACGTA", "", "A", "C", "N", s, "N" * 300, "ACGT", "A" * 640, "C" * 640, "ACGT" * 50, "ACNGT", "AAAAA", "AAAA"]
    got, _ = _check(reads, refs)
    cig = [assess.cigar(o) for o in got]
    assert cig[:6] == ["*", "5D", "4I", "1=", "1X", "1X"]
    assert cig[6] == "700=" and _band(700, 700, 0) == 1          # w* = 0: a band of one diagonal
    assert cig[7] == "300X" and cig[8] == "4X"
    assert cig[9] == "260I640="                                  # the 260-base gap is left-aligned
    assert np.bincount(got[10], minlength=4).tolist() == [0, 640, 260, 0]
    assert cig[11] == "200=" and cig[12] == "2=1X2=" and cig[13:] == ["1D4=", "1I4="]


def test_lengths_around_every_boundary(built):
    """63 / 64 / 65 (a wave), THREADS and 2 * THREADS +- 1, in equal and unequal combinations, related and unrelated content.
    The band widths 2 w* + 1 + |m-n| of the set cover every residue mod 4 and mod 8: every fill of the last back-pointer byte
    and both parities of the half rows."""
    rng = np.random.default_rng(2)
    T = assess.THREADS
    lens = [63, 64, 65, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1]
    reads, refs = [], []
    for n in lens:
        base = assess_ref.random_seq(n, rng)
        reads += [base, base, base]
        refs += [assess_ref.mutate(base, 0.15, rng), assess_ref.random_seq(n, rng), assess_ref.random_seq(lens[(lens.index(n) + 4) % len(lens)], rng)]
    # k N's appended to one side cost exactly k: w* = 0 and a band of k + 1 diagonals, for the residues chance may leave out
    for n, k in ((65, 3), (257, 4), (64, 11), (255, 12)):
        base = assess_ref.random_seq(n, rng)
        reads += [base + "N" * k, base]
        refs += [base, base + "N" * k]
    _, em = _check(reads, refs)
    widths = {2 * trace_ref.tight_band(len(a), len(b), E) + 1 + abs(len(b) - len(a)) for a, b, (E, _) in zip(reads, refs, em)}
    assert {w % 4 for w in widths} == set(range(4)) and {w % 8 for w in widths} == set(range(8)), sorted(widths)


def test_lds_to_workspace_threshold(built):
    """An all-N read against a random reference has E = max(n, m) and a band of max(n, m) + 1 diagonals: LDS_SLOTS - 1,
    LDS_SLOTS (the last one LDS holds) and LDS_SLOTS + 1 (the first in the workspace row), with the longer side as the read and
    as the reference.  4 MB of back-pointers a pair at the top."""
    rng = np.random.default_rng(3)
    L = assess.LDS_SLOTS
    reads, refs = [], []
    for longest in (L - 2, L - 1, L):
        short = (longest - 37) & ~1                      # even: E - |m-n| = short, so the band is 2 w* + 1 + |m-n| = longest + 1
        reads += ["N" * longest, "N" * short]
        refs += [assess_ref.random_seq(short, rng), assess_ref.random_seq(longest, rng)]
    _, em = _check(reads, refs)
    assert [_band(len(a), len(b), E) for a, b, (E, _) in zip(reads, refs, em)] == [L - 1, L - 1, L, L, L + 1, L + 1]
    assert [E for E, _ in em] == [L - 2, L - 2, L - 1, L - 1, L, L]
    # the other way round: a random read against an all-N reference, and a related pair in the same call as the widest band
    base = assess_ref.random_seq(600, rng)
    _check([refs[4], base], [reads[4], assess_ref.mutate(base, 0.1, rng)])


def test_divergence_regimes_on_the_golden_reads(built):
    """The five golden consensus reads (2.6 k to 13 k bases) against their 12 % mutations, and the shortest one at 30 %."""
    rng = np.random.default_rng(4)
    gold = [assess_ref.golden_read(ROOT, k) for k in range(1, 6)]
    reads = list(gold) + [min(gold, key=len)]
    refs = [assess_ref.mutate(g, 0.12, rng) for g in gold] + [assess_ref.mutate(min(gold, key=len), 0.30, rng)]
    _, em = _check(reads, refs)
    ratio = np.array([E / len(b) for (E, _), b in zip(em, refs)])
    assert np.all((ratio[:5] > 0.07) & (ratio[:5] < 0.13)) and ratio[5] > 0.2, ratio


@pytest.fixture(scope="module")
def batch():
    """512 pairs of 300 .. 500 bases and the reference's answer for them, computed once."""
    rng = np.random.default_rng(5)
    reads = [assess_ref.random_seq(int(rng.integers(300, 501)), rng) for _ in range(512)]
    refs = [assess_ref.mutate(r, (0.05, 0.15, 0.4)[k % 3], rng) if k % 7 else assess_ref.random_seq(int(rng.integers(300, 501)), rng)
            for k, r in enumerate(reads)]
    return reads, refs, [trace_ref.full_trace(a, b) for a, b in zip(reads, refs)]


def test_batch_is_deterministic_and_order_independent(built, batch):
    reads, refs, want = batch
    first, _ = _check(reads, refs, want)
    second = assess.align_ops(reads, refs)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(first, second))
    for k in reversed(range(len(reads))):
        one = assess.align_ops([reads[k]], [refs[k]])
        assert one[0].tobytes() == first[k].tobytes(), k


def test_a_small_workspace_splits_the_batch_and_changes_nothing(built, batch):
    reads, refs, want = batch
    n = [len(r) for r in reads]
    m = [len(r) for r in refs]
    plan = assess.plan_trace_batches(n, m, [E for E, _, _ in want], 2 << 20)
    assert len(plan) >= 3 and sum((b for b, _ in plan), []) == list(range(512)) and all(nb <= 2 << 20 for _, nb in plan)
    assert len(assess.plan_trace_batches(n, m, [E for E, _, _ in want], 4096 << 20)) == 1
    _check(reads, refs, want, workspace_mb=2)


def test_a_wrong_edit_or_match_is_a_status_not_a_fault(built):
    """The raw call with E one too large and M one too small for pairs 1 and 3 (so that the column counts still agree and the
    host has nothing to refuse): status 1 for those, their slices untouched, the other pairs correct."""
    import torch
    rng = np.random.default_rng(6)
    reads = [assess_ref.random_seq(n, rng) for n in (200, 310, 150, 420, 90)]
    refs = [assess_ref.mutate(r, 0.15, rng) for r in reads]
    want = [trace_ref.full_trace(a, b) for a, b in zip(reads, refs)]
    a = [assess.encode(s) for s in reads]
    b = [assess.encode(s) for s in refs]
    edit = np.array([E for E, _, _ in want], dtype=np.int32)
    match = np.array([M for _, M, _ in want], dtype=np.int32)
    for bad in (1, 3):
        edit[bad] += 1
        match[bad] -= 1
    codes = np.ascontiguousarray(np.concatenate(a + b))
    la, lb = np.array([len(s) for s in a]), np.array([len(s) for s in b])
    read_off = np.concatenate([[0], np.cumsum(la)]).astype(np.int64)
    ref_off = (read_off[-1] + np.concatenate([[0], np.cumsum(lb)])).astype(np.int64)
    ops_off = np.concatenate([[0], np.cumsum(edit.astype(np.int64) + match)]).astype(np.int64)
    ops = np.full(int(ops_off[-1]), 7, dtype=np.uint8)
    status = np.full(5, -1, dtype=np.int32)
    sizes = [assess.trace_pair_size(int(n), int(m), int(e)) for n, m, e in zip(la, lb, edit)]
    nbytes = assess.trace_workspace_size(5, sum(s[0] for s in sizes), int(max(la.max(), lb.max())), max(s[1] for s in sizes))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    st = _lib.load().chiron_align_trace(0, codes.ctypes.data, read_off.ctypes.data, ref_off.ctypes.data, 5, edit.ctypes.data, match.ctypes.data,
                                        ops_off.ctypes.data, 0, ops.ctypes.data, status.ctypes.data, ws.data_ptr(),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == _lib.OK
    assert status.tolist() == [0, 1, 0, 1, 0]
    for k in range(5):
        piece = ops[ops_off[k]:ops_off[k + 1]]
        if k in (1, 3):
            assert np.all(piece == 7)
        else:
            assert piece.tobytes() == want[k][2].tobytes(), k
    # align_ops never hands the kernel a wrong (E, M); the same pairs through it are all traced
    _check(reads, refs, want)


def test_assess_profile_end_to_end(built, tmp_path):
    """The golden tree of test_assess_command_end_to_end: `assess --profile` gives every read's cigar and the pooled profile of
    the reference; without the flag the report has its old keys and no profile."""
    rng = np.random.default_rng(7)
    out = tmp_path / "out"
    (out / "result").mkdir(parents=True)
    (out / "reference").mkdir()
    want_cigar, profiles = {}, []
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
        ops = trace_ref.trace(read, ref)
        want_cigar["read%d" % k] = trace_ref.cigar(ops)
        profiles.append(trace_ref.error_profile(read, ref, ops))
    reports = {}
    for key, extra in (("with", ["--profile"]), ("without", [])):
        path = tmp_path / (key + ".json")
        r = subprocess.run([sys.executable, "-m", "chiron_amd.entry", "assess", "-i", str(out), "-o", str(path)] + extra, cwd=ROOT,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        reports[key] = json.loads(path.read_text())
    rep = reports["with"]
    assert {rec["name"]: rec["cigar"] for rec in rep["reads"]} == want_cigar
    assert rep["profile"] == trace_ref.merge(profiles)
    plain = reports["without"]
    assert "profile" not in plain and all("cigar" not in rec for rec in plain["reads"])
    assert set(plain) == {"paired", "unpaired_count", "unpaired", "pooled", "identity_mean", "identity_median", "reads", "input", "reference",
                          "strand_mode"}
    del rep["profile"]
    for rec in rep["reads"]:
        del rec["cigar"]
    assert rep == plain


def test_map_cigar_end_to_end(built, tmp_path):
    """A two-contig genome, a forward and a reverse-strand read: `map --cigar` writes a SAM whose every CIGAR, replayed over its
    SEQ and the genome from POS, reproduces both sequences and NM, and a PAF whose cg:Z: tag is that CIGAR.  Without the flag
    there is no SAM and the PAF has its twelve columns."""
    import map_ref
    rng = np.random.default_rng(8)
    contigs = [("ctgA", assess_ref.random_seq(6000, rng)), ("ctgB", assess_ref.random_seq(5000, rng))]
    reads = {"fwd": assess_ref.mutate(contigs[0][1][1500:2400], 0.1, rng),
             "rev": map_ref.revcomp(assess_ref.mutate(contigs[1][1][2000:2700], 0.1, rng))}
    with open(tmp_path / "genome.fa", "w") as f:
        f.write("".join(">%s\n%s\n" % c for c in contigs))
    with open(tmp_path / "reads.fa", "w") as f:
        f.write("".join(">%s\n%s\n" % (name, seq) for name, seq in reads.items()))
    outs = {}
    for key, extra in (("with", ["--cigar"]), ("without", [])):
        r = subprocess.run([sys.executable, "-m", "chiron_amd.entry", "map", "-i", str(tmp_path / "reads.fa"), "-g", str(tmp_path / "genome.fa"),
                            "-o", str(tmp_path / key)] + extra, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        outs[key] = tmp_path / key
    assert not (outs["without"] / "mapped.sam").exists()
    plain = (outs["without"] / "mapped.paf").read_text().splitlines()
    assert len(plain) == 2 and all(len(ln.split("\t")) == 12 for ln in plain)
    paf = (outs["with"] / "mapped.paf").read_text().splitlines()
    assert [ln.split("\t")[:12] for ln in paf] == [ln.split("\t") for ln in plain]
    sam = (outs["with"] / "mapped.sam").read_text().splitlines()
    assert sam[:3] == ["@HD\tVN:1.6\tSO:unknown", "@SQ\tSN:ctgA\tLN:6000", "@SQ\tSN:ctgB\tLN:5000"] and len(sam) == 5
    report = {r["name"]: r for r in json.loads((outs["with"] / "map_report.json").read_text())["reads"]}
    old = {r["name"]: r for r in json.loads((outs["without"] / "map_report.json").read_text())["reads"]}
    seqs = dict(contigs)
    for line, pline in zip(sam[3:], paf):
        name, flag, contig, pos, mapq, cg, rnext, pnext, tlen, seq, qual, nm = line.split("\t")
        r = report[name]
        assert (int(flag), contig, int(pos), mapq, qual) == (0 if name == "fwd" else 16, "ctgA" if name == "fwd" else "ctgB", r["start"] + 1, "255", "*")
        assert seq == (reads[name] if name == "fwd" else map_ref.revcomp(reads[name]))
        used_read, used_ref, edits = trace_ref.replay(cg, seq, seqs[contig][int(pos) - 1:])
        assert used_read == len(seq) and used_ref == r["end"] - r["start"] and nm == "NM:i:%d" % edits == "NM:i:%d" % r["edit"]
        assert pline.split("\t")[12:] == ["cg:Z:" + cg]
        assert cg == r["cigar"] == trace_ref.cigar(trace_ref.trace(seq, seqs[contig][r["start"]:r["end"]]))
        assert {k: v for k, v in r.items() if k != "cigar"} == old[name]
