"""GPU: chiron_align_infix (csrc/map.hip) through chiron_amd.map against the full-table reference of tests/map_ref.py.  Every
case asserts E, M, start, end and the accepted band equal to the reference exactly: there is no tolerance.  Edge cases, lengths
around the kernel's boundaries with every flank, the band-doubling thresholds, the LDS-to-workspace threshold, determinism, the
`map` command end to end (and `assess` on what it wrote), and the window-edge rule."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from chiron_amd import map as cmap

import assess_ref
import map_ref
from test_map_cpu import E2E_SEED

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(reads, wins, band0=cmap.BAND0):
    got = cmap.align_infix(reads, wins, band0)
    for k, (a, b) in enumerate(zip(reads, wins)):
        E, M, s, e = map_ref.full_table(a, b)
        row = tuple(int(got[f][k]) for f in ("edit", "match", "start", "end", "band"))
        assert row == (E, M, s, e, map_ref.expected_band(len(a), len(b), E, band0)), (k, len(a), len(b), band0)
    return got


def _slots(n, m, w):
    dlo, dhi = map_ref.band_edges(n, m, w)
    return dhi - dlo + 1


def test_edge_cases(built):
    rng = np.random.default_rng(1)
    s = assess_ref.random_seq(700, rng)
    left, right = assess_ref.random_seq(90, rng), assess_ref.random_seq(110, rng)
    unit = assess_ref.random_seq(200, rng)
    reads = ["", "ACGT", "", s, s + assess_ref.random_seq(300, rng), "N" * 300, "NNNN", s, s, unit, "acgu" * 50, "ACNGT", "A"]
    wins = ["ACGTA", "", "", s, s, left + s, "ACGT", s + right, left + s, left + unit + right + unit + left, "TT" + "ACGT" * 50 + "GG",
            "ACNGT", "C"]
    got = _check(reads, wins)
    rows = [tuple(int(got[f][k]) for f in ("edit", "match", "start", "end")) for k in range(len(reads))]
    assert rows[0] == (0, 0, 0, 0) and rows[1] == (4, 0, 0, 0) and rows[2] == (0, 0, 0, 0)
    assert rows[3] == (0, 700, 0, 700)                       # read equals window
    assert rows[4][0] == 300 and rows[4][1] == 700           # read longer than window: its overhang is inserted
    assert rows[5] == (300, 0, 0, 0)                         # all N: against the empty substring at the very start
    assert rows[7] == (0, 700, 0, 700) and rows[8] == (0, 700, 90, 790)      # at the very start, at the very end
    assert rows[9] == (0, 200, 90, 290)                      # two exact copies: the smaller s
    assert rows[10] == (0, 200, 2, 202)                      # lower case and U
    assert rows[11][0] == 1 and rows[11][1] == 4


def test_lengths_around_every_boundary_with_every_flank(built):
    """n around a wave, THREADS and 2 * THREADS; flanks of 0, 1, 64 and 300 on each side; an exact, a 15 % and an unrelated read."""
    rng = np.random.default_rng(2)
    reads, wins = [], []
    for n in (63, 64, 65, 255, 256, 257, 511, 512, 513):
        for k, slack in enumerate((0, 1, 64, 300)):
            core = assess_ref.random_seq(n, rng)
            win = assess_ref.random_seq(slack, rng) + core + assess_ref.random_seq(slack, rng)
            reads += [core, assess_ref.mutate(core, 0.15, rng), assess_ref.random_seq(n, rng)]
            wins += [win, win, win]
    got = _check(reads, wins)
    assert np.all(got["edit"][0::3] == 0) and np.all(got["edit"][2::3] > got["edit"][1::3])


def test_band_doubles_exactly_when_the_cost_passes_it(built):
    """k N's appended to a clean read add exactly k to E: E = w is accepted in the first band, E = w + 1 in the second."""
    rng = np.random.default_rng(3)
    w = cmap.BAND0
    core = assess_ref.random_seq(600, rng)
    win = assess_ref.random_seq(100, rng) + core + assess_ref.random_seq(100, rng)
    got = _check([core + "N" * w, core + "N" * (w + 1), "N" * w + core, "N" * (w + 1) + core], [win] * 4)
    assert got["edit"].tolist() == [w, w + 1, w, w + 1] and got["band"].tolist() == [w, 2 * w, w, 2 * w]


def test_lds_to_workspace_threshold(built):
    """Accepted bands of LDS_SLOTS - 1, LDS_SLOTS and LDS_SLOTS + 1 diagonals: the last one LDS holds and the first in the
    workspace row.  A clean read of 1000 bases with 600 N's has E = 600, accepted at w = 1024, where the band of a longer window
    has m - n + 2049 diagonals; an all-N read of 1500 has E = 1500, accepted at w = 2048 > n, which is the whole table of
    n + m + 1 diagonals."""
    rng = np.random.default_rng(4)
    L = cmap.LDS_SLOTS
    core = assess_ref.random_seq(1000, rng)
    reads, wins, want_slots = [], [], []
    for slots in (L - 1, L, L + 1):
        n = 1600
        m = n + slots - 2049
        reads.append(core + "N" * 600)
        wins.append(core + assess_ref.random_seq(m - 1000, rng))
        reads.append("N" * 300 + core + "N" * 300)
        wins.append(assess_ref.random_seq(m - 1000, rng) + core)
        reads.append("N" * 1500)
        wins.append(assess_ref.random_seq(slots - 1501, rng))
        want_slots += [slots] * 3
    got = _check(reads, wins)
    assert got["band"].tolist() == [1024, 1024, 2048] * 3
    assert [_slots(len(a), len(b), int(w)) for a, b, w in zip(reads, wins, got["band"])] == want_slots
    # the full table at once, on chip and on the row
    _check(reads[:3] + reads[6:], wins[:3] + wins[6:], band0=0)


def test_band0_zero_equals_band0_256(built):
    rng = np.random.default_rng(5)
    reads, wins = [], []
    for n in (100, 700, 1300):
        core = assess_ref.random_seq(n, rng)
        win = assess_ref.random_seq(200, rng) + core + assess_ref.random_seq(250, rng)
        reads += [assess_ref.mutate(core, 0.12, rng), assess_ref.mutate(core, 0.5, rng), assess_ref.random_seq(n, rng)]
        wins += [win] * 3
    banded = _check(reads, wins, band0=cmap.BAND0)
    full = _check(reads, wins, band0=0)
    assert np.all(full["band"] == 0)
    for f in ("edit", "match", "start", "end"):
        assert np.array_equal(banded[f], full[f]), f


def test_batch_of_256_is_deterministic_and_order_independent(built):
    rng = np.random.default_rng(6)
    reads, wins = [], []
    for k in range(256):
        core = assess_ref.random_seq(int(rng.integers(500, 651)), rng)
        reads.append(assess_ref.mutate(core, (0.05, 0.15, 0.4)[k % 3], rng) if k % 7 else assess_ref.random_seq(len(core), rng))
        wins.append(assess_ref.random_seq(int(rng.integers(0, 80)), rng) + core + assess_ref.random_seq(int(rng.integers(0, 80)), rng))
    first = _check(reads, wins)
    second = cmap.align_infix(reads, wins)
    assert first.tobytes() == second.tobytes()
    for k in reversed(range(256)):
        one = cmap.align_infix([reads[k]], [wins[k]])
        assert one[0].tobytes() == first[k].tobytes(), k


def _reference_aligner(rs, ws, band0):
    return map_ref.infix_rows(rs, ws, band0, cmap.INFIX_DTYPE)


@pytest.fixture(scope="module")
def mapped(built, tmp_path_factory):
    """`chiron map` in a child process on the planted case; the host pipeline on the reference aligner next to it."""
    tmp = tmp_path_factory.mktemp("map_e2e")
    contigs, reads, truth = map_ref.planted_case(E2E_SEED)
    with open(tmp / "genome.fa", "w") as f:
        for name, seq in contigs:
            f.write(">%s a contig\n" % name)
            f.write("".join(seq[i:i + 80] + "\n" for i in range(0, len(seq), 80)))
    with open(tmp / "reads.fa", "w") as f:
        f.write("".join(">%s\n%s\n" % (name, seq) for name, seq in reads.items()))
    r = subprocess.run([sys.executable, "-m", "chiron_amd.entry", "map", "-i", str(tmp / "reads.fa"), "-g", str(tmp / "genome.fa"), "-o",
                        str(tmp / "out")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    want = cmap.map_reads(reads, cmap.Genome(contigs), aligner=_reference_aligner)
    return {"tmp": tmp, "reads": reads, "truth": truth, "report": json.loads((tmp / "out" / "map_report.json").read_text()),
            "want": want, "stderr": r.stderr}


def test_map_command_end_to_end(mapped):
    report, want, truth = mapped["report"], mapped["want"], mapped["truth"]
    by = {r["name"]: r for r in report["reads"]}
    assert len(by) == 26 and report["unmapped"] == ["noise0", "noise1"] and "noise1" in mapped["stderr"]
    assert report["totals"]["mapped"] == 24 and report["totals"]["unmapped"] == 2 and report["totals"]["edge"] == 0
    for name, (contig, start, end, strand, edits) in truth.items():
        r = by[name]
        assert (r["status"], r["contig"], r["strand"]) == ("mapped", contig, strand), name
        assert r["edit"] <= edits, (name, r["edit"], edits)            # the planted alignment is itself an infix alignment
        assert r["start"] < end and start < r["end"], (name, r["start"], r["end"], start, end)
    assert report["reads"] == json.loads(json.dumps(want["reads"]))     # the whole record, every read, the noise included
    assert report["totals"] == json.loads(json.dumps(want["totals"]))
    from chiron_amd import assess
    refs = assess.load_references(str(mapped["tmp"] / "out" / "reference"))
    assert refs == want["references"] and set(refs) == set(truth)
    paf = (mapped["tmp"] / "out" / "mapped.paf").read_text().splitlines()
    assert len(paf) == 24 and all(len(ln.split("\t")) == 12 for ln in paf)


def test_assess_on_the_mapped_references_and_assess_with_a_genome(mapped):
    """`assess -r <out>/reference` reports the mapping's E per read; `assess -g` gives the same fields in one go."""
    tmp = mapped["tmp"]
    by = {r["name"]: r for r in mapped["report"]["reads"]}
    runs = {"r": ["-r", str(tmp / "out" / "reference")], "g": ["-g", str(tmp / "genome.fa")]}
    reps = {}
    for key, extra in runs.items():
        r = subprocess.run([sys.executable, "-m", "chiron_amd.entry", "assess", "-i", str(tmp / "reads.fa"), "-o", str(tmp / (key + ".json"))] + extra,
                           cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        reps[key] = json.loads((tmp / (key + ".json")).read_text())
        assert reps[key]["paired"] == 24 and reps[key]["unpaired"] == ["noise0", "noise1"]
        for rec in reps[key]["reads"]:
            m = by[rec["name"]]
            for f in ("edit", "match", "mismatch", "insertion", "deletion", "identity", "read_len"):
                assert rec[f] == m[f], (key, rec["name"], f)
            assert rec["ref_len"] == m["end"] - m["start"]
    for rec in reps["g"]["reads"]:
        m = by[rec["name"]]
        assert (rec["strand"], rec["contig"], rec["start"], rec["end"]) == (m["strand"], m["contig"], m["start"], m["end"])
    assert reps["g"]["pooled"] == reps["r"]["pooled"]


def test_window_edge_rule_widens_until_the_read_is_inside(built):
    """The host is handed a candidate 2 * slack above the read's true place (seeds, the test hook): the window starts inside the
    read, the match touches its left edge (s = 0), the slack doubles -- twice, 256 to 1024 -- and the read is found whole.  A read
    whose candidate is right is not widened."""
    rng = np.random.default_rng(8)
    contig = assess_ref.random_seq(20000, rng)
    genome = cmap.Genome([("c", contig)])
    reads, seeds = {}, {}
    for k, (start, off) in enumerate(((6000, 512), (12000, 0))):
        reads["r%d" % k] = assess_ref.mutate(contig[start:start + 800], 0.08, rng)
        seeds["r%d" % k] = {"strand": "forward", "delta": start + off, "contig": 0}
    got = cmap.map_reads(reads, genome, seeds=seeds)
    want = cmap.map_reads(reads, genome, seeds=seeds, aligner=_reference_aligner)
    assert got["reads"] == want["reads"] and got["references"] == want["references"]
    by = {r["name"]: r for r in got["reads"]}
    assert by["r0"]["status"] == by["r1"]["status"] == "mapped"
    assert by["r0"]["widenings"] == 2 and by["r1"]["widenings"] == 0
    for k, start in ((0, 6000), (1, 12000)):
        assert abs(by["r%d" % k]["start"] - start) <= 8 and abs(by["r%d" % k]["end"] - start - 800) <= 8
    assert set(got["references"]) == {"r0", "r1"}
