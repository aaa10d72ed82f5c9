"""GPU: chiron_signal_levels (csrc/signal.hip) through chiron_amd.squiggle against the numpy formulation of tests/squiggle_ref.py
(which tests/test_squiggle_cpu.py holds to the plain-Python one), and `squiggle` end to end.  Everything is an integer: every
comparison is exact."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from chiron_amd import _lib, squiggle

import squiggle_cases as cases
import squiggle_ref as ref
from ws_guard import FILLS, Recorder

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIECE = 1024                      # samples a wave of signal_kernel stages at once


def _check(signals, starts, bins, n_bins, want_levels=True):
    """One call against the reference, every plane element and every level.  -> the GPU's (planes, levels)."""
    planes, levels = squiggle.reduce_call(signals, starts, bins, n_bins, want_levels)
    want_planes, want_levels_ = ref.reduce_numpy(signals, starts, bins, n_bins)
    assert planes.dtype == np.int64 and planes.shape == (4, n_bins)
    bad = np.argwhere(planes != want_planes)
    assert len(bad) == 0, (bad[:5].tolist(), planes[tuple(bad[0])], want_planes[tuple(bad[0])])
    if want_levels:
        assert len(levels) == len(want_levels_)
        for r, (a, b) in enumerate(zip(levels, want_levels_)):
            assert a.dtype == np.int32 and a.shape == b.shape, r
            bad = np.flatnonzero(a != b)
            assert len(bad) == 0, (r, bad[:5].tolist(), a[bad[:5]].tolist(), b[bad[:5]].tolist())
    else:
        assert levels is None
    return planes, levels


SPANS = [0, 1, 63, 64, 65, PIECE - 1, PIECE, PIECE + 1, 5000]


def test_every_span_length(built):
    """Spans of 0, 1, 63, 64, 65, piece - 1, piece, piece + 1 and 5000 samples: each alone in a read, all in one read in both
    orders (so that every one of them crosses piece borders at another offset), and each between ordinary neighbours."""
    rng = np.random.default_rng(2000)
    per_read = [[s] for s in SPANS] + [SPANS, SPANS[::-1]]
    for s in SPANS:
        per_read.append(rng.integers(1, 12, 70).tolist() + [s] + rng.integers(1, 12, 70).tolist())
    signals, starts, bins, n_bins = cases.spans_set(rng, per_read, 9, heads=[int(h) for h in rng.integers(0, 9, len(per_read))])
    planes, levels = _check(signals, starts, bins, n_bins)
    assert levels[0].tolist() == [squiggle.EMPTY] and levels[1][0] == signals[1][starts[1][0]]
    assert planes[1].sum() == sum(int(st[n + 1] - st[n]) for st, b in zip(starts, bins) for n in range(len(b)) if b[n] >= 0)
    # the same spans over small values: the sums stay far from any limit, a wrong sample count shows as a wrong level
    _check(*cases.spans_set(rng, per_read, 3, low=-5, high=6))


@pytest.mark.parametrize("bases", [1, 63, 64, 65, 257])
def test_read_lengths(built, bases):
    rng = np.random.default_rng(2100 + bases)
    _check(*cases.spans_set(rng, [rng.integers(0, 20, bases).tolist()], 5, heads=[3]))
    _check(*cases.spans_set(rng, [rng.integers(0, 20, bases).tolist() for _ in range(3)], 5, heads=[0, 7, 1]))


def test_read_borders_and_heads_inside_one_wave(built):
    """Reads of 0 to 5 bases behind heads of 0 to 40 samples, some reads without a sample or without a base: a wave's 64 bases span
    a dozen reads, and its run of samples holds what lies between them."""
    rng = np.random.default_rng(2200)
    per_read = [rng.integers(0, 15, int(rng.integers(0, 6))).tolist() for _ in range(400)]
    heads = [int(h) for h in rng.integers(0, 41, 400)]
    per_read[5], heads[5] = [], 0                                  # neither a base nor a sample
    per_read[6], heads[6] = [], 3000                               # samples nobody owns, three pieces of them
    per_read[7], heads[7] = [0, 0, 0], 0                           # bases without a sample
    _check(*cases.spans_set(rng, per_read, 64, heads=heads))
    signals, starts, bins, n_bins = cases.random_set(rng, reads=300, n_bins=17, empty=0.3)
    _check(signals, starts, bins, n_bins)


def test_bins(built):
    rng = np.random.default_rng(2300)
    signals, starts, bins, n_bins = cases.spans_set(rng, [rng.integers(0, 9, 300).tolist() for _ in range(3)], 40)
    # every bin -1: the levels come, the planes stay clear
    planes, levels = _check(signals, starts, [np.full(300, -1, np.int32)] * 3, 40)
    assert not planes.any() and sum((lv != squiggle.EMPTY).sum() for lv in levels) > 700
    # 300 events on one bin, the rest of the call elsewhere
    full = cases.spans_set(rng, [rng.integers(1, 9, 300).tolist(), rng.integers(0, 9, 300).tolist()], 40)
    planes, _ = _check(full[0], full[1], [np.full(300, 13, np.int32), np.where(full[2][1] == 13, -1, full[2][1]).astype(np.int32)], 40)
    assert planes[0, 13] == 300
    # bins == 0: levels only, and no planes to hand in
    planes, levels = _check(signals, starts, [np.full(300, -1, np.int32)] * 3, 0)
    assert planes.shape == (4, 0) and len(levels) == 3
    # level_out NULL: planes only
    _check(signals, starts, bins, n_bins, want_levels=False)
    # neither: a call that computes and returns nothing, and one without a read whose planes are cleared
    assert squiggle.reduce_call(signals, starts, [np.full(300, -1, np.int32)] * 3, 0, want_levels=False)[1] is None
    planes, levels = squiggle.reduce_call([], [], [], 6)
    assert planes.shape == (4, 6) and not planes.any() and levels == []


def test_squared_sum_past_32_bits(built):
    """70,000 events of level -32768 on one bin: sum = -70000 * 2^15 and sq = 70000 * 2^30, far past 2^32."""
    rng = np.random.default_rng(2400)
    spans = rng.integers(1, 4, 70000)
    st = np.concatenate([[0], np.cumsum(spans)]).astype(np.int32)
    planes, levels = _check([np.full(int(st[-1]), -32768, np.int16)], [st], [np.full(70000, 2, np.int32)], 4)
    assert planes[:, 2].tolist() == [70000, int(spans.sum()), -70000 * 32768, 70000 * 32768 * 32768] and planes[3, 2] > 1 << 32
    assert (levels[0] == -32768).all()


@pytest.mark.parametrize("bases", [600000, 2 * squiggle.THREADS * squiggle.MAX_GROUPS + 777])
def test_more_bases_than_the_launch_has_lanes(built, bases):
    """One launch holds THREADS x MAX_GROUPS lanes, a base each.  600,000 bases of 1 to 3 samples make some waves take a second chunk
    of 64; twice the launch and 777 more make every wave take a second one and some a third."""
    assert bases > squiggle.THREADS * squiggle.MAX_GROUPS
    rng = np.random.default_rng(2500)
    reads = 40
    cut = np.sort(rng.choice(np.arange(1, bases), reads - 1, replace=False))
    lens = np.diff(np.concatenate([[0], cut, [bases]]))
    signals, starts, bins = [], [], []
    for n in lens:
        st = np.concatenate([[0], np.cumsum(rng.integers(1, 4, n))])
        signals.append(rng.integers(-32768, 32768, int(st[-1])).astype(np.int16))
        starts.append(st.astype(np.int32))
        bins.append(rng.integers(-1, 5000, n).astype(np.int32))
    planes, _ = _check(signals, starts, bins, 5000)
    assert planes[0].sum() > 0.99 * bases


def _planned_reads(rng, count, genome_len):
    reads = []
    for k in range(count):
        r = cases.random_read(rng, genome_len, name="r%d" % k, columns=int(rng.integers(30, 120)))
        r["starts"] = (int(rng.integers(0, 30)) + np.concatenate([[0], np.cumsum(rng.integers(0, 25, len(r["called"])))])).astype(np.int32)
        r["signal"] = rng.integers(-32768, 32768, int(r["starts"][-1]) + 5).astype(np.int16)
        reads.append(r)
    return reads


def test_a_read_contributes_the_same_alone_in_a_batch_and_across_tiles(built):
    rng = np.random.default_rng(2600)
    genome = cases.PlainGenome(rng.integers(0, 4, 500))
    reads = _planned_reads(rng, 40, 500)
    whole = squiggle.levels(reads, genome)
    want = squiggle.levels(reads, genome, reducer=ref.reduce_numpy)
    assert whole["tiles"] == 1 and np.array_equal(whole["planes"], want["planes"]) and whole["planes"][:, 0].sum() > 1500
    budget = squiggle.workspace_size(6, 6 * 1500, 6 * 120, 2 * 50)
    tiled = squiggle.levels(reads, genome, workspace_mb=budget / (1 << 20))
    assert tiled["tiles"] >= 5 and np.array_equal(tiled["planes"], whole["planes"])
    for a, b, c in zip(whole["levels"], tiled["levels"], want["levels"]):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    # alone: the batch is the sum of its reads, and a read's levels are its own
    total = np.zeros_like(whole["planes"])
    for i, r in enumerate(reads):
        alone = squiggle.levels([r], genome)
        total += alone["planes"]
        assert np.array_equal(alone["levels"][0], whole["levels"][i]), i
    assert np.array_equal(total, whole["planes"])
    # the k-mer planes in one run of reads and in planned runs
    km = squiggle.kmer_levels(reads, genome, 4)
    parts = squiggle.kmer_levels(reads, genome, 4, workspace_mb=squiggle.workspace_size(7, 7 * 1500, 7 * 120, 256, False) / (1 << 20))
    assert np.array_equal(km, parts) and np.array_equal(km, squiggle.kmer_levels(reads, genome, 4, reducer=ref.reduce_numpy)) and km[0].sum() > 1500


def test_two_runs_give_identical_bytes(built):
    rng = np.random.default_rng(2700)
    signals, starts, bins, n_bins = cases.random_set(rng, reads=200, n_bins=11)       # few bins: every atomic add meets others
    a = squiggle.reduce_call(signals, starts, bins, n_bins)
    b = squiggle.reduce_call(signals, starts, bins, n_bins)
    assert a[0].tobytes() == b[0].tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1]))


def test_workspace_contract(built, monkeypatch):
    """"Caller's memory" of include/chiron_amd.h for chiron_signal_levels: under each fill of tests/ws_guard.py the workspace is
    exactly the size function's bytes between two guards and holds the fill on entry, and so do the host outputs.  The guards are
    intact afterwards, no output element keeps the fill (the result equals the reference under all three, which an element left
    unwritten cannot), and the three results are the same bytes."""
    import torch
    rng = np.random.default_rng(2800)
    per_read = [rng.integers(0, 12, 150).tolist() + [PIECE + 1, 0, 5000] + rng.integers(0, 12, 40).tolist(), [], rng.integers(0, 12, 65).tolist()]
    signals, starts, bins, n_bins = cases.spans_set(rng, per_read, 23, heads=[5, 40, 0])
    samples, sample_off, start, base_off, bin_flat = ref.flatten(signals, starts, bins)
    n_bases = int(base_off[-1])
    want_planes, want_level = ref.reduce_flat(samples, sample_off, start, base_off, bin_flat, n_bins)
    results = []
    for fill in FILLS:
        for want_levels in (True, False):
            rec = Recorder(fill)
            monkeypatch.setattr(_lib, "alloc_hook", rec)
            try:
                lib, ws, stream = _lib.device_workspace(lambda: squiggle.workspace_size(len(signals), int(sample_off[-1]), n_bases, n_bins, want_levels),
                                                        0, "test", "level kernel")
                planes = np.full((4, n_bins), fill * 0x0101010101010101, dtype=np.uint64).view(np.int64)
                level = np.full(n_bases, fill * 0x01010101, dtype=np.uint32).view(np.int32)
                _lib.check(lib.chiron_signal_levels(0, samples.ctypes.data, sample_off.ctypes.data, start.ctypes.data, base_off.ctypes.data,
                                                    bin_flat.ctypes.data, len(signals), n_bins, 0, planes.ctypes.data,
                                                    level.ctypes.data if want_levels else None, ws.data_ptr(), stream))
            finally:
                monkeypatch.setattr(_lib, "alloc_hook", None)
            torch.cuda.synchronize()
            rec.check()
            assert rec.sizes == [squiggle.workspace_size(len(signals), int(sample_off[-1]), n_bases, n_bins, want_levels)]
            assert np.array_equal(planes, want_planes), fill
            if want_levels:
                assert np.array_equal(level, want_level), fill
                results.append(planes.tobytes() + level.tobytes())
            else:
                assert (level.view(np.uint32) == fill * 0x01010101).all()          # NULL level_out: nothing is written there
    assert len(results) == 3 and results[0] == results[1] == results[2]


def test_planted_modification_on_the_gpu(built):
    """The planted case with the case's own forced alignment and the reduction on the GPU: the planes, the levels and every row of
    `compare` equal the reference pipeline's, and the five largest |t| are forward 298 .. 302."""
    case = cases.planted()
    got, want = {}, {}
    for s in "ab":
        kw = dict(frame_aligner=cases.frame_aligner_of(case[s]), kmer=5)
        got[s] = squiggle.sample(case[s], case["genome"], cases.SEGMENT_LEN, cases.RATIO, **kw)
        want[s] = squiggle.sample(case[s], case["genome"], cases.SEGMENT_LEN, cases.RATIO, reducer=ref.reduce_numpy, **kw)
        assert np.array_equal(got[s]["planes"], want[s]["planes"]) and np.array_equal(got[s]["kmer_planes"], want[s]["kmer_planes"])
        assert all(np.array_equal(a, b) for a, b in zip(got[s]["levels"], want[s]["levels"])) and got[s]["report"] == want[s]["report"]
    a = squiggle.compare(got["a"]["planes"].transpose(1, 0, 2), got["b"]["planes"].transpose(1, 0, 2), 5)
    b = squiggle.compare(want["a"]["planes"].transpose(1, 0, 2), want["b"]["planes"].transpose(1, 0, 2), 5)
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in b) and set(a) == set(b)
    assert squiggle.compare_lines(a, case["genome"]) == squiggle.compare_lines(b, case["genome"])
    t = np.where(a["keep"], np.abs(a["t"]), -1.0).reshape(-1)
    assert sorted(np.argsort(-t)[:5].tolist()) == [298, 299, 300, 301, 302]


def test_squiggle_command(built, tmp_path):
    """`chiron squiggle --synthetic-weights` on a tiny `call` + `map --cigar` tree: signals under raw/, a mapped.sam whose reads
    carry those names.  With synthetic weights the frame alignment means nothing; the command's plumbing is what is run.  The
    control is the sample itself: every compared position has t = 0."""
    import chiron_amd as ca
    rng = np.random.default_rng(2900)
    seq = "".join("ACGT"[v] for v in rng.integers(0, 4, 400))
    (tmp_path / "genome.fa").write_text(">ctg\n%s\n" % seq)
    raw = tmp_path / "call" / "raw"
    raw.mkdir(parents=True)
    lines = ["@HD\tVN:1.6\tSO:unknown", "@SQ\tSN:ctg\tLN:400"]
    complement = {"A": "T", "C": "G", "G": "C", "T": "A"}
    for k in range(6):
        start = 20 * k
        piece = list(seq[start:start + 120])
        piece[40] = complement[piece[40]]
        piece = "".join(piece)
        sig = ca.synthetic_signal(1, 1500, seed=60 + k)[0]
        (raw / ("read%d.signal" % k)).write_text(" ".join(str(int(v)) for v in sig))
        lines.append("\t".join(["read%d" % k, "16" if k % 2 else "0", "ctg", str(start + 1), "255", "40=1X79=", "*", "0", "0", piece, "*", "NM:i:1"]))
    lines.append("\t".join(["nosig", "0", "ctg", "1", "255", "50=", "*", "0", "0", seq[:50], "*", "NM:i:0"]))
    (tmp_path / "map").mkdir()
    (tmp_path / "map" / "mapped.sam").write_text("".join(ln + "\n" for ln in lines))
    common = ["-s", str(tmp_path / "call"), "-g", str(tmp_path / "genome.fa"), "--synthetic-weights", "-b", "8"]
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, "-m", "chiron_amd.entry", "squiggle", "-i", str(tmp_path / "map"), "-o", str(out), "--control",
                        str(tmp_path / "map" / "mapped.sam"), "--control-signal", str(tmp_path / "call"), "--kmer", "3", "--events",
                        "--min-events", "2"] + common, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    report = json.loads((out / "squiggle_report.json").read_text())
    rd = report["reads"]
    assert rd["total"] == 7 and rd["dropped"]["no_signal"] == 1 and rd["total"] == rd["used"] + sum(rd["dropped"].values()) and rd["used"] >= 1
    assert set(rd["dropped"]) == set(squiggle.READ_DROPS) and report["tiles"] >= 1 and report["kmer"] == 3 and report["normalize"] == "mad"
    assert report["bases"] == 120 * rd["used"] and report["samples"] == 1500 * rd["used"] and report["control"]["reads"] == rd
    assert "squiggle: %d of 7 reads used" % rd["used"] in r.stdout
    rows = [ln.split("\t") for ln in (out / "levels.tsv").read_text().splitlines()]
    assert rows[0] == list(squiggle.LEVEL_COLUMNS) and all(len(row) == len(rows[0]) for row in rows)
    assert sum(int(row[4]) for row in rows[1:]) == report["events"] <= report["bases"] and all(row[0] == "ctg" and row[2] in "+-" for row in rows[1:])
    assert all(seq[int(row[1]) - 1] == row[3] for row in rows[1:])
    rows = [ln.split("\t") for ln in (out / "compare.tsv").read_text().splitlines()]
    assert rows[0] == list(squiggle.COMPARE_COLUMNS) and len(rows) == 1 + report["compared"]
    assert all(float(row[10]) == 0 and float(row[12]) == 0 and row[4] == row[7] for row in rows[1:])
    rows = [ln.split("\t") for ln in (out / "kmer_levels.tsv").read_text().splitlines()]
    assert rows[0] == list(squiggle.KMER_COLUMNS) and len(rows) == 1 + report["kmers_seen"] <= 65 and all(len(row[0]) == 3 for row in rows[1:])
    names = sorted(os.listdir(str(out / "events")))
    assert len(names) == rd["used"] == report["event_files"] and "nosig.tsv" not in names
    rows = [ln.split("\t") for ln in (out / "events" / names[0]).read_text().splitlines()]
    assert rows[0] == list(squiggle.EVENT_COLUMNS) and len(rows) == 121 and sum(row[3] == "ctg" for row in rows[1:]) == 120
    assert sum(int(row[1]) for row in rows[1:]) + int(rows[1][0]) == 1500                   # the spans tile the read behind its head
    assert sorted(report["files"]) == ["compare.tsv", "kmer_levels.tsv", "levels.tsv"]
    # a directory of `map` without --cigar is told so
    (tmp_path / "plain").mkdir()
    r = subprocess.run([sys.executable, "-m", "chiron_amd.entry", "squiggle", "-i", str(tmp_path / "plain"), "-o", str(tmp_path / "o2")] + common,
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--cigar" in r.stderr
