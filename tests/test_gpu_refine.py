"""GPU: chiron_signal_refine (csrc/refine.hip) through chiron_amd.squiggle against tests/refine_ref.py's numpy formulation of the
definition (which tests/test_refine_cpu.py holds to the plain-Python one and to a brute force), and `sample(..., refine=...)` end to
end.  Every result is a property of the inputs: every comparison is exact."""
import os

import numpy as np
import pytest

from chiron_amd import _lib, squiggle

import refine_cases as cases
import refine_ref as ref
import squiggle_cases
import squiggle_ref
from ws_guard import FILLS, Recorder

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(signals, levels, starts):
    """One call against the reference, every start and every cost.  -> (starts, costs) of the GPU."""
    got, cost = squiggle.refine_call(signals, levels, starts)
    want, want_cost = ref.refine(signals, levels, starts)
    assert cost.dtype == np.int64 and cost.shape == (len(signals),) and len(got) == len(signals)
    bad = np.flatnonzero(cost != want_cost)
    assert len(bad) == 0, (bad[:5].tolist(), cost[bad[:5]].tolist(), want_cost[bad[:5]].tolist())
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == np.int32 and a.shape == b.shape, i
        bad = np.flatnonzero(a != b)
        assert len(bad) == 0, (i, bad[:5].tolist(), a[bad[:5]].tolist(), b[bad[:5]].tolist())
    return got, cost


def _both_outcomes(cost):
    return bool((cost == squiggle.INFEASIBLE).any()) and bool((cost != squiggle.INFEASIBLE).any())


def test_random_items(built):
    """200 items of 1 .. 40 bases with empty spans, heads and tails, feasible and infeasible in one call; the cost is the cost of
    the starts that came with it, and never above that of strictly increasing initial starts."""
    rng = np.random.default_rng(3000)
    signals, levels, starts = cases.random_items(rng, 200)
    got, cost = _check(signals, levels, starts)
    assert _both_outcomes(cost)
    improved = 0
    for x, e, a, s, c in zip(signals, levels, starts, got, cost):
        if c == squiggle.INFEASIBLE:
            assert np.array_equal(s, a)
            continue
        assert ref.cost_of(x, e, s) == c and (np.diff(s) > 0).all() and s[0] == a[0] and s[-1] == a[-1]
        if (np.diff(a) > 0).all():
            assert c <= ref.cost_of(x, e, a)
            improved += int(c < ref.cost_of(x, e, a))
    assert improved > 20


SHIFTS = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 5000]


@pytest.mark.parametrize("where", ["middle", "first", "last"])
def test_window_shift(built, where):
    """a[n] - a[n-1] at every value at which the row takes another number of pieces or another lane of them, at a middle base, at
    the first and at the last."""
    rng = np.random.default_rng(3100)
    signals, levels, starts = [], [], []
    for d in SHIFTS:
        for wide in (False, True):
            spans = rng.integers(1, 12, 11)
            spans[{"middle": 5, "first": 0, "last": 10}[where]] = d
            x, e, a = cases.item_of(rng, spans, int(rng.integers(0, 4)), int(rng.integers(0, 4)), wide)
            signals.append(x)
            levels.append(e)
            starts.append(a)
    _, cost = _check(signals, levels, starts)
    assert (cost != squiggle.INFEASIBLE).sum() >= 2 * (len(SHIFTS) - 1)


def test_crowded_starts(built):
    """Runs of bases that start in one sample, with and without the room to spread them."""
    rng = np.random.default_rng(3200)
    signals, levels, starts = [], [], []
    for run in (2, 31, 32, 33, 63, 64, 65, 70):
        for before, after in ((100, 100), (100, 3), (3, 100), (3, 3), (40, 40)):
            spans = [5, before] + [0] * (run - 1) + [after, 5]
            x, e, a = cases.item_of(rng, spans, 2, 2)
            signals.append(x)
            levels.append(e)
            starts.append(a)
    _, cost = _check(signals, levels, starts)
    assert _both_outcomes(cost)


@pytest.mark.parametrize("bases", [1, 2, 63, 64, 65, 300])
def test_tight_items(built, bases):
    """S = L and S = L + 1: one sample a base, and one base with two; from the right starts and from sorted random ones."""
    rng = np.random.default_rng(3300 + bases)
    signals, levels, starts = [], [], []
    for extra in (0, 1):
        spans = np.ones(bases, dtype=np.int64)
        spans[int(rng.integers(0, bases))] += extra
        x, e, a = cases.item_of(rng, spans, 0, 0)
        for k in range(3):
            signals.append(x)
            levels.append(e)
            guess = np.sort(rng.integers(0, len(x) + 1, bases + 1)) if k else a
            guess[0], guess[-1] = 0, len(x)
            starts.append(guess.astype(np.int32))
    got, cost = _check(signals, levels, starts)
    assert cost[0] != squiggle.INFEASIBLE and np.array_equal(got[0], np.arange(bases + 1))


@pytest.mark.parametrize("bases", [2, 5, 70])
def test_ties(built, bases):
    """A constant signal against a constant level: every assignment costs the same, the tie rule alone decides."""
    rng = np.random.default_rng(3400 + bases)
    signals, levels, starts = [], [], []
    for k in range(4):
        a = np.concatenate([[0], np.cumsum(rng.integers(1, 12, bases))]).astype(np.int32)
        signals.append(np.full(int(a[-1]), 7, np.int16))
        levels.append(np.full(bases, 7 if k % 2 else 3, np.int32))
        starts.append(a)
    got, cost = _check(signals, levels, starts)
    assert cost[1] == 0 and cost[0] == 4 * len(signals[0])
    assert any(not np.array_equal(s, a) for s, a in zip(got, starts))


def test_cost_past_32_bits(built):
    """Samples of 32767 against levels of -32767, and the reverse: 70,000 samples cost 70,000 x 65534, past 2^32."""
    rng = np.random.default_rng(3500)
    a = np.concatenate([[0], np.cumsum(rng.multinomial(70000 - 700, np.ones(700) / 700) + 1)]).astype(np.int32)
    signals = [np.full(70000, 32767, np.int16), np.full(70000, -32767, np.int16)]
    levels = [np.full(700, -32767, np.int32), np.full(700, 32767, np.int32)]
    _, cost = _check(signals, levels, [a, a])
    assert cost.tolist() == [70000 * 65534] * 2 and cost[0] > 1 << 32


def test_more_items_than_waves(built):
    """More items than the launch has waves, so that waves take a second and a third item: 20,000 two-base items between two long
    ones."""
    waves = _lib.REFINE_THREADS // 64 * _lib.REFINE_MAX_GROUPS
    header = open(os.path.join(ROOT, "include", "chiron_amd.h")).read()
    for name in ("THREADS", "MAX_GROUPS", "HALF"):
        assert int(header.split("#define CHIRON_REFINE_%s " % name)[1].split()[0]) == getattr(_lib, "REFINE_" + name)
    rng = np.random.default_rng(3600)
    count = 20000
    assert count > 2 * waves
    signals, levels, starts = [], [], []
    for k in range(count + 2):
        spans = rng.integers(1, 12, 500) if k in (0, count + 1) else rng.integers(0, 9, 2)
        x, e, a = cases.item_of(rng, spans, int(rng.integers(0, 3)), int(rng.integers(0, 3)))
        signals.append(x)
        levels.append(e)
        starts.append(a)
    _, cost = _check(signals, levels, starts)
    assert _both_outcomes(cost) and cost[0] != squiggle.INFEASIBLE and cost[-1] != squiggle.INFEASIBLE


def test_odd_offsets(built):
    """Items of odd sample counts: every item but the first starts at an odd or an even sample in turn."""
    rng = np.random.default_rng(3700)
    signals, levels, starts = [], [], []
    for k in range(60):
        spans = rng.integers(1, 12, int(rng.integers(1, 80)))
        x, e, a = cases.item_of(rng, spans, 1, 0)
        if len(x) % 2 == 0:
            x = np.concatenate([x, x[:1]])
        signals.append(x)
        levels.append(e)
        starts.append(a)
    assert all(len(x) % 2 == 1 for x in signals)
    _check(signals, levels, starts)


def test_empty_calls(built):
    got, cost = squiggle.refine_call([], [], [])
    assert got == [] and cost.shape == (0,)
    got, cost = _check([np.arange(5, dtype=np.int16), np.zeros(0, np.int16)], [np.zeros(0, np.int32)] * 2, [np.array([3], np.int32), np.array([0], np.int32)])
    assert [g.tolist() for g in got] == [[3], [0]] and cost.tolist() == [0, 0]
    # an item without a base among items with bases
    rng = np.random.default_rng(3800)
    signals, levels, starts = cases.random_items(rng, 5)
    signals.insert(2, np.arange(4, dtype=np.int16))
    levels.insert(2, np.zeros(0, np.int32))
    starts.insert(2, np.array([4], np.int32))
    got, cost = _check(signals, levels, starts)
    assert got[2].tolist() == [4] and cost[2] == 0


def test_workspace_contract(built, monkeypatch):
    """"Caller's memory" of include/chiron_amd.h for chiron_signal_refine: under each fill of tests/ws_guard.py the workspace is
    exactly the size function's bytes between two guards and holds the fill on entry, and so do the host outputs.  The guards are
    intact afterwards, the result equals the reference under all three (which an element left unwritten cannot), and the three
    results are the same bytes."""
    import torch
    rng = np.random.default_rng(3900)
    signals, levels, starts = cases.random_items(rng, 40)
    x, e, a = cases.item_of(rng, [5, 3, 200, 0, 0, 7, 5000, 2] + rng.integers(1, 12, 150).tolist(), 3, 2)
    crowded = cases.item_of(rng, [0, 0, 0, 0, 0, 2], 1, 1)                               # six bases on two samples: no solution
    signals, levels, starts = (signals + [x, np.zeros(2, np.int16), crowded[0]], levels + [e, np.zeros(0, np.int32), crowded[1]],
                               starts + [a, np.array([1], np.int32), crowded[2]])
    samples, sample_off, level, start, base_off = ref.flatten(signals, levels, starts)
    items, n_bases = len(signals), int(base_off[-1])
    want, want_cost = ref.refine(signals, levels, starts)
    want = np.concatenate(want)
    assert _both_outcomes(want_cost)
    results = []
    for fill in FILLS:
        rec = Recorder(fill)
        monkeypatch.setattr(_lib, "alloc_hook", rec)
        try:
            lib, ws, stream = _lib.device_workspace(lambda: squiggle.refine_workspace_size(items, int(sample_off[-1]), n_bases), 0, "test", "refine kernel")
            out = np.full(n_bases + items, fill * 0x01010101, dtype=np.uint32).view(np.int32)
            cost = np.full(items, fill * 0x0101010101010101, dtype=np.uint64).view(np.int64)
            _lib.check(lib.chiron_signal_refine(0, samples.ctypes.data, sample_off.ctypes.data, level.ctypes.data, start.ctypes.data, base_off.ctypes.data,
                                                items, 0, out.ctypes.data, cost.ctypes.data, ws.data_ptr(), stream))
        finally:
            monkeypatch.setattr(_lib, "alloc_hook", None)
        torch.cuda.synchronize()
        rec.check()
        assert rec.sizes == [squiggle.refine_workspace_size(items, int(sample_off[-1]), n_bases)]
        assert np.array_equal(out, want) and np.array_equal(cost, want_cost), fill
        results.append(out.tobytes() + cost.tobytes())
    assert len(results) == 3 and results[0] == results[1] == results[2]


def test_planted_borders_on_the_gpu(built):
    """The planted case with jittered borders through squiggle.sample(..., refine=...): the refined starts, the planes, the levels
    and the report equal those with refiner= set to the reference."""
    case = cases.planted(squiggle_cases.PLANTED_SEED)
    genome = case["genome"]
    kw = dict(reducer=squiggle_ref.reduce_numpy)
    control = squiggle.sample(case["b"], genome, squiggle_cases.SEGMENT_LEN, squiggle_cases.RATIO, frame_aligner=squiggle_cases.frame_aligner_of(case["b"]),
                              kmer=5, **kw)
    table = squiggle.table_of(control["kmer_planes"], 5)
    for s in ("a_jit", "b_jit"):
        kw = dict(frame_aligner=squiggle_cases.frame_aligner_of(case[s]), refine=(table, 5))
        got = squiggle.sample(case[s], genome, squiggle_cases.SEGMENT_LEN, squiggle_cases.RATIO, **kw)
        want = squiggle.sample(case[s], genome, squiggle_cases.SEGMENT_LEN, squiggle_cases.RATIO, reducer=squiggle_ref.reduce_numpy, refiner=ref.refine, **kw)
        assert len(got["reads"]) == len(want["reads"]) == 30
        assert all(np.array_equal(a["starts"], b["starts"]) for a, b in zip(got["reads"], want["reads"]))
        assert np.array_equal(got["planes"], want["planes"]) and all(np.array_equal(a, b) for a, b in zip(got["levels"], want["levels"]))
        assert got["report"] == want["report"] and got["report"]["refine"]["moved"] > 4000


def test_squiggle_command_refines_in_two_passes(built, tmp_path):
    """`chiron squiggle --kmer 3`, then `--refine <its kmer_levels.tsv>` on the same tiny tree, sample and control alike.  With
    synthetic weights the frame alignment means nothing; the command's plumbing is what is run: the table is read, both samples
    are refined before anything is summed, and the report says so."""
    import json
    import subprocess
    import sys
    import chiron_amd as ca
    rng = np.random.default_rng(4100)
    seq = "".join("ACGT"[v] for v in rng.integers(0, 4, 400))
    (tmp_path / "genome.fa").write_text(">ctg\n%s\n" % seq)
    raw = tmp_path / "call" / "raw"
    raw.mkdir(parents=True)
    lines = ["@HD\tVN:1.6\tSO:unknown", "@SQ\tSN:ctg\tLN:400"]
    for k in range(6):
        start = 20 * k
        sig = ca.synthetic_signal(1, 1500, seed=60 + k)[0]
        (raw / ("read%d.signal" % k)).write_text(" ".join(str(int(v)) for v in sig))
        lines.append("\t".join(["read%d" % k, "16" if k % 2 else "0", "ctg", str(start + 1), "255", "120=", "*", "0", "0", seq[start:start + 120], "*", "NM:i:0"]))
    (tmp_path / "map").mkdir()
    (tmp_path / "map" / "mapped.sam").write_text("".join(ln + "\n" for ln in lines))
    common = ["-i", str(tmp_path / "map"), "-s", str(tmp_path / "call"), "-g", str(tmp_path / "genome.fa"), "--synthetic-weights", "-b", "8", "--kmer", "3"]
    run = lambda extra: subprocess.run([sys.executable, "-m", "chiron_amd.entry", "squiggle"] + common + extra, cwd=ROOT, capture_output=True, text=True,
                                       timeout=300)
    r = run(["-o", str(tmp_path / "one")])
    assert r.returncode == 0, r.stderr
    first = json.loads((tmp_path / "one" / "squiggle_report.json").read_text())
    assert "refine" not in first and first["reads"]["used"] >= 1
    table = str(tmp_path / "one" / "kmer_levels.tsv")
    r = run(["-o", str(tmp_path / "two"), "--refine", table, "--refine-min-events", "2", "--events", "--control", str(tmp_path / "map"), "--control-signal",
             str(tmp_path / "call"), "--min-events", "2"])
    assert r.returncode == 0, r.stderr
    report = json.loads((tmp_path / "two" / "squiggle_report.json").read_text())
    ref_ = report["refine"]
    k, levels = squiggle.load_level_table(table, 2)
    assert k == 3 and ref_["table"] == table and ref_["k"] == 3 and ref_["min_events"] == 2 and ref_["kmers_known"] == int((levels != squiggle.UNKNOWN).sum()) > 0
    assert set(squiggle.REFINE_COUNTS) <= set(ref_) and ref_["items"] >= 1 and ref_["bases"] <= report["bases"] and ref_["infeasible"] <= ref_["items"]
    assert 0 <= ref_["moved"] <= ref_["borders"] < ref_["bases"] + 1
    control = report["control"]["refine"]
    assert {key: control[key] for key in squiggle.REFINE_COUNTS} == {key: ref_[key] for key in squiggle.REFINE_COUNTS}     # the control is the sample itself
    rows = [ln.split("\t") for ln in (tmp_path / "two" / "compare.tsv").read_text().splitlines()]
    assert len(rows) == 1 + report["compared"] and all(float(row[10]) == 0 for row in rows[1:])
    # the events tile each read as before, and a refined item gives every base of it a sample
    names = sorted(os.listdir(str(tmp_path / "two" / "events")))
    rows = [ln.split("\t") for ln in (tmp_path / "two" / "events" / names[0]).read_text().splitlines()]
    assert len(rows) == 121 and sum(int(row[1]) for row in rows[1:]) + int(rows[1][0]) == 1500
    # a file that is no table is refused before the engine starts
    r = run(["-o", str(tmp_path / "three"), "--refine", str(tmp_path / "genome.fa")])
    assert r.returncode != 0 and "kmer_levels.tsv" in r.stderr
