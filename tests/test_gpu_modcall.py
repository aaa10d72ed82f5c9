"""GPU: chiron_signal_score (csrc/site_score.hip) through chiron_amd.modcall against tests/site_ref.py's numpy formulation of the
definition (which tests/test_modcall_cpu.py holds to the plain-Python one and to a brute force), and `modcall` end to end.  Every
result is a property of the inputs: every comparison is exact."""
import json
import os

import numpy as np
import pytest

from chiron_amd import _lib, modcall, squiggle

import modcall_cases as cases
import site_ref as ref
from ws_guard import FILLS, Recorder

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(segments, candidates):
    """One call against the reference, every cost.  -> the GPU's costs."""
    got = modcall.score_call(segments, candidates)
    want = ref.score(segments, candidates)
    assert got.dtype == np.int32 and got.shape == (len(candidates),)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())
    return got


def _both_outcomes(cost):
    return bool((cost == modcall.INFEASIBLE).any()) and bool((cost != modcall.INFEASIBLE).any())


def test_every_width_at_every_length(built):
    """Every L in 1 .. 16 against S in {1, L - 1, L, L + 1, 63, 64, 65, 127, 128, 129, 4096}: the lengths at which a lane starts
    another piece of 64 samples, the shortest feasible and the longest infeasible one, and the cap.  At 4096 the samples are -32768
    and the levels 32767, so the cost is 4096 * 65535, the largest there is."""
    rng = np.random.default_rng(7000)
    segments, candidates = [], []
    for L in range(1, 17):
        for S in sorted({1, L - 1, L, L + 1, 63, 64, 65, 127, 128, 129, 4096}):
            wide = bool(rng.integers(0, 2))
            segments.append(np.full(S, -32768, np.int16) if S == 4096 else cases.samples_of(rng, S, wide))
            candidates.append((len(segments) - 1, np.full(L, 32767, np.int32) if S == 4096 else cases.levels_of(rng, L, wide)))
    got = _check(segments, candidates)
    assert _both_outcomes(got) and (got == 4096 * 65535).sum() == 16 and (1 << 27) < 4096 * 65535 < (1 << 28)
    for (g, e), c in zip(candidates, got):
        assert (c == modcall.INFEASIBLE) == (len(segments[g]) < len(e))


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_candidate_counts(built, count):
    """A wave with one lane, one lane short, full, one lane into the second wave, and one into the second workgroup."""
    rng = np.random.default_rng(7100 + count)
    _check(*cases.random_call(rng, max(count // 3, 1), count, max_samples=140))


def test_a_wave_of_mixed_lanes(built):
    """64 candidates, a lane each, whose S runs from 1 to 300 and whose L from 1 to 16: lanes that stop early keep their rows while
    the wave runs on, and columns past a lane's L are computed and ignored."""
    rng = np.random.default_rng(7200)
    S = rng.permutation(np.concatenate([[1, 300, 2, 299], rng.integers(1, 301, 60)]))
    L = rng.permutation(np.concatenate([np.arange(1, 17)] * 4))
    segments = [cases.samples_of(rng, int(s), bool(k % 2)) for k, s in enumerate(S)]
    candidates = [(k, cases.levels_of(rng, int(n), bool(k % 2))) for k, n in enumerate(L)]
    assert _both_outcomes(_check(segments, candidates))


def test_one_segment_for_a_whole_wave(built):
    """64 candidates on one segment: one row of the slice, every lane reads the same address; then 64 and one more on two."""
    rng = np.random.default_rng(7300)
    x = cases.samples_of(rng, 150, True)
    got = _check([x], [(0, cases.levels_of(rng, int(rng.integers(1, 17)), True)) for _ in range(64)])
    assert len(set(got.tolist())) > 32
    y = cases.samples_of(rng, 70, False)
    _check([x, y], [(k % 2, cases.levels_of(rng, int(rng.integers(1, 17)), k % 2 == 0)) for k in range(129)])


def test_shuffled_segment_order(built):
    """Candidates that name their segments in no order, so that a wave's lanes of one segment are not neighbours, and a segment
    shows up in several waves."""
    rng = np.random.default_rng(7400)
    segments, candidates = cases.random_call(rng, 90, 400, max_samples=200)
    order = rng.permutation(len(candidates))
    got = _check(segments, [candidates[k] for k in order])
    assert np.array_equal(got, ref.score(segments, candidates)[order]) and _both_outcomes(got)


def test_segments_without_a_candidate_and_empty_segments(built):
    rng = np.random.default_rng(7500)
    segments = [cases.samples_of(rng, n, True) for n in (0, 50, 0, 0, 200, 7, 0, 64, 0)]
    candidates = [(g, cases.levels_of(rng, L, True)) for g, L in ((0, 1), (4, 16), (2, 3), (7, 16), (7, 1), (8, 2), (4, 1))]      # 1, 3, 5 and 6 have none
    got = _check(segments, candidates)
    assert (got == modcall.INFEASIBLE).tolist() == [True, False, True, False, False, True, False]
    assert modcall.score_call([], []).shape == (0,) and modcall.score_call(segments, []).shape == (0,)


def test_more_candidates_than_the_launch_has_lanes(built):
    """2048 * 256 + 1 candidates of one level on one sample, spread over 1000 segments: the launch's lanes take a second candidate,
    and the last wave's second batch has one lane."""
    lanes = _lib.SITE_THREADS * _lib.SITE_MAX_GROUPS
    header = open(os.path.join(ROOT, "include", "chiron_amd.h")).read()
    for name in ("THREADS", "MAX_GROUPS", "MAX_SAMPLES", "MAX_COLUMNS"):
        assert int(header.split("#define CHIRON_SITE_%s " % name)[1].split()[0]) == getattr(_lib, "SITE_" + name)
    rng = np.random.default_rng(7600)
    count = lanes + 1
    assert count == 2048 * 256 + 1
    x = cases.samples_of(rng, 1000, True)
    seg = rng.integers(0, 1000, count).astype(np.int32)
    level = cases.levels_of(rng, count, True)
    off = np.arange(count + 1, dtype=np.int64)
    sample_off = np.arange(1001, dtype=np.int64)
    want = np.abs(x.astype(np.int64)[seg] - level).astype(np.int32)
    assert np.array_equal(ref.score_flat(x, sample_off, level, off, seg), want)
    cost = np.zeros(count, np.int32)
    need = modcall.score_workspace_size(1000, 1000, count, count)
    lib, ws, stream = _lib.device_workspace(need, 0, "test", "site kernel")
    _lib.check(lib.chiron_signal_score(0, x.ctypes.data, sample_off.ctypes.data, 1000, level.ctypes.data, off.ctypes.data, seg.ctypes.data, count,
                                       cost.ctypes.data, ws.data_ptr(), need, 0, stream))
    bad = np.flatnonzero(cost != want)
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), bad[-5:].tolist())


def test_workspace_contract(built, monkeypatch):
    """"Caller's memory" of include/chiron_amd.h for chiron_signal_score: under each fill of tests/ws_guard.py the workspace is
    exactly the size function's bytes between two guards and holds the fill on entry, and so does the host output.  The guards are
    intact afterwards, the result equals the reference under all three (which an element left unwritten cannot), and the three
    results are the same bytes.  A workspace said to be one byte short is refused before anything is written.  The offsets start
    above 0: what lies in front of them belongs to nobody."""
    import torch
    rng = np.random.default_rng(7700)
    segments, candidates = cases.random_call(rng, 40, 300, max_samples=260)
    segments += [np.zeros(0, np.int16), cases.samples_of(rng, 129, True)]
    candidates += [(40, np.array([5], np.int32)), (41, cases.levels_of(rng, 16, True)), (41, cases.levels_of(rng, 1, True))]
    samples, sample_off, level, level_off, seg = ref.flatten(segments, candidates)
    want = ref.score(segments, candidates)
    assert _both_outcomes(want)
    samples, sample_off = np.ascontiguousarray(np.concatenate([np.full(3, 999, np.int16), samples])), sample_off + 3
    level, level_off = np.ascontiguousarray(np.concatenate([np.full(5, squiggle.UNKNOWN, np.int32), level])), level_off + 5
    n_seg, n_cand = len(segments), len(candidates)
    need = modcall.score_workspace_size(n_seg, int(sample_off[-1] - sample_off[0]), n_cand, int(level_off[-1] - level_off[0]))
    results = []
    for fill in FILLS:
        rec = Recorder(fill)
        monkeypatch.setattr(_lib, "alloc_hook", rec)
        try:
            lib, ws, stream = _lib.device_workspace(need, 0, "test", "site kernel")
            out = np.full(n_cand, fill * 0x01010101, dtype=np.uint32).view(np.int32)
            before = out.copy()
            args = (0, samples.ctypes.data, sample_off.ctypes.data, n_seg, level.ctypes.data, level_off.ctypes.data, seg.ctypes.data, n_cand, out.ctypes.data,
                    ws.data_ptr())
            st = lib.chiron_signal_score(*args, need - 1, 0, stream)
            assert st == _lib.ERR_INVALID and ("a workspace of %d bytes, %d are needed" % (need - 1, need)) in lib.chiron_last_error().decode()
            assert np.array_equal(out, before)
            _lib.check(lib.chiron_signal_score(*args, need, 0, stream))
        finally:
            monkeypatch.setattr(_lib, "alloc_hook", None)
        torch.cuda.synchronize()
        rec.check()
        assert rec.sizes == [need]
        assert np.array_equal(out, want), fill
        results.append(out.tobytes())
    assert len(results) == 3 and results[0] == results[1] == results[2]


def test_planted_case_on_the_gpu(built, tmp_path):
    """The planted case at seed 3 with the scorer on the GPU: the rows, and mod_calls.tsv, mod_sites.tsv and the report written from
    them, equal those with scorer= set to the reference.  What the calls say about the planted states is the reference's business
    (tests/test_modcall_cpu.py); the GPU's bar is equality with it."""
    case = cases.planted(cases.PLANTED_SEED)
    tables = cases.tables_of(case)
    for name in ("a_jit", "b_jit"):
        kept = cases.prepared(case[name])
        got = modcall.modcall(kept, case["genome"], tables, cases.K)
        want = modcall.modcall(kept, case["genome"], tables, cases.K, scorer=ref.score)
        assert got == want and len(got["rows"]) > 300 and got["batches"] == 1
        meta = {"min_delta": modcall.MIN_DELTA, "reads": {"total": 30, "used": 30}}
        a = modcall.write_outputs(str(tmp_path / (name + "_gpu")), got, case["genome"], meta)
        b = modcall.write_outputs(str(tmp_path / (name + "_ref")), want, case["genome"], meta)
        assert a == b
        for f in ("mod_calls.tsv", "mod_sites.tsv", "modcall_report.json"):
            assert (tmp_path / (name + "_gpu") / f).read_bytes() == (tmp_path / (name + "_ref") / f).read_bytes(), f
        assert len((tmp_path / (name + "_gpu") / "mod_calls.tsv").read_text().splitlines()) == 1 + len(got["rows"])
    # the same reads in several calls
    small = modcall.modcall(kept, case["genome"], tables, cases.K, workspace_mb=0.02)
    assert small["batches"] > 3 and dict(small, batches=1) == want


def test_modcall_command_from_files(built, tmp_path):
    """`chiron modcall` on a tiny tree -- a SAM, .signal files, a genome and two kmer_levels.tsv -- once on the GPU and once with
    scorer= set to the reference: the three files are the same bytes.  With synthetic weights the frame alignment means nothing; the
    command's plumbing is what is run: both tables are read, the reads are prepared as squiggle prepares them, and the report says
    what was done.  Two tables of different k are refused before the engine starts."""
    import chiron_amd as ca
    from chiron_amd import entry
    rng = np.random.default_rng(7800)
    seq = "".join("ACGT"[v] for v in rng.integers(0, 4, 400))
    (tmp_path / "genome.fa").write_text(">ctg\n%s\n" % seq)
    raw = tmp_path / "call" / "raw"
    raw.mkdir(parents=True)
    lines = ["@HD\tVN:1.6\tSO:unknown", "@SQ\tSN:ctg\tLN:400"]
    for k in range(6):
        start = 20 * k
        sig = ca.synthetic_signal(1, 1500, seed=80 + k)[0]
        (raw / ("read%d.signal" % k)).write_text(" ".join(str(int(v)) for v in sig))
        lines.append("\t".join(["read%d" % k, "16" if k % 2 else "0", "ctg", str(start + 1), "255", "120=", "*", "0", "0",
                                seq[start:start + 120], "*", "NM:i:0"]))
    (tmp_path / "map").mkdir()
    (tmp_path / "map" / "mapped.sam").write_text("".join(ln + "\n" for ln in lines))
    for name, k in (("table", 3), ("alt", 3), ("other", 2)):
        rows = ["\t".join(squiggle.KMER_COLUMNS) + "\n"]
        for code in range(4 ** k):
            rows.append("%s\t9\t9.000\t%.5f\t0.10000\n" % ("".join("ACGT"[(code >> (2 * (k - 1 - j))) & 3] for j in range(k)), rng.normal(0, 1.0)))
        (tmp_path / (name + ".tsv")).write_text("".join(rows))
    argv = ["modcall", "-i", str(tmp_path / "map"), "-s", str(tmp_path / "call"), "-g", str(tmp_path / "genome.fa"), "--synthetic-weights", "-b", "8",
            "--table", str(tmp_path / "table.tsv"), "--alt-table", str(tmp_path / "alt.tsv"), "--min-delta", "2"]
    got = entry.main(argv + ["-o", str(tmp_path / "gpu")])
    args = entry.build_parser().parse_args(argv + ["-o", str(tmp_path / "ref")])
    want = modcall.modcall_command(args, scorer=ref.score)
    for f in ("mod_calls.tsv", "mod_sites.tsv"):
        assert (tmp_path / "gpu" / f).read_bytes() == (tmp_path / "ref" / f).read_bytes(), f
    on_disk = json.loads((tmp_path / "gpu" / "modcall_report.json").read_text())
    assert got == on_disk and {k: v for k, v in got.items() if k != "input"} == {k: v for k, v in want.items() if k != "input"}
    assert got["k"] == 3 and got["kmers_known"] == [64, 64] and got["motif"] == "CG" and got["flank"] == 2 and got["min_delta"] == 2.0
    assert got["min_delta_tuned_on_real_reads"] is False and got["files"] == ["mod_calls.tsv", "mod_sites.tsv"]
    assert got["reads"]["total"] == 6 and got["reads"]["used"] >= 1 and got["groups"]["scored"] >= 1 and got["batches"] == 1
    assert got["groups"]["seen"] == got["groups"]["scored"] + sum(got["groups"]["dropped"].values()) and set(got["groups"]["dropped"]) == set(modcall.GROUP_DROPS)
    rows = [ln.split("\t") for ln in (tmp_path / "gpu" / "mod_calls.tsv").read_text().splitlines()]
    assert tuple(rows[0]) == modcall.CALL_COLUMNS and len(rows) == 1 + got["groups"]["scored"] == 1 + sum(got["calls"].values())
    assert all(r[1] == "ctg" and r[4] in "+-" and r[10] in modcall.CALLS and seq[int(r[2]) - 1] == ("C" if r[4] == "+" else "G") for r in rows[1:])
    with pytest.raises(SystemExit) as ei:
        entry.main(argv[:argv.index("--alt-table") + 1] + [str(tmp_path / "other.tsv"), "-o", str(tmp_path / "bad")])
    assert "the same k" in str(ei.value)
