"""GPU: chiron_ctc_score (csrc/ctc_score.hip) through chiron_amd.polish.score against the numpy float64 restatement of
tests/polish_ref.py, and `polish` end to end.

Tolerance: |got - ref| <= 1e-9 * max(1, |ref|).  Derived, not measured: both sides round exp and log, a few ulp (2.2e-16) per lse,
over at most 4096 frames, about 1e-11 relative for the longest items; an fp32 recursion or a result rounded to float misses by
1e-7 relative or more.  Infinities and status codes must be equal."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from chiron_amd import _lib, map as cmap, pileup, polish

import polish_cases as cases
import polish_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9


def _codes(s):
    return np.array(["ACGT".index(c) for c in s], dtype=np.uint8)


def _close(got, want):
    return got == want if not np.isfinite(want) else abs(got - want) <= TOL * max(1.0, abs(want))


def _check(x, items, cands, want=None, **kw):
    """polish.score against the reference, candidate by candidate.  -> the GPU's result."""
    got = polish.score(x, items, cands, **kw)
    want = want or polish_ref.score(x, items, cands)
    assert len(got["loglik"]) == len(got["status"]) == len(items)
    for i, (gl, gs, wl, ws) in enumerate(zip(got["loglik"], got["status"], want["loglik"], want["status"])):
        assert gl.dtype == np.float64 and gs.dtype == np.int32 and len(gl) == len(gs) == len(cands[i])
        assert np.array_equal(gs, ws), (i, gs, ws)
        for k in range(len(gl)):
            assert _close(gl[k], wl[k]), (i, k, items[i], len(cands[i][k]), gl[k], wl[k], gl[k] - wl[k])
    return got


def _no_repeats(rng, L):
    return (np.cumsum(rng.integers(1, 4, size=L)) % 4).astype(np.uint8)


def _with_repeats(rng, L):
    lab = rng.integers(0, 4, size=L).astype(np.uint8)
    lab[1::3] = lab[0:-1:3][:len(lab[1::3])]                    # every third base repeats its neighbour
    return lab


def test_edge_cases_in_one_launch(built):
    rng = np.random.default_rng(310)
    parts, items, cands = [], [], []

    def add(x, labs):
        at = sum(len(p) for p in parts)
        parts.append(np.asarray(x, np.float32).reshape(-1, 5))
        items.append((at, at + len(parts[-1])))
        cands.append(labs)

    add(np.zeros((0, 5)), [_codes(""), _codes("A")])                        # T = 0: L = 0 is 0.0, L = 1 is infeasible
    add(rng.normal(0, 3, (5, 5)), [_codes("")])                             # L = 0, T = 5: the blanks' sum
    add(rng.normal(0, 3, (1, 5)), [_codes(""), _codes("G"), _codes("GT")])  # T = 1
    add(rng.normal(0, 3, (9, 5)), [_codes("C"), _codes("T")])               # L = 1
    add(rng.normal(0, 3, (7, 5)), [_codes("AAAA")])                         # T = 2L - 1: one path
    add(rng.normal(0, 3, (6, 5)), [_codes("AAAA"), _codes("AAAC"), _codes("ACAC")])   # T = 2L - 2: infeasible, one path, many
    add(rng.choice([-80.0, 80.0], (12, 5)), [_codes("ACG"), _codes(""), _codes("TTT")])   # logits of +-80
    add(np.where(rng.random((10, 5)) < 0.5, -80.0, rng.normal(0, 1, (10, 5))), [_codes("GAT")])
    long_x = cases.planted(rng, rng.integers(0, 4, 1500).astype(np.uint8), dwell_p=0.36)[:4096]
    assert len(long_x) == polish.MAX_FRAMES
    add(long_x, [rng.integers(0, 4, 127).astype(np.uint8), _no_repeats(rng, 127)])       # 4096 frames, L = 127, a wrong labelling
    x = np.concatenate(parts)
    got = _check(x, items, cands)
    assert got["loglik"][0].tolist() == [0.0, -np.inf] and got["status"][0].tolist() == [0, 1]
    assert got["status"][2].tolist() == [0, 0, 1] and got["status"][5].tolist() == [1, 0, 0]
    assert _close(got["loglik"][1][0], float(polish_ref.log_softmax(parts[1])[:, 4].sum()))
    assert np.all(np.isfinite(got["loglik"][-1])) and np.all(got["loglik"][-1] < -1000) and not got["status"][-1].any()
    assert np.all(np.isfinite(got["loglik"][6])) and np.all(np.isfinite(got["loglik"][7]))
    # a float-rounded result would miss the tolerance here: the bound separates the two
    ll = got["loglik"][-1][0]
    assert abs(float(np.float32(ll)) - ll) > TOL * abs(ll)
    # no item, no candidate: nothing to do, and no device is needed for it
    assert polish.score(x, [], []) == {"loglik": [], "status": []}
    empty = polish.score(x, [(0, 5)], [[]])
    assert len(empty["loglik"]) == 1 and empty["loglik"][0].shape == (0,)


@pytest.mark.parametrize("repeats", [False, True])
def test_lane_and_state_boundaries(built, repeats):
    """L around the lane boundaries (a lane owns four states, two bases) and at the last lane, each at the fewest frames it can
    have and at T = 3L."""
    rng = np.random.default_rng(311 + repeats)
    parts, items, cands, at = [], [], [], 0
    for L in (1, 2, 31, 32, 63, 64, 127):
        lab = _with_repeats(rng, L) if repeats else _no_repeats(rng, L)
        rep = int(np.count_nonzero(lab[1:] == lab[:-1]))
        assert (rep > 0) == (repeats and L > 1)
        other = lab.copy()
        other[L // 2] = (other[L // 2] + 1) % 4
        for T in (L + rep, 3 * L):
            x = cases.planted(rng, lab, dwell_p=0.5)[:T] if T > L + rep else rng.normal(0, 2, (T, 5)).astype(np.float32)
            x = np.concatenate([x, rng.normal(0, 2, (T - len(x), 5)).astype(np.float32)])
            parts.append(x)
            items.append((at, at + T))
            cands.append([lab, other, lab[:-1], np.concatenate([lab, lab[:1]])[:polish.MAX_LABEL]])
            at += T
    got = _check(np.concatenate(parts), items, cands)
    assert all(st[0] == 0 for st in got["status"])
    assert any(st[3] == 1 for st in got["status"])                # one base more than the frames allow


def test_candidates_share_and_overlap_frames(built):
    rng = np.random.default_rng(313)
    lab = rng.integers(0, 4, 400).astype(np.uint8)
    x = cases.planted(rng, lab, dwell_p=0.4)
    F = len(x)
    items, cands = [], []
    for k, b in enumerate(range(0, F - 60, 30)):                  # items of 60 frames that overlap their neighbours by half
        items.append((b, b + 60))
        cands.append([] if k == 3 else [rng.integers(0, 4, int(rng.integers(8, 30))).astype(np.uint8) for _ in range(5)])
    items.append((0, 600))                                        # and one over the first twenty of them
    cands.append([lab[:100], lab[:127]])
    assert len(cands[3]) == 0 and len(items) > 20
    got = _check(x, items, cands)
    # an item scored alone, from a copy of its frames, gives the same bits: nothing leaks between items
    for i in (0, 5, len(items) - 2):
        b, e = items[i]
        alone = polish.score(x[b:e].copy(), [(0, e - b)], [cands[i]])
        assert alone["loglik"][0].tobytes() == got["loglik"][i].tobytes()
    # runs planned against a small workspace hand each run only its frames: the same bits again
    small = polish.workspace_size(400, 8, 40, 40 * 30) / (1 << 20)
    assert len(polish.plan_batches(items[:-1], cands[:-1], int(small * (1 << 20)))) >= 3
    tiled = polish.score(x, items[:-1], cands[:-1], workspace_mb=small)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(tiled["loglik"], got["loglik"][:-1]))


def test_more_candidates_than_waves(built):
    """4 * MAX_GROUPS + 37 candidates of T = 8, L = 3: a launch has at most 4 * MAX_GROUPS waves, so 37 waves take a second
    candidate."""
    rng = np.random.default_rng(314)
    n = 4 * polish.MAX_GROUPS + 37
    assert polish.THREADS // 64 == 4 and polish.MAX_GROUPS == _lib.SCORE_MAX_GROUPS
    x = rng.normal(0, 2, (n + 7, 5)).astype(np.float32)
    items = [(k, k + 8) for k in range(n)]
    cands = [[lab] for lab in rng.integers(0, 4, (n, 3)).astype(np.uint8)]
    got = _check(x, items, cands)
    assert np.isfinite(np.concatenate(got["loglik"])).sum() > n // 2


def test_determinism(built):
    rng = np.random.default_rng(315)
    x = cases.planted(rng, rng.integers(0, 4, 300).astype(np.uint8))
    items, cands = [], []
    for _ in range(128):
        b = int(rng.integers(0, len(x) - 80))
        items.append((b, b + int(rng.integers(20, 80))))
        cands.append([rng.integers(0, 4, int(rng.integers(1, 25))).astype(np.uint8) for _ in range(2)])
    first = _check(x, items, cands)
    again = polish.score(x, items, cands)
    order = rng.permutation(len(items))
    mixed = polish.score(x, [items[i] for i in order], [cands[i][::-1] for i in order])
    for k, i in enumerate(order):
        assert first["loglik"][i].tobytes() == again["loglik"][i].tobytes() == mixed["loglik"][k][::-1].tobytes()
        assert np.array_equal(first["status"][i], mixed["status"][k][::-1])


def test_planted_case_end_to_end(built):
    """The planted case of the CPU test with every stage on the GPU -- map_reads' infix alignment, add_cigars, pileup.count,
    label.align, polish.score -- against the same pipeline on the references: the same candidates, reads_scored and accepted set,
    every read's logliks within the tolerance and the llr within the tolerance summed over a variant's reads."""
    truth, draft, called, logits, seeds = cases.end_to_end_case()
    genome, piled_ref, want = cases.reference_pipeline(draft, called, logits, seeds)
    res = cmap.map_reads(called, genome, seeds=seeds)
    cmap.add_cigars(res, called, genome)
    source = pileup.from_map(res, called, genome)
    piled = pileup.count(source["alignments"], genome, want_counts=True)
    assert np.array_equal(piled["counts"], piled_ref["counts"])
    got = polish.polish(cases.reads_of(res, called, logits, genome), genome, piled["counts"], piled["depth"])
    key = lambda r: (r["g"], r["type"], r["alt"], r["count"], r["depth"], r["reads_scored"])
    assert [key(r) for r in got["variants"]] == [key(r) for r in want["variants"]] and len(want["variants"]) > 100
    assert got["report"] == want["report"]
    left_out = 0
    for g, w in zip(got["variants"], want["variants"]):
        # every read's two logliks within the kernel's tolerance, and so the llr within that tolerance summed over the reads
        assert len(g["logliks"]) == len(w["logliks"]) == w["reads_scored"]
        bound = 0.0
        for (g_ref, g_alt), (w_ref, w_alt) in zip(g["logliks"], w["logliks"]):
            assert _close(g_ref, w_ref) and _close(g_alt, w_alt), (g, w)
            bound += TOL * max(1.0, abs(w_ref)) + TOL * max(1.0, abs(w_alt))
        assert abs(g["llr"] - w["llr"]) <= bound, (g["llr"], w["llr"], bound)
        if w["reads_scored"] and abs(w["llr"] - want["report"]["min_llr"]) <= 1e-6:
            left_out += 1
        else:
            assert g["accepted"] == w["accepted"], (g, w)
    assert left_out == 0                                                     # the seed was picked so (and at most 1 % may be)
    if not left_out:
        assert [key(r) for r in got["accepted"]] == [key(r) for r in want["accepted"]]
    before = cases.edits_against(truth, dict(draft))
    after = cases.edits_against(truth, polish.apply(genome, got["accepted"]))
    print("edits against the truth: draft %d, polished %d" % (before, after))
    assert after < before


def test_polish_command(built, tmp_path):
    """`chiron polish --synthetic-weights` on a tiny `call` + `map --cigar` tree: signals under raw/, a mapped.sam whose reads carry
    those names.  With synthetic weights the logits mean nothing; the command's plumbing is what is run."""
    import chiron_amd as ca
    rng = np.random.default_rng(316)
    seq = "".join("ACGT"[v] for v in rng.integers(0, 4, 400))
    (tmp_path / "genome.fa").write_text(">ctg\n%s\n" % seq)
    raw = tmp_path / "call" / "raw"
    raw.mkdir(parents=True)
    lines = ["@HD\tVN:1.6\tSO:unknown", "@SQ\tSN:ctg\tLN:400"]
    for k in range(6):
        start = 20 * k
        piece = list(seq[start:start + 120])
        piece[40 + k % 2] = "ACGT"[("ACGT".index(piece[40 + k % 2]) + 1) % 4]         # a substitution half of the reads share
        piece = "".join(piece)
        reverse = k % 2 == 1
        sig = ca.synthetic_signal(1, 1500, seed=40 + k)[0]
        (raw / ("read%d.signal" % k)).write_text(" ".join(str(int(v)) for v in sig))
        ops = "40=1X79=" if k % 2 == 0 else "41=1X78="
        lines.append("\t".join(["read%d" % k, "16" if reverse else "0", "ctg", str(start + 1), "255", ops, "*", "0", "0", piece, "*", "NM:i:1"]))
    lines.append("\t".join(["nosig", "0", "ctg", "1", "255", "50=", "*", "0", "0", seq[:50], "*", "NM:i:0"]))
    (tmp_path / "map").mkdir()
    (tmp_path / "map" / "mapped.sam").write_text("".join(ln + "\n" for ln in lines))
    r = subprocess.run([sys.executable, "-m", "chiron_amd.entry", "polish", "-i", str(tmp_path / "map"), "-s", str(tmp_path / "call"), "-g",
                        str(tmp_path / "genome.fa"), "-o", str(tmp_path / "out"), "--synthetic-weights", "-b", "8", "--min-alt", "1"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    again = cmap.load_genome(str(tmp_path / "out" / "polished.fasta"))
    assert again.names == ["ctg"] and abs(int(again.lengths[0]) - 400) <= 10
    report = json.loads((tmp_path / "out" / "polish_report.json").read_text())
    rd, it, cd = report["reads"], report["items"], report["candidates"]
    assert rd["total"] == 7 and rd["dropped"]["no_signal"] == 1 and rd["total"] == rd["used"] + sum(rd["dropped"].values())
    assert it["total"] == it["scored"] + sum(it["dropped"].values()) and cd["total"] == cd["scored"] + sum(cd["skipped"].values()) >= 2
    lines = (tmp_path / "out" / "polish_variants.tsv").read_text().splitlines()
    assert lines[0].split("\t") == list(polish.VARIANT_COLUMNS) and len(lines) == 1 + cd["scored"]
    assert sum(int(ln.split("\t")[-1]) for ln in lines[1:]) == report["accepted"]["total"]
    assert report["contigs"][0]["polished_length"] == int(again.lengths[0])
    # a directory of `map` without --cigar is told so
    (tmp_path / "plain").mkdir()
    r = subprocess.run([sys.executable, "-m", "chiron_amd.entry", "polish", "-i", str(tmp_path / "plain"), "-s", str(tmp_path / "call"), "-g",
                        str(tmp_path / "genome.fa"), "-o", str(tmp_path / "o2"), "--synthetic-weights"], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and "--cigar" in r.stderr
