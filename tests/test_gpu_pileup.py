"""GPU: chiron_pileup (csrc/pileup.hip) through chiron_amd.pileup against the column-by-column reference of tests/pileup_ref.py.
Every case asserts counts, depth, call and clipped equal to the reference exactly: edge cases, the scan's carries across waves and
chunks, contention on a few addresses, random sets that exercise every clause of the call rule, tiling and determinism, and
`chiron pileup` end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from chiron_amd import assess, map as cmap, pileup

import pileup_cases as cases
import pileup_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = pileup_ref.S


def _check(alns, g0, g1, ref=None, min_depth=3, want=None):
    """One raw call against the reference.  -> (counts, depth, call, clipped) of the GPU."""
    ref = np.zeros(max(g1 - g0, 0), np.uint8) if ref is None else np.asarray(ref, np.uint8)
    got = pileup.pileup_tile(alns, g0, g1, ref, min_depth)
    want = want or pileup_ref.counter(alns, g0, g1, ref, min_depth)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.uint8
    assert np.array_equal(got[0], want[0]), np.argwhere(got[0] != want[0])[:5]
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and got[3] == want[3]
    return got


def _aln(pos, cigar, rng=None, read=None):
    ops = pileup.ops_from_cigar(cigar)
    n = int((ops != 3).sum())
    if read is None:
        read = (rng or np.random.default_rng(0)).integers(0, 4, n)
    return int(pos), np.asarray(read, np.uint8), ops


def test_edge_cases(built):
    rng = np.random.default_rng(170)
    ref = rng.integers(0, 5, 40).astype(np.uint8)
    counts, depth, call, clipped = _check([], 100, 140, ref)                          # no alignments: all low depth
    assert not counts.any() and np.array_equal(call[:, 0], ref) and np.all(call[:, 6] == 1) and clipped == 0
    _, _, call, _ = _check([], 100, 140, ref, min_depth=0)                            # min_depth 0: all reference, called
    assert np.array_equal(call[:, 0], ref) and not call[:, 6].any()
    alns = [_aln(105, "*"), _aln(105, "7I", rng), _aln(110, "6D"), _aln(104, "3I5=2I", rng), _aln(101, "2=%dI2=" % S, rng),
            _aln(101, "2=%dI2=" % (S + 1), rng), _aln(101, "2=%dI2=" % (S + 5), rng),
            _aln(120, "3=2I3=", read=[4, 0, 4, 4, 4, 1, 2, 4]),                       # N in diagonal columns and in an insertion
            _aln(100, "4=1D3X", rng), _aln(133, "2=1I1D4=", rng),                     # starts exactly at g0, ends exactly at g1
            _aln(95, "10=", rng), _aln(136, "3=1I6=", rng),                           # partly outside, at either end
            _aln(20, "30=", rng), _aln(140, "5=", rng), _aln(90, "5=1I5=", rng), _aln(99, "1=2I", rng)]   # wholly outside
    for md in (0, 1, 3):
        counts, depth, call, clipped = _check(alns, 100, 140, ref, min_depth=md)
    assert clipped == 7 + 3 + 2 + 2
    assert counts[pileup_ref.OVER].sum() == 2 and counts[pileup_ref.OVER, 2] == 2     # S, S + 1, S + 5 inserted bases: 0, 1, 1
    assert counts[pileup_ref.INS + 5 * (S - 1):pileup_ref.INS + 5 * S, 2].sum() == 3
    assert counts[pileup_ref.DEL, 10:16].tolist() == [1] * 6 and counts[4, 20] == 1 and counts[pileup_ref.INS + 4, 22] == 1
    # the empty tile: nothing but the clipping, and no device
    got = pileup.pileup_tile(alns, 100, 100, np.zeros(0, np.uint8), 3)
    assert got[0].shape == (pileup.PLANES, 0) and got[1].shape == (0,) and got[2].shape == (0, 8) and got[3] == clipped


def test_scan_carries_at_every_wave_and_chunk_boundary(built):
    """Alignments of 63 .. 1025 columns and of the kernel's chunk +- 1; in each an 'I' run, a 'D' run and an 'I' run longer than S
    start just before every multiple of 64 that the alignment has, so each straddles a wave or chunk boundary: the smallest shapes
    at which q, i or k can be carried wrongly."""
    rng = np.random.default_rng(171)
    T, chunk = pileup.THREADS, pileup.CHUNK
    lens = sorted({63, 64, 65, T - 1, T, T + 1, 1023, 1024, 1025, chunk - 1, chunk, chunk + 1, 2 * chunk + 3})
    alns = []
    for n in lens:
        for kind, length, lead in ((2, 3, 2), (3, 3, 1), (2, S + 3, S + 1), (2, 70, 35), (3, 130, 64)):
            ops = np.zeros(n, dtype=np.uint8)
            for edge in range(64, n + 63, 64):
                lo = edge - lead
                if lo > 0 and lo + length < n - 1:
                    ops[lo:lo + length] = kind
            if not ops.any():
                ops[n // 2:n // 2 + min(length, n // 4)] = kind
            alns.append((int(rng.integers(0, 50)), rng.integers(0, 4, int((ops != 3).sum())).astype(np.uint8), ops))
        alns.append(cases.random_alignment(rng, n, rng.integers(0, 50), p_ins=0.3, p_del=0.2, n_rate=0.02))
    total = 60 + 2 * chunk + 3
    ref = rng.integers(0, 4, total).astype(np.uint8)
    counts, _, _, _ = _check(alns, 0, total, ref)
    assert counts[pileup_ref.OVER].sum() > 30
    # every alignment alone gives its own share: a result depends on nothing but that alignment
    acc = np.zeros_like(counts)
    for a in alns[::7]:
        acc += _check([a], 0, total, ref)[0]
    assert np.array_equal(acc, pileup_ref.count_columns(alns[::7], 0, total)[0])


def test_contention(built):
    rng = np.random.default_rng(172)
    one = cases.random_alignment(rng, 300, 10, p_ins=0.1, p_del=0.1)
    planes, clipped = pileup_ref.count_columns([one], 0, 330)
    ref = rng.integers(0, 4, 330).astype(np.uint8)
    want = planes * 2000
    depth, call = pileup_ref.call_tile(want, ref, 3)
    counts, _, _, _ = _check([one] * 2000, 0, 330, ref, want=(want, depth, call, clipped * 2000))
    assert set(np.unique(counts).tolist()) == {0, 2000}
    short = _aln(3, "3=1X1D3=", rng)                                               # 8 columns on positions 3 .. 10
    planes, clipped = pileup_ref.count_columns([short], 0, 12)
    want = planes * 70000                                                            # above any 16-bit shortcut
    depth, call = pileup_ref.call_tile(want, ref[:12], 3)
    counts, _, _, _ = _check([short] * 70000, 0, 12, ref[:12], want=(want, depth, call, 0))
    assert counts.max() == 70000 and counts[:, 3:11].sum() == 70000 * 8


@pytest.fixture(scope="module")
def random_case():
    """300 alignments over a 700-position tile from a two-letter alphabet at high indel rates, and the reference's answer."""
    rng = np.random.default_rng(173)
    alns = cases.random_set(rng, 300, 700, max_columns=30, p_ins=0.35, p_del=0.25, letters=2, n_rate=0.03)
    ref = rng.integers(0, 2, 700).astype(np.uint8)
    ref[rng.random(700) < 0.1] = 4                   # a tie between two non-reference bases needs a reference that is neither
    planes, clipped = pileup_ref.count_columns(alns, 0, 700)
    return alns, ref, planes, clipped


def test_random_sets_exercise_every_clause(built, random_case):
    alns, ref, planes, clipped = random_case
    for md in (1, 3, 5):
        clauses = {}
        depth, call = pileup_ref.call_tile(planes, ref, md, clauses)
        _check(alns, 0, 700, ref, md, want=(planes, depth, call, clipped))
        if md == 3:
            # (a chain that stops before a slot that would pass cannot come from alignments -- whoever has a (k+2)-th inserted base
            # has a (k+1)-th -- so that clause is test_pileup_cpu.py's, on hand-made counts)
            want = ("low", "base", "deletion", "tie_ref", "tie_code", "tie_deletion", "insertion", "insertion_chain")
            assert all(clauses.get(k, 0) >= 3 for k in want), clauses
            assert (depth == md).sum() > 10 and (depth == md - 1).sum() > 10
    # only-N positions and insertion slots of only N, which chance does not give: the same tile with reads of N alone
    n_alns = [(pos, np.full(len(read), 4, np.uint8), ops) for pos, read, ops in alns[:150]]
    clauses = {}
    planes_n, clipped_n = pileup_ref.count_columns(n_alns, 0, 700)
    depth, call = pileup_ref.call_tile(planes_n, ref, 2, clauses)
    assert clauses.get("only_n", 0) > 50 and clauses.get("insertion_n", 0) >= 3, clauses
    _check(n_alns, 0, 700, ref, 2, want=(planes_n, depth, call, clipped_n))


def test_tiling_and_determinism(built, random_case):
    alns, ref, planes, clipped = random_case
    depth, call = pileup_ref.call_tile(planes, ref, 3)
    whole = _check(alns, 0, 700, ref, 3, want=(planes, depth, call, clipped))
    for width in (1, 100, 257):
        parts = [pileup.pileup_tile(alns, g0, min(g0 + width, 700), ref[g0:g0 + width], 3) for g0 in range(0, 700, width)]
        assert np.array_equal(np.concatenate([p[0] for p in parts], axis=1), whole[0]), width
        assert np.array_equal(np.concatenate([p[1] for p in parts]), whole[1]) and np.array_equal(np.concatenate([p[2] for p in parts]), whole[2])
        assert all(p[3] == clipped for p in parts)                                    # clipped does not depend on the tile
    genome = cmap.Genome([("c", "".join("ACGTN"[v] for v in ref))])
    plan = pileup.plan_tiles(alns, 700, 24 << 10)
    assert len(plan) >= 4
    calls = []

    def counter(a, g0, g1, r, md):
        calls.append((g0, g1))
        return pileup.pileup_tile(a, g0, g1, r, md)

    tiled = pileup.count(alns, genome, workspace_mb=24 / 1024, counter=counter, want_counts=True)      # 24 KiB: several tiles
    assert len(calls) == len(plan) + 1 and calls[:-1] == [t[:2] for t in plan]
    assert np.array_equal(tiled["counts"], whole[0]) and np.array_equal(tiled["depth"], whole[1]) and np.array_equal(tiled["call"], whole[2])
    assert tiled["clipped"] == clipped and tiled["over_total"] == int(planes[pileup_ref.OVER].sum())
    plain = pileup.count(alns, genome, want_counts=True)                              # the library itself, one tile
    assert np.array_equal(plain["counts"], whole[0]) and np.array_equal(plain["call"], whole[2]) and plain["clipped"] == clipped
    assert "counts" not in pileup.count(alns, genome)
    order = np.random.default_rng(174).permutation(len(alns))
    again = pileup.pileup_tile([alns[i] for i in order], 0, 700, ref, 3)
    third = pileup.pileup_tile(alns, 0, 700, ref, 3)
    for a, b, c in zip(whole, again, third):
        assert np.array_equal(a, b) and np.array_equal(a, c)


def test_pileup_command_end_to_end(built, tmp_path):
    """The CPU test's case through the commands: `map --cigar` on the GPU, then `pileup` on its output directory.  The outputs
    equal what the reference pipeline makes of the same mapped.sam, and the consensus is closer to the truth than the genome."""
    truth, given, reads, _ = cases.end_to_end_case()
    (tmp_path / "genome.fa").write_text("".join(">%s\n%s\n" % c for c in given))
    (tmp_path / "reads.fa").write_text("".join(">%s\n%s\n" % kv for kv in reads.items()))
    for cmd in (["map", "-i", str(tmp_path / "reads.fa"), "-g", str(tmp_path / "genome.fa"), "-o", str(tmp_path / "map"), "--cigar"],
                ["pileup", "-i", str(tmp_path / "map"), "-g", str(tmp_path / "genome.fa"), "-o", str(tmp_path / "pile")]):
        r = subprocess.run([sys.executable, "-m", "chiron_amd.entry"] + cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
    genome = cmap.Genome(given)
    source = pileup.read_sam(str(tmp_path / "map" / "mapped.sam"), genome)
    assert source["used"] >= 50
    want = cases.reference_consensus(source, genome)
    seqs = dict(assess.read_records(str(tmp_path / "pile" / "consensus.fasta")))
    assert seqs == want["consensus"]
    lines = (tmp_path / "pile" / "variants.tsv").read_text().splitlines()
    assert lines[0].split("\t") == list(pileup.VARIANT_COLUMNS)
    assert [ln.split("\t") for ln in lines[1:]] == [[str(r[k]) for k in pileup.VARIANT_COLUMNS] for r in want["variants"]]
    report = json.loads((tmp_path / "pile" / "pileup_report.json").read_text())
    t = report["totals"]
    assert report["alignments_used"] == source["used"] and report["clipped"] == want["clipped"] and report["min_depth"] == 3
    assert report["over_total"] == int(want["counts"][pileup_ref.OVER].sum())
    assert t["substitutions"] + t["deletions"] + t["insertions"] == len(want["variants"]) == len(lines) - 1
    assert [c["consensus_length"] for c in report["contigs"]] == [len(seqs[name]) for name, _ in given]
    assert t["low_depth"] == int((want["call"][:, 6] == 1).sum()) - cmap.SEPARATOR
    assert abs(t["mean_depth"] - float(np.concatenate([want["depth"][:len(given[0][1])], want["depth"][len(given[0][1]) + cmap.SEPARATOR:]]).mean())) < 1e-9
    rows = assess.align_pairs([seqs[name] for name, _ in truth] + [seq for _, seq in given], [seq for _, seq in truth] * 2)
    after, before = int(rows["edit"][:2].sum()), int(rows["edit"][2:].sum())
    print("edits against the truth: given genome %d, consensus %d" % (before, after))
    assert after < before
    # a directory of `map` without --cigar is told so
    (tmp_path / "plain").mkdir()
    r = subprocess.run([sys.executable, "-m", "chiron_amd.entry", "pileup", "-i", str(tmp_path / "plain"), "-g", str(tmp_path / "genome.fa"),
                        "-o", str(tmp_path / "p2")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--cigar" in r.stderr
