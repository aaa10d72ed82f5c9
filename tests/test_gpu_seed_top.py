"""GPU: chiron_seed_candidates (csrc/seed.hip) through chiron_amd.map.vote_reads_top against the definition, map.vote_top: the same
lists of the same dicts, no tolerance.  The cases are those of tests/seed_top_ref.py, which test_seed_top_cpu.py runs through the
numpy restatement of the kernel first."""
import ctypes as C

import numpy as np
import pytest
import torch

from chiron_amd import _lib, map as cmap

import map_ref
import seed_ref
import seed_top_ref
from ws_guard import FILLS, Recorder

pytestmark = pytest.mark.gpu

CASES = ("copies_at_radius", "copies_past_radius", "reverse_copy", "five_copies", "five_copies_all", "equal_scores", "min_score_cuts",
         "min_score_one", "short_reads", "overhang")


@pytest.fixture(scope="module")
def hand():
    cases = seed_top_ref.hand_cases()
    assert set(cases) == set(CASES)
    return cases


@pytest.mark.parametrize("name", CASES)
def test_hand_case_equals_vote_top(built, hand, name):
    index, reads, max_cand, min_score = hand[name]
    want = [cmap.vote_top(index, r, max_cand, min_score) for r in reads]
    got = cmap.vote_reads_top(index, reads, max_cand, min_score)
    assert got == want
    for g, w in zip(got, want):                                              # the same Python types, not only equal values
        assert [[type(v) for v in p.values()] for p in g] == [[type(v) for v in p.values()] for p in w] and [list(p) for p in g] == [list(p) for p in w]
    assert cmap.vote_reads_top(index, reads[::-1], max_cand, min_score) == want[::-1]
    if name == "five_copies":
        assert [len(p) for p in got] == [4, 4] and {p["votes"] for p in got[0]} == {286}
    if name == "copies_past_radius":
        assert [p["votes"] for p in got[0][:2]] == [286, 286]
    if name == "overhang":
        assert got[0][0]["delta"] == -200


@pytest.fixture(scope="module")
def random_reads():
    index, reads = seed_top_ref.random_reads()
    return index, reads, {k: [cmap.vote_top(index, r, k) for r in reads] for k in (1, 4, 8)}


def test_random_reads_equal_vote_top(built, random_reads):
    """300 reads of 15 .. 600 bases against a 20 kb genome with planted repeats, negative deltas included."""
    index, reads, want = random_reads
    for max_cand in (4, 8, 1):
        assert cmap.vote_reads_top(index, reads, max_cand) == want[max_cand], max_cand
    assert cmap.vote_reads_top(index, reads, 4, 30) == [[p for p in picks if p["votes"] >= 30] for picks in want[4]]
    assert cmap.vote_reads_top(index, reads, 4, 30) == [cmap.vote_top(index, r, 4, 30) for r in reads]
    assert cmap.vote_reads_top(index, reads[::-1], 4) == want[4][::-1]
    assert cmap.vote_reads_top(index, [], 4) == [] and cmap.vote_reads_top(index, [np.zeros(0, np.uint8)], 4) == [[]]


def test_one_candidate_equals_seed_reads(built, random_reads, hand):
    """max_cand = 1 is chiron_seed_reads without votes_second: field for field, and the raw arrays too."""
    index, reads, _ = random_reads
    for idx, rs in [(index, reads)] + [(hand[name][0], hand[name][1]) for name in ("equal_scores", "short_reads", "overhang", "five_copies")]:
        single = cmap.vote_reads(idx, rs)
        top = cmap.vote_reads_top(idx, rs, 1)
        for v, picks in zip(single, top):
            assert picks == ([{key: v[key] for key in ("votes", "strand", "delta", "g")}] if v["votes"] else [])
        val32, pos32 = idx[0].astype(np.uint32), idx[1].astype(np.int32)
        genome_len = int(idx[1].max()) + cmap.K
        votes, _, strand, delta, g = cmap.seed_reads(val32, pos32, genome_len, rs)
        count, votes1, strand1, delta1, g1 = cmap.seed_candidates(val32, pos32, genome_len, rs, 1)
        hit = votes > 0
        assert np.array_equal(count, hit.astype(np.int32)) and np.array_equal(votes1[:, 0], votes) and np.array_equal(strand1[:, 0], strand)
        assert np.array_equal(delta1[:, 0][hit], delta[hit]) and np.array_equal(g1[:, 0][hit], g[hit])
        assert not delta1[:, 0][~hit].any() and not g1[:, 0][~hit].any()                  # slots from the count on are zero


def test_more_reads_than_workgroups_and_counter_hygiene(built):
    """2100 reads on at most 2048 workgroups: the later reads run on counters an earlier read used.  Every third read repeats its
    predecessor and every fifth has no hit, so a counter that was not cleared shows as a doubled or a spurious vote; then one read
    2049 times, whose last copy is the second tenant of the first one's workgroup."""
    index, reads = seed_top_ref.hygiene_reads()
    assert len(reads) == 2100 > _lib.SEED_MAX_GROUPS
    want = [cmap.vote_top(index, r, 4) for r in reads]
    assert cmap.vote_reads_top(index, reads, 4) == want
    assert sum(len(p) == 0 for p in want) >= 400 and sum(len(p) >= 3 for p in want) > 300
    assert cmap.vote_reads_top(index, reads[::-1], 4) == want[::-1]
    # 2049 reads that are all the same read, then its second tenant: workgroup 0 takes read 0 and read 2048
    one = next(r for r, p in zip(reads, want) if len(p) >= 3)
    same = cmap.vote_reads_top(index, [one] * (_lib.SEED_MAX_GROUPS + 1), 4)
    assert same == [cmap.vote_top(index, one, 4)] * (_lib.SEED_MAX_GROUPS + 1)
    val32, pos32 = index[0].astype(np.uint32), index[1].astype(np.int32)
    genome_len = int(index[1].max()) + cmap.K
    runs = [b"".join(a.tobytes() for a in cmap.seed_candidates(val32, pos32, genome_len, reads, 4)) for _ in range(2)]
    assert runs[0] == runs[1]


@pytest.mark.parametrize("max_cand", [1, 4, 8])
def test_exactly_sized_poisoned_guarded_memory(built, monkeypatch, random_reads, max_cand):
    """"Caller's memory" of include/chiron_amd.h: under each fill of tests/ws_guard.py the workspace is exactly the bytes the size
    function names, with guards on both sides, and the host outputs hold the fill on entry; the results are the same bytes, no
    output element keeps a poison that is not a result, and the guards stay whole."""
    index, reads, want = random_reads
    reads = reads[:120] + [np.zeros(0, np.uint8), reads[0]]
    lens = [len(r) for r in reads]
    val32, pos32 = np.ascontiguousarray(index[0], np.uint32), np.ascontiguousarray(index[1], np.int32)
    genome_len = int(index[1].max()) + cmap.K
    need = cmap.seed_candidates_workspace_size(len(val32), genome_len, len(reads), max(lens), sum(lens), max_cand)
    read_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    codes = np.ascontiguousarray(np.concatenate(reads + [np.zeros(1, np.uint8)]))
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    seen = []
    for fill in FILLS:
        rec = Recorder(fill)
        ws = rec.byte_buffer(need, torch.device("cuda", 0))
        out = [np.full(len(reads), fill * 0x01010101, np.uint32).view(np.int32)]
        out += [np.full((len(reads), max_cand), fill * 0x01010101, np.uint32).view(np.int32) for _ in range(2)]
        out += [np.full((len(reads), max_cand), fill * 0x0101010101010101, np.uint64).view(np.int64) for _ in range(2)]
        _lib.check(lib.chiron_seed_candidates(0, val32.ctypes.data, pos32.ctypes.data, len(val32), genome_len, codes.ctypes.data,
                                              read_off.ctypes.data, len(reads), max_cand, 1, 0, *[o.ctypes.data for o in out], ws.data_ptr(), stream))
        torch.cuda.synchronize()
        rec.check()
        count, votes, strand, delta, g = out
        got = [[{"votes": int(votes[q, k]), "strand": "reverse" if strand[q, k] else "forward", "delta": int(delta[q, k]), "g": int(g[q, k])}
                for k in range(int(count[q]))] for q in range(len(reads))]
        assert got == want[max_cand][:120] + [[], want[max_cand][0]], fill
        for q in range(len(reads)):                                          # every element is written: zeros from the count on
            for a in (votes, strand, delta, g):
                assert not a[q, int(count[q]):].any(), (fill, q)
        seen.append(b"".join(o.tobytes() for o in out))
    assert seen[0] == seen[1] == seen[2]
    # and through the wrapper: vote_reads_top asks for exactly that many bytes
    for fill in FILLS:
        rec = Recorder(fill)
        monkeypatch.setattr(_lib, "alloc_hook", rec)
        try:
            got = cmap.vote_reads_top(index, reads, max_cand)
        finally:
            monkeypatch.setattr(_lib, "alloc_hook", None)
        torch.cuda.synchronize()
        rec.check()
        assert rec.sizes == [need] and got == want[max_cand][:120] + [[], want[max_cand][0]]


def test_map_command_with_candidates_writes_the_same_with_either_seed(built, tmp_path):
    """map_command at candidates 4 with --cigar: the GPU seeding and the host's vote_top give the same files, the SAM carries the
    mapq, and pileup's reader drops by it."""
    import json
    from chiron_amd import pileup
    contigs, reads, _ = seed_top_ref.repeat_case()
    names = sorted(reads)[:4] + sorted(reads)[-12:]
    (tmp_path / "genome.fa").write_text("".join(">%s\n%s\n" % (name, seq) for name, seq in contigs))
    (tmp_path / "reads.fa").write_text("".join(">%s\n%s\n" % (name, reads[name]) for name in names) + ">noise\n%s\n" % ("ACGTTGCA" * 40))
    report = {seed: cmap.map_command(str(tmp_path / "reads.fa"), str(tmp_path / "genome.fa"), str(tmp_path / seed), cigar=True, seed=seed,
                                     candidates=4) for seed in ("gpu", "host")}
    for key in ("reads", "totals", "unmapped", "candidates", "second_ratio", "mapq0", "mapq1_59", "mapq60", "won_by_later_pick"):
        assert report["gpu"][key] == report["host"][key], key
    assert report["gpu"]["candidates"] == 4 and report["gpu"]["totals"]["mapped"] == 16 and report["gpu"]["unmapped"] == ["noise"]
    assert report["gpu"]["mapq0"] + report["gpu"]["mapq1_59"] + report["gpu"]["mapq60"] == 17
    for name in ("mapped.paf", "mapped.sam"):
        assert (tmp_path / "gpu" / name).read_bytes() == (tmp_path / "host" / name).read_bytes(), name
    assert json.loads((tmp_path / "gpu" / "map_report.json").read_text())["seed"] == "gpu"
    by = {r["name"]: r for r in report["gpu"]["reads"]}
    sam = [ln.split("\t") for ln in (tmp_path / "gpu" / "mapped.sam").read_text().splitlines() if not ln.startswith("@")]
    assert [(c[0], int(c[4])) for c in sam] == [(n, by[n]["mapq"]) for n in sorted(names)]
    genome = cmap.Genome(contigs)
    src = pileup.read_sam(str(tmp_path / "gpu" / "mapped.sam"), genome, min_mapq=60)
    assert src["names"] == [n for n in sorted(names) if by[n]["mapq"] == 60] and src["low_mapq"] == 16 - len(src["names"]) > 0


def test_planted_repeat_reads_map_as_the_reference_pipeline(built):
    """40 reads of the planted repeat (30 from the second copy, 10 controls) through GPU seeding and chiron_align_infix: the records
    of the reference pipeline (host vote_top, the full-table reference aligner), at candidates 4 and at candidates 1."""
    contigs, reads, truth = seed_top_ref.repeat_case()
    names = sorted(reads)[:10] + sorted(reads)[-30:]
    assert sum(n.startswith("ctl") for n in names) == 10
    reads = {n: reads[n] for n in names}
    genome = cmap.Genome(contigs)
    memo = {}

    def aligner(rs, ws, band0):
        rows = np.zeros(len(rs), dtype=cmap.INFIX_DTYPE)
        for k, (a, b) in enumerate(zip(rs, ws)):
            key = (a.tobytes(), b.tobytes(), band0)
            if key not in memo:
                memo[key] = map_ref.infix_rows([a], [b], band0, cmap.INFIX_DTYPE)[0]
            rows[k] = memo[key]
        return rows

    for candidates in (4, 1):
        want = cmap.map_reads(reads, genome, aligner=aligner, candidates=candidates)
        got = cmap.map_reads(reads, genome, candidates=candidates, seeder=cmap.seeder_of("gpu"), top_seeder=cmap.top_seeder_of("gpu"))
        assert got == want, candidates
    by = {r["name"]: r for r in want["reads"]}
    assert all("mapq" not in r for r in want["reads"])
    four = {r["name"]: r for r in cmap.map_reads(reads, genome, aligner=aligner, candidates=4)["reads"]}
    wrong1 = [n for n in names if n.startswith("rep") and seed_top_ref.on_wrong_copy(by[n], truth[n])]
    wrong4 = [n for n in names if n.startswith("rep") and seed_top_ref.on_wrong_copy(four[n], truth[n])]
    assert len(wrong1) >= 2 and wrong4 == [] and all(four[n]["mapq"] == 60 for n in names if n.startswith("ctl"))
