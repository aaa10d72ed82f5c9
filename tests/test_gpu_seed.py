"""GPU: chiron_seed_reads (csrc/seed.hip) through chiron_amd.map.vote_reads against the definition, chiron_amd.map.vote.  Every
case asserts vote_reads(index, reads) == [vote(index, r) for r in reads]: the same keys, the same Python values, no tolerance.
The hand cases are those of tests/seed_ref.py, which test_seed_cpu.py also runs through the numpy restatement of the kernel."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from chiron_amd import map as cmap

import map_ref
import seed_ref
from test_map_cpu import E2E_SEED

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = ("degenerate_reads", "empty_index", "nothing_matches", "lengths", "ties", "palindrome", "bin_boundaries", "second_copy_near",
         "second_copy_far", "repeats_occ64", "repeats_occ8", "two_contigs")


@pytest.fixture(scope="module")
def hand():
    cases, extra = seed_ref.hand_cases()
    assert set(cases) == set(CASES)
    return cases, extra, {name: [cmap.vote(index, r) for r in reads] for name, (index, reads) in cases.items()}


@pytest.mark.parametrize("name", CASES)
def test_hand_case_equals_vote(built, hand, name):
    cases, extra, want = hand
    index, reads = cases[name]
    got = cmap.vote_reads(index, reads)
    assert got == want[name]
    for g, w in zip(got, want[name]):                                        # the same Python types, not only equal values
        assert list(g) == list(w) and [type(v) for v in g.values()] == [type(v) for v in w.values()]
    assert cmap.vote_reads(index, reads[::-1]) == want[name][::-1]
    if name == "two_contigs":
        for v, contig in zip(got, extra[name]["contigs"]):
            assert (v["votes"] == 0) if contig is None else (extra[name]["genome"].contig_of(v["g"]) == contig)
    if name == "second_copy_near":
        assert [v["votes_second"] for v in got] == [0, 0]
    if name == "second_copy_far":
        assert [v["votes_second"] for v in got] == [286, 286]
    if name == "ties":
        assert got[0]["delta"] == extra[name]["two_copies_delta"] and got[0]["votes_second"] == got[0]["votes"]
        assert got[2]["delta"] == -300 and got[1]["strand"] == "reverse"


def test_no_reads_and_one_empty_read(built):
    index, _ = seed_ref.hand_cases()[0]["nothing_matches"]
    assert cmap.vote_reads(index, []) == []
    assert cmap.vote_reads(index, [np.zeros(0, np.uint8)]) == [cmap.vote(index, np.zeros(0, np.uint8))]


@pytest.fixture(scope="module")
def many():
    index, reads = seed_ref.hygiene_case(2500)
    return index, reads, [cmap.vote(index, r) for r in reads]


def test_more_reads_than_workgroups_and_counter_hygiene(built, many):
    """2500 reads on at most 2048 workgroups: the later reads run on counters an earlier read used.  Every third read repeats its
    predecessor and every seventh is unrelated, so a counter that was not cleared shows as a doubled or a spurious vote."""
    from chiron_amd import _lib
    index, reads, want = many
    assert len(reads) > _lib.SEED_MAX_GROUPS
    got = cmap.vote_reads(index, reads)
    assert got == want
    assert sum(v["votes"] == 0 for v in want) > 200 and sum(v["strand"] == "reverse" for v in want) > 500
    assert cmap.vote_reads(index, reads[::-1]) == want[::-1]
    for k in np.random.default_rng(7).choice(len(reads), 32, replace=False).tolist():
        assert cmap.vote_reads(index, [reads[k]]) == [want[k]], k
    val32, pos32 = index[0].astype(np.uint32), index[1].astype(np.int32)
    genome_len = int(index[1].max()) + cmap.K
    runs = [b"".join(a.tobytes() for a in cmap.seed_reads(val32, pos32, genome_len, reads)) for _ in range(2)]
    assert runs[0] == runs[1]


@pytest.fixture(scope="module")
def long_reads():
    index, reads = seed_ref.long_read_cases()
    codes = list(reads.values())
    return index, codes, [cmap.vote(index, r) for r in codes]


def test_long_reads_equal_vote(built, long_reads):
    """4 k to 131072 bases, the longest read the kernel takes, on both strands: see seed_ref.long_read_cases."""
    index, reads, want = long_reads
    got = cmap.vote_reads(index, reads)
    assert got == want
    assert cmap.vote_reads(index, reads[::-1]) == want[::-1]
    val32, pos32 = index[0].astype(np.uint32), index[1].astype(np.int32)
    genome_len = int(index[1].max()) + cmap.K
    runs = [b"".join(a.tobytes() for a in cmap.seed_reads(val32, pos32, genome_len, reads)) for _ in range(2)]
    assert runs[0] == runs[1]


def test_one_long_read_among_short_ones(built):
    """The 131072-base read and 300 short reads in one call: the call's kc_stride, off and nbins are sized by the long read.
    Every read's answer is the one it gets alone, with the long read first and with it last."""
    index, long, short = seed_ref.mixed_batch()
    alone = [cmap.vote_reads(index, [r])[0] for r in [long] + short]
    assert alone == [cmap.vote(index, r) for r in [long] + short]
    assert cmap.vote_reads(index, [long] + short) == alone
    assert cmap.vote_reads(index, short + [long]) == alone[1:] + alone[:1]


def test_batching_equals_one_call(built, many):
    index, reads, want = many
    reads, want = reads[:900], want[:900]
    lens = [len(r) for r in reads]
    genome_len = int(index[1].max()) + cmap.K
    whole = cmap.seed_workspace_size(len(index[0]), genome_len, len(reads), max(lens), sum(lens))
    budget_mb = whole / 3.5 / (1 << 20)
    batches = cmap.plan_seed_batches(lens, len(index[0]), genome_len, int(budget_mb * (1 << 20)))
    assert len(batches) >= 3 and all(len(b) > 1 for b in batches)
    assert cmap.vote_reads(index, reads, workspace_mb=budget_mb) == want == cmap.vote_reads(index, reads)


def test_map_command_with_either_seed_writes_the_same(built, tmp_path):
    contigs, reads, truth = map_ref.planted_case(E2E_SEED)
    with open(tmp_path / "genome.fa", "w") as f:
        f.write("".join(">%s\n%s\n" % (name, seq) for name, seq in contigs))
    with open(tmp_path / "reads.fa", "w") as f:
        f.write("".join(">%s\n%s\n" % (name, seq) for name, seq in reads.items()))
    report = {}
    for seed in ("gpu", "host"):
        r = subprocess.run([sys.executable, "-m", "chiron_amd.entry", "map", "-i", str(tmp_path / "reads.fa"), "-g", str(tmp_path / "genome.fa"),
                            "-o", str(tmp_path / seed), "--seed", seed], cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        report[seed] = json.loads((tmp_path / seed / "map_report.json").read_text())
        assert report[seed]["seed"] == seed
    for key in ("reads", "totals", "unmapped"):
        assert report["gpu"][key] == report["host"][key], key
    assert report["gpu"]["totals"]["mapped"] == 24 and report["gpu"]["unmapped"] == ["noise0", "noise1"]
    assert (tmp_path / "gpu" / "mapped.paf").read_bytes() == (tmp_path / "host" / "mapped.paf").read_bytes()
    names = sorted(os.listdir(tmp_path / "gpu" / "reference"))
    assert names == sorted(os.listdir(tmp_path / "host" / "reference")) and len(names) == 24
    for name in names:
        assert (tmp_path / "gpu" / "reference" / name).read_bytes() == (tmp_path / "host" / "reference" / name).read_bytes(), name

    memo = {}

    def aligner(rs, ws, band0):                                              # the reference aligner, each pair computed once
        rows = np.zeros(len(rs), dtype=cmap.INFIX_DTYPE)
        for k, (a, b) in enumerate(zip(rs, ws)):
            key = (a.tobytes(), b.tobytes(), band0)
            if key not in memo:
                memo[key] = map_ref.infix_rows([a], [b], band0, cmap.INFIX_DTYPE)[0]
            rows[k] = memo[key]
        return rows

    genome = cmap.Genome(contigs)
    want = cmap.map_reads(reads, genome, aligner=aligner)
    pairs = len(memo)
    assert cmap.map_reads(reads, genome, aligner=aligner, seeder=cmap.seeder_of("gpu")) == want and len(memo) == pairs
    assert report["gpu"]["reads"] == json.loads(json.dumps(want["reads"]))
