"""CPU: tests/consensus_ref.py (a restatement of the consensus rules in plain NumPy) equals the host consensus -- assemble.cpp behind
assembly.simple_assembly_qs, np.argmax, and the vote summary eval.qs derives -- on every read of tests/consensus_cases.py, exactly;
and every read is what its name says, decided by the restatement alone.  The host functions need no GPU."""
import numpy as np
import pytest

from chiron_amd import assembly, eval as ce

import consensus_cases
import consensus_host
import consensus_ref


@pytest.fixture(scope="module")
def ref():
    return consensus_host.reference()


def test_the_restatement_equals_the_host_path(built, ref):
    for name, segs, qs, kernal in consensus_cases.cases():
        want = ref[name, kernal]
        base, n1, n2, q_top, cons, cqs = consensus_host.host_consensus(segs, qs, kernal)
        assert cons.shape == (4, want["length"]), (name, kernal)
        assert np.array_equal(cons, want["counts"]) and cqs.tobytes() == want["qsum"].tobytes(), (name, kernal)
        assert np.array_equal(base, want["base"]), (name, kernal)
        assert np.array_equal(n1, want["n1"]) and np.array_equal(n2, want["n2"]), (name, kernal)
        assert np.asarray(q_top, dtype=np.float64).tobytes() == want["q_top"].tobytes(), (name, kernal)
        assert ce.qs(cons, cqs) == ce.qs_from_votes(n1, n2, q_top)      # the summary is the one eval.qs scores


def test_the_restatement_equals_glue_kernal_pair_by_pair(built):
    for name in consensus_cases.names():
        segs, _ = consensus_cases.read(name)
        disp = consensus_ref.displacements([consensus_ref.codes(s) for s in segs], "glue")
        for s in range(1, len(segs)):
            assert assembly.glue_kernal(segs[s], segs[s - 1]) == disp[s], (name, s)
            assert assembly.stick_kernal(segs[s], segs[s - 1]) == len(segs[s - 1])


def _overlaps(name):
    segs = [consensus_ref.codes(s) for s in consensus_cases.read(name)[0]]
    return [0] + [consensus_ref.glue_overlap(segs[s], segs[s - 1]) for s in range(1, len(segs))]


def test_long_overlaps_are_long():
    segs, _ = consensus_cases.read("long_overlaps")
    assert len(segs) == 300 and min(map(len, segs)) >= 100 and 350 < max(map(len, segs)) <= 400
    chosen, true = np.asarray(_overlaps("long_overlaps")), np.asarray(consensus_cases.info("long_overlaps")["true_overlap"])
    assert (chosen >= 5).sum() > 100 and (chosen >= 20).sum() >= 10 and (chosen >= 30).sum() >= 3
    assert chosen.max() <= 39 and true.max() == 39
    # glue finds the true overlap wherever its range reaches it (3 % substitutions leave the score far above any other's)
    reach = np.asarray([0] + [consensus_ref.max_overlap(len(segs[s - 1]), len(segs[s])) for s in range(1, 300)])
    found = (true >= 8) & (true < reach)
    assert found.sum() > 100 and np.array_equal(chosen[found], true[found])


def test_clamp_pairs_have_their_min_decided_by_the_side_they_name():
    segs, _ = consensus_cases.read("clamp")
    chosen = _overlaps("clamp")
    pairs = consensus_cases.info("clamp")["pairs"]
    assert sorted(len(segs[s - 1]) for s, side, _ in pairs if side == "prev") == list(consensus_cases.CLAMP_PREV)
    assert sorted(len(segs[s]) for s, side, _ in pairs if side == "n") == [1, 2, 6]
    for s, side, overlap in pairs:
        tenth, n = int(np.floor(0.1 * len(segs[s - 1]))), len(segs[s])
        assert (n < tenth) if side == "n" else (tenth < n), (s, side)
        assert chosen[s] == overlap and consensus_ref.max_overlap(len(segs[s - 1]), n) == min(tenth, n), (s, side)
    # the overlaps tried: none (the loop runs zero times), or overlap 1 alone
    tried = {len(segs[s - 1]): len(consensus_ref.glue_scores(consensus_ref.codes(segs[s]), consensus_ref.codes(segs[s - 1])))
             for s, side, _ in pairs if side == "prev"}
    assert tried == {9: 0, 10: 0, 11: 0, 19: 0, 20: 1, 21: 1}
    # without the clamp by n the periodic tail would match on into the next segment
    s = pairs[0][0]
    run_on = consensus_ref.codes(segs[s] + segs[s + 1])
    assert consensus_ref.glue_overlap(run_on, consensus_ref.codes(segs[s - 1])) == 16 != chosen[s] == 4


def test_ties_choose_the_smallest_overlap_at_the_highest_score():
    segs, _ = consensus_cases.read("ties")
    chosen = _overlaps("ties")
    tied = consensus_cases.info("ties")["tied"]
    assert len(tied) == 4
    for s, at in tied:
        scores = consensus_ref.glue_scores(consensus_ref.codes(segs[s]), consensus_ref.codes(segs[s - 1]))
        top = max(scores.values())
        assert top > 0 and sorted(i for i, v in scores.items() if v == top) == at and len(at) >= 2, (s, scores)
        assert chosen[s] == min(at)


def test_empties_are_where_their_names_say():
    want = {"first": [0], "second": [1], "middle": [5], "two_in_a_row": [10, 11], "last": [14], "all": [0, 1, 2, 3, 4]}
    for tag, at in want.items():
        segs, _ = consensus_cases.read("empties.%s" % tag)
        assert [i for i, s in enumerate(segs) if not s] == at == consensus_cases.info("empties.%s" % tag)["empty"]
        assert len(segs) == (5 if tag == "all" else 14 + len(at))
        for kernal in ("glue", "stick"):
            r = consensus_ref.consensus(segs, None, kernal)
            assert (r["length"] == 0) == (tag == "all")
            for i in at:                                  # an empty segment moves on by its predecessor's length; its successor by 0
                if i + 1 < len(segs):
                    assert r["start"][i + 1] == r["start"][i]


def test_chunk_counts_straddle_the_scan_s_chunks():
    assert consensus_cases.CHUNK == 1024
    for n in consensus_cases.CHUNK_COUNTS:
        segs, _ = consensus_cases.read("chunks.n%d" % n)
        assert len(segs) == n and {len(s) for s in segs} <= set(range(1, 13))
        assert n < 20 or {len(s) for s in segs} == set(range(1, 13))
    assert {n % 1024 for n in consensus_cases.CHUNK_COUNTS} == {2, 1023, 0, 1} and max(consensus_cases.CHUNK_COUNTS) > 3 * 1024


def _voters(r, lens, col):
    return [s for s in range(len(lens)) if r["start"][s] <= col < r["start"][s] + lens[s]]


def test_longest_late_has_its_longest_segment_in_a_later_chunk(ref):
    for name, at, chunk, partial, n_seg in (("index1500", 1500, 1, False, 2501), ("index2300", 2300, 2, True, 2501),
                                            ("crossed", 1500, 1, False, 2503)):
        name = "longest_late.%s" % name
        segs, _ = consensus_cases.read(name)
        lens = [len(s) for s in segs]
        assert len(segs) == n_seg and int(np.argmax(lens)) == at == consensus_cases.info(name)["longest"] > 1024
        assert lens[at] == 600 and min(lens) == 1 and sorted(lens)[-2] == (30 if name.endswith("crossed") else 3)
        assert sum(n > 3 for n in lens) == (2 if name.endswith("crossed") else 1)
        assert at // 1024 == chunk and ((chunk + 1) * 1024 > len(segs)) == partial
        r = ref[name, "glue"]
        start = r["start"]
        # the vote of ANY column walks back over every segment that starts less than maxn = 600 columns before it: hundreds
        col = int(start[at]) - 1
        assert int(((start > col - 600) & (start <= col)).sum()) > 250
        # the result DEPENDS on maxn where a column's earliest voter starts more than 3 columns (the next longest tiny segment)
        # before it and is not the last segment to start at or before it: the long segment's last columns, shared with its successor
        overlaps = _overlaps(name)
        assert overlaps[at + 1] >= 1
        end = int(start[at]) + 599
        assert _voters(r, lens, end)[:2] == [at, at + 1] and r["n1"][end] >= 2 and end - int(start[at]) > 3
        shared = np.flatnonzero(r["n1"] >= 2)
        first = {_voters(r, lens, c)[0] for c in shared}          # columns are shared behind the long segment and nowhere else
        assert first == ({at, at + 1} if name.endswith("crossed") else {at})
        if name.endswith("crossed"):                     # the walk back from the last voter crosses a segment to reach the long one
            assert overlaps[at + 1:at + 3] == [29, 2] and _voters(r, lens, end) == [at, at + 1, at + 2] and r["n1"][end] == 3
        else:
            assert overlaps[at + 1] == 2 and lens[at + 1] == 3
        assert (ref[name, "stick"]["n1"] == 1).all()


def test_every_read_that_can_disagree_in_a_column_has_a_tied_column(ref):
    """A column with n1 == n2 is where the base (first maximum), n2 (with multiplicity) and q_top (last maximum) part ways.  Two
    segments share a column only under glue and only behind a predecessor of 20 bases or more (floor(0.1 * prev_n) >= 2): the
    chunk reads (1..12 bases) and every read under stick hold exactly one vote per column, which is asserted for them instead.
    The longest_late reads share columns (asserted above) but cannot disagree in one: a 3-base segment is tried at overlaps 1
    and 2 only, and a mismatch leaves neither a positive score."""
    tied_reads = []
    for (name, kernal), r in ref.items():
        if r["length"] == 0:
            continue
        if name.startswith("chunks") or kernal == "stick":
            assert (r["n1"] == 1).all() and (r["n2"] == 0).all(), (name, kernal)
        elif name.startswith("longest_late"):
            assert (r["n1"] >= 2).any() and (r["n2"] == 0).all(), (name, kernal)
        else:
            cols = np.flatnonzero((r["n1"] == r["n2"]) & (r["n1"] >= 1))
            assert cols.size, (name, kernal)
            # the quality comes from another base than the one called
            assert (r["qsum"][r["base"][cols], cols] != r["q_top"][cols]).any(), (name, kernal)
            tied_reads.append(name)
    assert tied_reads == ["long_overlaps", "clamp", "ties"] + ["empties.%s" % t for t in ("first", "second", "middle", "two_in_a_row", "last")]
