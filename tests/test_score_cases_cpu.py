"""CPU: the rows of tests/score_cases.py are what the GPU test of Engine.score's edit distance needs them to be.  Every designed
row has the distance its name claims, decided by plain dynamic programming (ctc.levenshtein), every word count of the kernel has
a row whose distance is small and one whose distance is large, the rendered logits decode to the hypotheses, and the rows sit
where the kernel's 64-row blocks and the SparseTensor's ends are."""
import numpy as np
import pytest

from chiron_amd import assembly, ctc

import score_cases

T = 400


@pytest.fixture(scope="module")
def rows():
    return score_cases.edit_cases(T)


@pytest.fixture(scope="module")
def dist(rows):
    return {name: ctc.levenshtein(hyp, truth) for name, hyp, truth in rows}


def test_every_row_has_the_distance_its_name_claims(rows, dist):
    claim = score_cases.claims(T)
    assert sorted(claim) == sorted(dist) and len(dist) == len(rows)          # names are unique
    for name, (lo, hi) in claim.items():
        assert lo <= dist[name] <= hi, (name, dist[name], lo, hi)
    by = {name: (hyp, truth) for name, hyp, truth in rows}
    for m in score_cases.LENGTHS:
        if m <= T // 2:
            assert dist["exact_m%d" % m] == 0 and dist["ins_first_m%d" % m] == 1 and dist["del_first_m%d" % m] == 1
            assert dist["del_first_ins_last_m%d" % m] == (2 if m >= 2 else 1)
            assert dist["sub_word_edges_m%d" % m] == len([i for i in (63, 64, 127, 128, 191, 192) if i < m])
            assert by["del_first_m%d" % m][0] == by["exact_m%d" % m][1][1:]
        else:
            assert dist["exact_m%d" % m] == m - 200 and by["exact_m%d" % m][0] == by["exact_m%d" % m][1][:200]
            for tag in ("head", "tail"):
                assert dist["del_first_m%d_%s" % (m, tag)] == m - 199
        hyp, truth = by["unrelated_m%d" % m]
        assert len(truth) == m and len(hyp) == min(m, 200)
    for name, (hyp, truth) in by.items():
        assert all(0 <= c <= 3 for c in hyp + truth) and len(truth) <= score_cases.LMAX and len(hyp) <= T
        if name.startswith("homopolymer") or name.startswith("period2"):
            assert set(hyp) == {0} and len(truth) in (128, 192, 256) and len(hyp) != len(truth)
            assert truth == ([0] * len(truth) if name.startswith("homopolymer") else [0, 1] * (len(truth) // 2))
        if name.startswith("infix"):
            m = len(truth)
            assert len(hyp) == T and m in (65, 129) and any(hyp[o:o + m] == truth for o in range(1, T - m))
            assert dist[name] == T - m
    assert dist["empty_truth"] == 40 and by["empty_truth"][1] == [] and by["both_empty"] == ([], [])
    for m in (1, 64, 65, 320):
        assert by["empty_hyp_m%d" % m][0] == [] and len(by["empty_hyp_m%d" % m][1]) == m


def test_the_row_wise_distance_is_the_plain_one(rows, dist):
    hyps = [hyp for _, hyp, _ in rows]
    labels, ll = score_cases.dense_truths(rows)
    assert [score_cases.levenshtein_rows(hyp, truth) for _, hyp, truth in rows] == [dist[name] for name, _, _ in rows]
    want = [ctc.normalized_edit_distance([], []) if not truth and not hyp else np.float32(np.inf) if not truth
            else np.float32(dist[name]) / np.float32(len(truth)) for name, hyp, truth in rows]
    assert score_cases.normalized(hyps, labels, ll).tobytes() == np.asarray(want, dtype=np.float32).tobytes()
    assert want[[name for name, _, _ in rows].index("empty_truth")] == ctc.normalized_edit_distance([1], [])
    ll64 = np.minimum(ll, 64)
    assert score_cases.normalized(hyps, labels[:, :64], ll64).tobytes() == ctc.edit_distance(hyps, labels[:, :64], ll64).tobytes()
    rng = np.random.default_rng(6)
    for _ in range(200):
        a, b = rng.integers(0, 3, int(rng.integers(0, 12))).tolist(), rng.integers(0, 3, int(rng.integers(0, 12))).tolist()
        assert score_cases.levenshtein_rows(a, b) == ctc.levenshtein(a, b), (a, b)


def test_every_word_count_has_a_small_and_a_large_distance(rows, dist):
    small, large = set(), set()
    for name, hyp, truth in rows:
        m = len(truth)
        if m and hyp:
            words = (m + 63) // 64
            if dist[name] <= 3:
                small.add(words)
            if 2 * dist[name] >= m:
                large.add(words)
    assert small == large == {1, 2, 3, 4, 5}
    # a truth that ends on bit 63 of its last word, at every word count it can, one or two edits away
    for m in (64, 128, 192):
        assert dist["del_first_m%d" % m] == 1 and dist["del_first_ins_last_m%d" % m] == 2
    assert dist["norepeat_del_first_m320"] == 1 and dist["norepeat_sub_m257"] == 3


def test_the_logits_decode_to_the_hypotheses(rows):
    hyps = [hyp for _, hyp, _ in rows]
    lg = score_cases.greedy_logits(hyps, T)
    assert lg.shape == (len(rows), T, 5) and lg.dtype == np.float32
    assert sorted(set(lg.ravel().tolist())) == [-4.0, 4.0, 6.0]
    path = lg.argmax(axis=2)
    for r, hyp in enumerate(hyps):
        assert assembly.mapping(path[r]).tolist() == hyp, rows[r][0]
    with pytest.raises(ValueError):
        score_cases.greedy_logits([[0, 0] + [1, 2] * 100], T)          # 202 bases with a repeat cannot be rendered


def test_the_rows_sit_at_the_block_edges_and_the_ends(rows):
    B = len(rows)
    assert B > 130                                                      # three 64-row blocks, the last one partial
    filler = [r for r in range(B) if rows[r][0].startswith("filler")]
    assert len(filler) == score_cases.N_FILLER and all(20 <= len(rows[r][1]) <= 60 and 20 <= len(rows[r][2]) <= 60 for r in filler)
    for at in score_cases.PINNED_DESIGNED:
        name, hyp, truth = rows[at]
        assert hyp and len(truth) > 64 and not name.startswith("filler"), (at, name)
    assert [r % B for r in score_cases.PINNED_DESIGNED] == [0, 63, 64, 127, 128, B - 1]
    for at in score_cases.PINNED_EMPTY_HYP:
        name, hyp, truth = rows[at]
        assert hyp == [] and len(truth) > 64 and rows[at - 1][1] and rows[at + 1][1], (at, name)
    assert [r % B for r in score_cases.PINNED_EMPTY_HYP] == [1, B - 2]
    labels, ll = score_cases.dense_truths(rows)
    assert labels.shape == (B, 320) and ll.max() == 320 and [labels[b, :ll[b]].tolist() for b in range(B)] == [t for _, _, t in rows]
    # cut to 64 positions, every multi-word row becomes a one-word row whose truth ends on bit 63
    assert int((np.minimum(ll, 64) == 64).sum()) > 80
