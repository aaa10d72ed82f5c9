"""CPU: the numpy restatement of chiron_ctc_score against brute force, the host-side pieces of chiron_amd.polish (segment,
candidates_from_counts, decide, apply), the refusals of the two entry points that are decided before a device is needed, and the
whole pipeline on the references through the scorer= and frame_aligner= hooks."""
import ctypes as C
import itertools

import numpy as np
import pytest

from chiron_amd import _lib, assess, map as cmap, pileup, polish

import assess_ref
import pileup_ref
import polish_cases as cases
import polish_ref


def _codes(s):
    return np.array(["ACGT".index(c) for c in s], dtype=np.uint8)


# ----------------------------------------------------------------------------------------------------------------------------
# the reference
# ----------------------------------------------------------------------------------------------------------------------------
def test_reference_equals_brute_force():
    """Every label over ACGT of L <= 3 (repeats included, L = 0 included) at every T <= 6: the recurrence equals the sum over all
    paths, and an infeasible pair has no path."""
    rng = np.random.default_rng(300)
    seen_infeasible = 0
    for L in range(4):
        for lab in itertools.product(range(4), repeat=L):
            lab = np.array(lab, dtype=np.uint8)
            for T in range(7):
                lp = polish_ref.log_softmax(rng.normal(0, 3, (T, 5)).astype(np.float32))
                got, status = polish_ref.score_one(lp, lab)
                want = polish_ref.brute_force(lp, lab)
                if status == 1:
                    seen_infeasible += 1
                    assert got == -np.inf and want == -np.inf
                    assert T < L + int(np.count_nonzero(lab[1:] == lab[:-1]))
                else:
                    assert np.isfinite(got) and abs(got - want) <= 1e-12 * max(1.0, abs(want)), (lab, T)
    assert seen_infeasible > 100
    assert polish_ref.score_one(np.zeros((0, 5)), _codes("")) == (0.0, 0)
    lp = polish_ref.log_softmax(rng.normal(0, 3, (5, 5)).astype(np.float32))
    assert abs(polish_ref.score_one(lp, _codes(""))[0] - lp[:, 4].sum()) < 1e-12
    assert np.allclose(np.exp(lp).sum(axis=1), 1.0, atol=1e-14)


def test_batch_reference_equals_the_plain_one():
    rng = np.random.default_rng(301)
    x = rng.normal(0, 3, (300, 5)).astype(np.float32)
    lp = polish_ref.log_softmax(x)
    items, cands = [], []
    for k in range(40):
        b = int(rng.integers(0, 280))
        e = int(rng.integers(b, min(b + 25, 300) + 1))
        items.append((b, e))
        cands.append([rng.integers(0, 2 if k % 2 else 4, int(rng.integers(0, 12))).astype(np.uint8) for _ in range(k % 4)])
    got = polish_ref.score(x, items, cands)
    seen = set()
    for (b, e), ls, ll, st in zip(items, cands, got["loglik"], got["status"]):
        assert ll.dtype == np.float64 and st.dtype == np.int32 and len(ll) == len(st) == len(ls)
        for lab, v, s in zip(ls, ll, st):
            want, ws = polish_ref.score_one(lp[b:e], lab)
            seen.add((ws, e - b == 0, len(lab) == 0))
            assert s == ws and (v == want if not np.isfinite(want) else abs(v - want) <= 1e-12 * max(1.0, abs(want)))
    assert {(0, False, False), (1, False, False), (0, False, True)} <= seen
    assert polish_ref.score(x, [], []) == {"loglik": [], "status": []}


# ----------------------------------------------------------------------------------------------------------------------------
# segment, candidates, decision, apply
# ----------------------------------------------------------------------------------------------------------------------------
def test_segment_on_hand_made_columns():
    ops = pileup.ops_from_cigar("3=1D2=2I3=1D1=")          # reference 100 .. 110, read bases 0 .. 10
    #  ref  100 101 102 103 104 105        106 107 108 109 110
    #  read   0   1   2   D   3   4  5i 6i   7   8   9   D  10
    n, m = 11, 11
    assert polish.read_prefix(ops).tolist() == [0, 1, 2, 3, 3, 4, 7, 8, 9, 10, 10, 11]
    assert polish.segment(100, ops, n, 100, 100 + m) == (0, 11)                # the whole alignment; ends exactly at pos + m
    assert polish.segment(100, ops, n, 103, 106) == (3, 7)                     # a D at the left edge; the insertion after 105 is inside
    assert polish.segment(100, ops, n, 101, 104) == (1, 3)                     # a D at the right edge (the last position inside)
    assert polish.segment(100, ops, n, 101, 103) == (1, 3)                     # ... and just outside: the same read bases
    assert polish.segment(100, ops, n, 106, 109) == (7, 10)                    # an I directly before the left edge belongs to 105: outside
    assert polish.segment(100, ops, n, 104, 105) == (3, 4) and polish.segment(100, ops, n, 104, 106) == (3, 7)   # an I next to the right edge
    assert polish.segment(100, ops, n, 109, 110) == (10, 10)                   # only a D: no read base
    assert polish.segment(100, ops, n, 109, 111) == (10, 11) and polish.segment(100, ops, n, 111, 111) == (11, 11)
    for g0, g1 in ((99, 105), (105, 112), (98, 99), (112, 113), (106, 105)):   # not covered
        assert polish.segment(100, ops, n, g0, g1) is None
    with pytest.raises(ValueError):
        polish.segment(100, ops, n + 1, 100, 105)
    # trailing 'I' columns (clipping in the pileup) count only when the window ends at pos + m
    tail = pileup.ops_from_cigar("2I3=2I")
    assert polish.segment(5, tail, 7, 5, 8) == (2, 7) and polish.segment(5, tail, 7, 5, 7) == (2, 4) and polish.segment(5, tail, 7, 6, 8) == (3, 7)
    before = polish.read_prefix(ops)                                           # handed in by a caller that asks for many windows
    assert polish.segment(100, ops, n, 103, 106, before) == (3, 7)


def test_read_window_with_soft_clips_on_either_strand():
    """read_window is what polish() cuts every read with: segment(), moved past the leading soft clip, mirrored for a reverse read.
    The SAM SEQ (genome orientation) is 3 clipped + 11 aligned + 2 clipped bases; a reverse read's called sequence is its reverse
    complement, so its leading clip of 3 lies at the END of the called sequence."""
    ops = pileup.ops_from_cigar("3=1D2=2I3=1D1=")          # as in test_segment_on_hand_made_columns: reference 100 .. 110
    rng = np.random.default_rng(302)
    seq = rng.integers(0, 4, 16).astype(np.uint8)          # genome orientation, clips included
    aligned = seq[3:14]
    fwd = {"name": "f", "pos": 100, "ops": ops, "reverse": False, "lead": 3, "called": seq}
    rev = dict(fwd, name="r", reverse=True, called=assess.reverse_complement(seq))
    for (g0, g1), (i_lo, i_hi) in (((100, 111), (0, 11)), ((103, 106), (3, 7)), ((106, 109), (7, 10)), ((101, 104), (1, 3)), ((109, 110), (10, 10))):
        assert polish.segment(100, ops, 11, g0, g1) == (i_lo, i_hi)
        lo, hi = polish.read_window(fwd, g0, g1)
        assert (lo, hi) == (3 + i_lo, 3 + i_hi) and np.array_equal(fwd["called"][lo:hi], aligned[i_lo:i_hi])
        lo, hi = polish.read_window(rev, g0, g1, polish.read_prefix(ops))
        assert (lo, hi) == (16 - 3 - i_hi, 16 - 3 - i_lo)
        assert np.array_equal(assess.reverse_complement(rev["called"][lo:hi]), aligned[i_lo:i_hi])      # the same bases, read backwards
    assert polish.read_window(fwd, 99, 105) is None and polish.read_window(rev, 105, 112) is None
    for bad in (dict(fwd, lead=6), dict(rev, called=rev["called"][:13]), dict(fwd, lead=-1)):
        with pytest.raises(ValueError):
            polish.read_window(bad, 100, 105)


def _planes(G, **at):
    counts = np.zeros((pileup.PLANES, G), dtype=np.int32)
    for key, v in at.items():
        plane, g = key.split("_")
        counts[{"A": 0, "C": 1, "G": 2, "T": 3, "N": 4, "D": pileup.PLANE_DEL, "iA": pileup.PLANE_INS, "iC": pileup.PLANE_INS + 1,
                "iG": pileup.PLANE_INS + 2, "iT": pileup.PLANE_INS + 3, "iN": pileup.PLANE_INS + 4, "i2A": pileup.PLANE_INS + 5}[plane], int(g)] = v
    return counts


def test_candidates_from_counts_clause_by_clause():
    genome = cmap.Genome([("c", "AAAAAAAANA")])
    counts = _planes(10, A_0=8, C_0=2,                 # depth 10: 2 >= max(2, ceil(2.0)) -> kept (0.2 * 10 must not round up to 3)
                     A_1=9, C_1=1, G_1=2,               # depth 12: ceil(2.4) = 3 -> G's 2 is below min_frac
                     A_2=2, T_2=1,                      # depth 3: T's 1 is below min_alt
                     A_3=3, D_3=2,                      # the deletion
                     A_4=5, iC_4=2, iT_4=1, i2A_4=5,    # insertion slot 0 by base; slot 1 is not a candidate
                     A_5=4, C_5=4, G_5=2, T_5=2, D_5=3, iA_5=3, iG_5=3,   # everything at once, in order
                     A_6=7,                             # the reference base alone is no candidate
                     N_7=5, A_7=1,                      # N is no candidate
                     C_8=9, D_8=9)                      # reference code 4: skipped
    depth = counts[:5].sum(axis=0) + counts[pileup.PLANE_DEL]
    got = polish.candidates_from_counts(counts, depth, genome)
    assert [(c["g"], c["type"], c["alt"], c["count"], c["depth"]) for c in got] == [
        (0, "SUB", 1, 2, 10), (3, "DEL", -1, 2, 5), (4, "INS", 1, 2, 5),
        (5, "SUB", 1, 4, 15), (5, "DEL", -1, 3, 15), (5, "INS", 0, 3, 15), (5, "INS", 2, 3, 15)]
    assert polish.threshold([0, 3, 5, 10, 11, 15, 16]).tolist() == [2, 2, 2, 2, 3, 3, 4]
    looser = polish.candidates_from_counts(counts, depth, genome, min_alt=1, min_frac=0.0)
    assert {(c["g"], c["type"], c["alt"]) for c in looser} >= {(1, "SUB", 1), (1, "SUB", 2), (2, "SUB", 3), (4, "INS", 3), (5, "SUB", 2), (5, "SUB", 3)}
    assert not any(c["g"] in (6, 8) for c in looser) and not any(c["g"] == 7 and c["alt"] == 4 for c in looser)
    assert polish.candidates_from_counts(np.zeros_like(counts), np.zeros(10, np.int32), genome, min_alt=0) == []


def test_the_votes_winning_calls_are_candidates():
    """Random planes without N: with min_alt = 1 a winning substitution or deletion has at least a fifth of the depth, so it is in
    the list whatever the counts are."""
    rng = np.random.default_rng(303)
    G = 400
    genome = cmap.Genome([("c", assess_ref.random_seq(G, rng))])
    counts = np.zeros((pileup.PLANES, G), dtype=np.int32)
    counts[:4] = rng.integers(0, 6, (4, G))
    counts[pileup.PLANE_DEL] = rng.integers(0, 7, G)
    depth, call = pileup_ref.call_tile(counts, genome.codes, 3)
    have = {(c["g"], c["type"], c["alt"]) for c in polish.candidates_from_counts(counts, depth, genome, min_alt=1)}
    won = pileup.variants(call, depth, counts, genome)
    assert len(won) > 200
    for v in won:
        assert (v["pos"] - 1, v["type"], "ACGT".index(v["alt"]) if v["type"] == "SUB" else -1) in have, v


def _rec(g, llr, n=5, kind="SUB", alt=1):
    return {"g": g, "type": kind, "alt": alt, "reads_scored": n, "llr": llr}


def test_greedy_acceptance():
    recs = [_rec(100, 5.0), _rec(104, 9.0), _rec(109, 4.0), _rec(113, 1.0), _rec(200, 0.0), _rec(210, -3.0), _rec(220, 8.0, n=2),
            _rec(300, 2.0, kind="INS"), _rec(300, 2.0, kind="DEL", alt=-1), _rec(300, 2.0), _rec(300, 2.0, alt=0), _rec(292, 2.0)]
    took = polish.decide(recs, flank=8)
    # 104 is best; 100 and 109 lie within 8 of it; 113 is 9 away from 104 and 4 from the rejected 109: taken.  0.0 is not above the
    # threshold; two reads are too few.  Equal llr: the smaller position first (292 blocks 300)
    assert [(r["g"], r["type"]) for r in took] == [(104, "SUB"), (113, "SUB"), (292, "SUB")]
    assert [r["accepted"] for r in recs] == [False, True, False, True] + [False] * 7 + [True]
    took = polish.decide(recs[7:11], flank=8)                   # equal llr at one position: SUB before DEL before INS, then the code
    assert [(r["g"], r["type"], r["alt"]) for r in took] == [(300, "SUB", 0)]
    assert [r["g"] for r in polish.decide(recs, flank=8, min_reads=2, min_llr=-5.0)] == [104, 113, 200, 210, 220, 292]
    assert [r["g"] for r in polish.decide(recs[:4], flank=3)] == [100, 104, 109, 113]
    assert polish.decide([], 8) == []


def test_apply_round_trips_through_the_edit_distance():
    rng = np.random.default_rng(304)
    given = [("one", assess_ref.random_seq(300, rng)), ("two", assess_ref.random_seq(200, rng))]
    genome = cmap.Genome(given)
    assert polish.apply(genome, []) == dict(given)
    accepted, kinds = [], ("SUB", "DEL", "INS")
    for k, g in enumerate(list(range(5, 300, 23)) + list(range(300 + cmap.SEPARATOR + 4, len(genome.codes), 31))):
        kind = kinds[k % 3]
        alt = -1 if kind == "DEL" else int((genome.codes[g] + 1 + k % 3) % 4)
        accepted.append({"g": g, "type": kind, "alt": alt})
    out = polish.apply(genome, accepted)
    per = {name: sum(1 for r in accepted if genome.names[genome.contig_of(r["g"])] == name) for name, _ in given}
    assert sum(per.values()) == len(accepted) and min(per.values()) > 4
    for name, seq in given:
        assert assess_ref.full_table(out[name], seq)[0] == per[name]        # edits 23 apart: none cancels another
        assert len(out[name]) == len(seq) + sum((r["type"] == "INS") - (r["type"] == "DEL") for r in accepted
                                                if genome.names[genome.contig_of(r["g"])] == name)
    first, last = {"g": 0, "type": "DEL", "alt": -1}, {"g": 299, "type": "INS", "alt": 2}
    out = polish.apply(genome, [first, last])
    assert out["one"] == given[0][1][1:] + "G" and out["two"] == given[1][1]
    with pytest.raises(ValueError):
        polish.apply(genome, [first, dict(first, type="SUB", alt=1)])
    cd = {"g": 300 + cmap.SEPARATOR + 8, "type": "INS", "alt": 3}
    ref, alt = polish.alleles(genome, cd, 8)
    assert cmap.decode(ref) == given[1][1][:17] and cmap.decode(alt) == given[1][1][:9] + "T" + given[1][1][9:17]
    assert polish.alleles(genome, dict(cd, g=cd["g"] - 1), 8) is None and polish.alleles(genome, {"g": 292, "type": "SUB", "alt": 0}, 8) is None
    assert cmap.decode(polish.alleles(genome, {"g": 291, "type": "DEL", "alt": -1}, 8)[1]) == given[0][1][283:291] + given[0][1][292:300]


# ----------------------------------------------------------------------------------------------------------------------------
# the entry points' refusals
# ----------------------------------------------------------------------------------------------------------------------------
def test_size_function(built):
    lib = _lib.load()
    n = C.c_size_t()
    size = lambda *a: (lib.chiron_ctc_score_workspace_size(*a, C.byref(n)), n.value)
    assert size(0, 0, 0, 0) == (_lib.OK, 0) and size(1000, 0, 0, 0) == (_lib.OK, 0) and size(1000, 5, 0, 0) == (_lib.OK, 0)
    st, nbytes = size(1000, 10, 20, 340)
    assert st == _lib.OK and 1000 * 5 * 12 + 20 * 36 + 340 <= nbytes <= 1000 * 5 * 12 + 20 * 36 + 340 + 6 * 256
    assert polish.workspace_size(1000, 10, 20, 340) == nbytes
    assert size(1000, 1 << 24, 20, 340)[1] == nbytes                   # items cost nothing
    for k, base in enumerate((1000, None, 20, 340)):                   # monotone in frames, candidates and label bytes
        if base is not None:
            prev = 0
            for v in (base, base + 1, base + 300):
                args = [1000, 10, 20, 340]
                args[k] = v
                st, got = size(*args)
                assert st == _lib.OK and got >= prev
                prev = got
    for bad in ((-1, 1, 1, 0), (1, -1, 1, 0), (1, 1, -1, 0), (1, 1, 1, -1)):
        assert size(*bad)[0] == _lib.ERR_INVALID and b"negative size" in lib.chiron_last_error()
    for bad, text in (((1, (1 << 24) + 1, 1, 0), b"16777217 items in one call, at most 2^24"),
                      ((1, 1, (1 << 24) + 1, 0), b"16777217 candidates in one call, at most 2^24"),
                      (((1 << 40) + 1, 1, 1, 0), b"1099511627777 frames in one call, at most 2^40"),
                      ((1, 1, 2, 255), b"255 label bytes for 2 candidates of at most 127 bases")):
        assert size(*bad)[0] == _lib.ERR_OVERFLOW and text in lib.chiron_last_error(), bad
    assert lib.chiron_ctc_score_workspace_size(1, 1, 1, 1, None) == _lib.ERR_INVALID


def _good():
    """A good call of two items and three candidates, as a dict in the prototype's order."""
    return {"device_id": 0, "scores": np.zeros(50, np.float32), "frames": 10, "item_begin": [0, 4], "item_end": [6, 10], "cand_off": [0, 2, 3],
            "items": 2, "labels": np.array([0, 1, 2, 3, 0, 0], np.uint8), "label_off": [0, 2, 4, 6], "candidates": 3, "flags": 0,
            "loglik_out": np.zeros(3, np.float64), "status_out": np.zeros(3, np.int32), "workspace": np.zeros(64, np.uint8), "stream": None}


def _nan_scores(v):
    x = np.zeros(50, np.float32)
    x[37] = v
    return x


REFUSALS = {
    "unknown_flags": ({"flags": 4}, 1, "chiron_ctc_score: unknown flags 0x4"),
    "negative_frames": ({"frames": -1}, 1, "chiron_ctc_score: negative size (frames -1, items 2, candidates 3, label bytes 0)"),
    "too_many_candidates": ({"candidates": (1 << 24) + 1}, 4, "chiron_ctc_score: 16777217 candidates in one call, at most 2^24"),
    "too_many_items": ({"items": (1 << 24) + 1}, 4, "chiron_ctc_score: 16777217 items in one call, at most 2^24"),
    "null_offsets": ({"cand_off": None}, 1, "chiron_ctc_score: null offsets"),
    "null_output": ({"status_out": None}, 1, "chiron_ctc_score: null output"),
    "null_scores": ({"scores": None}, 1, "chiron_ctc_score: null scores"),
    "cand_off_first": ({"cand_off": [1, 2, 3]}, 1, "chiron_ctc_score: cand_off[0] = 1, the first item's candidates start at 0"),
    "negative_first_label_offset": ({"label_off": [-1, 2, 4, 6]}, 1, "chiron_ctc_score: label_off[0] = -1 is negative"),
    "decreasing_cand_off": ({"cand_off": [0, 2, 1]}, 1, "chiron_ctc_score: cand_off[2] = 1 below its predecessor 2"),
    "cand_off_past": ({"cand_off": [0, 2, 4]}, 1, "chiron_ctc_score: cand_off[2] = 4 past the 3 candidates"),
    "cand_off_short": ({"cand_off": [0, 2, 2]}, 1, "chiron_ctc_score: cand_off[2] = 2, the items own 3 candidates"),
    "item_negative": ({"item_begin": [-1, 4]}, 1, "chiron_ctc_score: item 0 covers frames -1 .. 6, outside 0 .. 10"),
    "item_reversed": ({"item_begin": [0, 11], "item_end": [6, 10]}, 1, "chiron_ctc_score: item 1 covers frames 11 .. 10, outside 0 .. 10"),
    "item_past_frames": ({"item_end": [6, 11]}, 1, "chiron_ctc_score: item 1 covers frames 4 .. 11, outside 0 .. 10"),
    "item_too_long": ({"scores": np.zeros(5 * 5000, np.float32), "frames": 5000, "item_end": [6, 4101]}, 4,
                      "chiron_ctc_score: item 1 has 4097 frames, at most 4096"),
    "decreasing_label_off": ({"label_off": [0, 2, 1, 6]}, 1, "chiron_ctc_score: label_off[2] = 1 below its predecessor 2"),
    "label_too_long": ({"labels": np.zeros(200, np.uint8), "label_off": [0, 2, 130, 132]}, 4, "chiron_ctc_score: candidate 1 has 128 bases, at most 127"),
    "code_out_of_range": ({"labels": np.array([0, 1, 2, 3, 4, 0], np.uint8)}, 1, "chiron_ctc_score: code 4 at base 4 outside 0..3"),
    "nan_score": ({"scores": _nan_scores(np.nan)}, 1, "chiron_ctc_score: score 2 of frame 7 is not finite"),
    "inf_score": ({"scores": _nan_scores(-np.inf)}, 1, "chiron_ctc_score: score 2 of frame 7 is not finite"),
    "null_labels": ({"labels": None}, 1, "chiron_ctc_score: null labels"),
    "null_workspace": ({"workspace": None}, 1, "chiron_ctc_score: null workspace"),
    "no_device": ({"device_id": -1}, 2, "no HIP device -1: libchiron_amd has no CPU fallback"),
}


@pytest.mark.parametrize("check", sorted(REFUSALS))
def test_refusal_status_and_text(built, check):
    lib = _lib.load()
    change, status, text = REFUSALS[check]
    args = _good()
    args.update(change)
    keep = [np.asarray(v, dtype=np.int64) if isinstance(v, list) else v for v in args.values()]
    raw = [v.ctypes.data if isinstance(v, np.ndarray) else v for v in keep]
    assert (lib.chiron_ctc_score(*raw), lib.chiron_last_error().decode()) == (status, text)


def test_no_ops_touch_nothing(built):
    lib = _lib.load()
    for change in ({"items": 0}, {"candidates": 0}, {"items": 0, "candidates": 0, "frames": 0}):
        args = dict(_good(), workspace=None, device_id=-1, cand_off=None, loglik_out=None, **change)
        keep = [np.asarray(v, dtype=np.int64) if isinstance(v, list) else v for v in args.values()]
        assert lib.chiron_ctc_score(*[v.ctypes.data if isinstance(v, np.ndarray) else v for v in keep]) == _lib.OK
    assert polish.plan_batches([], [], 1 << 20) == []
    labs = [[np.zeros(17, np.uint8)] * 2] * 6
    items = [(0, 50), (40, 90), (1000, 1050), (1040, 1100), (5000, 5050), (5010, 5060)]
    assert polish.plan_batches(items, labs, 1 << 30) == [(0, 6, 0, 5060)]
    runs = polish.plan_batches(items, labs, polish.workspace_size(110, 2, 4, 68))
    assert runs == [(0, 2, 0, 90), (2, 4, 1000, 1100), (4, 6, 5000, 5060)]
    assert [r[:2] for r in polish.plan_batches(items, labs, 1)] == [(k, k + 1) for k in range(6)]       # an item alone always goes


# ----------------------------------------------------------------------------------------------------------------------------
# the pipeline on the references
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def end_to_end(built):
    truth, draft, called, logits, seeds = cases.end_to_end_case()
    genome, piled, out = cases.reference_pipeline(draft, called, logits, seeds)
    return truth, draft, genome, piled, out


def test_end_to_end_on_the_references(end_to_end):
    """map_reads(aligner=map_ref), add_cigars(tracer=trace_ref), count(counter=pileup_ref), polish(scorer=polish_ref,
    frame_aligner=ctc_align_ref) on the planted case, seed 5: one round of polishing brings the draft closer to the truth.  Measured
    with the references alone: the draft has 30 edits against the truth (summed over the two contigs), the vote's consensus 7, the
    polished sequence 9.  Whether polished beats the vote depends on the seed (seeds 1 .. 7: 36 / 16 / 9, 42 / 17 / 11, 42 / 7 / 10,
    38 / 14 / 8, 30 / 7 / 9, 40 / 11 / 12, 40 / 15 / 12 for draft / vote / polished); only polished < draft is asserted."""
    truth, draft, genome, piled, out = end_to_end
    rep = out["report"]
    assert rep["reads"] == {"total": 60, "used": 60, "dropped": {reason: 0 for reason in polish.READ_DROPS}}
    assert rep["items"]["total"] == rep["items"]["scored"] + sum(rep["items"]["dropped"].values())
    assert rep["candidates"]["total"] == rep["candidates"]["scored"] + sum(rep["candidates"]["skipped"].values()) == len(out["variants"]) > 100
    assert rep["items"]["scored"] == sum(r["reads_scored"] for r in out["variants"]) > 1000
    assert rep["accepted"]["total"] == len(out["accepted"]) == sum(r["accepted"] for r in out["variants"])
    polished = polish.apply(genome, out["accepted"])
    before = cases.edits_against(truth, dict(draft))
    vote = cases.edits_against(truth, pileup.consensus(piled["call"], genome))
    after = cases.edits_against(truth, polished)
    print("edits against the truth: draft %d, pileup consensus %d, polished %d" % (before, vote, after))
    assert after < before
    # the seed leaves no candidate on the threshold: the GPU test compares the accepted set without leaving any out
    assert not [r for r in out["variants"] if r["reads_scored"] and abs(r["llr"] - rep["min_llr"]) <= 1e-6]
    # accepted variants keep their distance, and each was eligible
    gs = [r["g"] for r in out["accepted"]]
    assert all(b - a > rep["flank"] for a, b in zip(gs, gs[1:]))
    assert all(r["reads_scored"] >= 3 and r["llr"] > 0 for r in out["accepted"])
    # the vote's own calls are candidates wherever their count meets the candidate threshold (reads without N)
    have = {(c["g"], c["type"], c["alt"]) for c in out["variants"]}
    thr = polish.threshold(piled["depth"])
    won = pileup_ref.variants(piled["call"], piled["depth"], piled["counts"], genome.codes, genome.names, genome.starts, genome.lengths)
    checked = 0
    for v in won:
        g = int(genome.starts[genome.names.index(v["contig"])]) + v["pos"] - 1
        code = "ACGT".index(v["alt"][0]) if v["type"] != "DEL" else -1
        count = int(piled["counts"][polish._plane(v["type"], code), g])
        if count >= thr[g]:
            checked += 1
            assert (g, v["type"], code) in have, v
    assert checked >= len(won) - 2 and checked > 20


def test_outputs(end_to_end, tmp_path):
    truth, draft, genome, piled, out = end_to_end
    report = polish.write_outputs(str(tmp_path), out, genome, {"genome": "draft.fa"})
    again = cmap.load_genome(str(tmp_path / "polished.fasta"))
    assert again.names == genome.names and dict(zip(again.names, [cmap.decode(again.codes[s:s + n]) for s, n in zip(again.starts, again.lengths)])) \
        == polish.apply(genome, out["accepted"])
    lines = (tmp_path / "polish_variants.tsv").read_text().splitlines()
    assert lines[0].split("\t") == list(polish.VARIANT_COLUMNS) and len(lines) == 1 + len(out["variants"])
    rows = [dict(zip(polish.VARIANT_COLUMNS, ln.split("\t"))) for ln in lines[1:]]
    assert sum(int(r["accepted"]) for r in rows) == report["accepted"]["total"]
    for row, rec in zip(rows, out["variants"]):
        c = genome.names.index(row["contig"])
        assert int(genome.starts[c]) + int(row["pos"]) - 1 == rec["g"] and row["type"] == rec["type"] and abs(float(row["llr"]) - rec["llr"]) < 1e-6
        assert (row["ref"] == "-") == (rec["type"] == "INS") and (row["alt"] == "-") == (rec["type"] == "DEL")
        if rec["type"] != "INS":
            assert row["ref"] == dict(draft)[row["contig"]][int(row["pos"]) - 1]
    assert [c["polished_length"] for c in report["contigs"]] == [int(n) for n in again.lengths] and report["genome"] == "draft.fa"


def test_read_strands_follow_read_sam(tmp_path):
    """reads_from_sam on a mapped.sam: the strand, the soft clips and the signal orientation, without changing pileup.read_sam."""
    genome = cmap.Genome([("c", "ACGTACGTACGTAAACCCGGGTTT")])
    sam = tmp_path / "mapped.sam"
    sam.write_text("@HD\tVN:1.6\n"
                   "fwd\t0\tc\t3\t255\t2S4=1I2=1S\t*\t0\t0\tTTGTACAGTA\t*\n"
                   "gone\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t*\n"
                   "rev\t16\tc\t13\t255\t3=1D2=3S\t*\t0\t0\tAAACCGGG\t*\n"
                   "second\t272\tc\t13\t255\t3=\t*\t0\t0\tAAA\t*\n")
    before = pileup.read_sam(str(sam), genome)
    source, reads = polish.reads_from_sam(str(sam), genome)
    assert source["names"] == before["names"] == ["fwd", "rev"] and sorted(source) == sorted(before) and source["skipped"] == before["skipped"]
    assert [(r["name"], r["pos"], r["reverse"], r["lead"]) for r in reads] == [("fwd", 2, False, 2), ("rev", 12, True, 0)]
    assert cmap.decode(reads[0]["called"]) == "TTGTACAGTA" and cmap.decode(reads[1]["called"]) == "CCCGGTTT"
    assert np.array_equal(reads[1]["ops"], source["alignments"][1][2]) and reads[0]["logits"] is None
