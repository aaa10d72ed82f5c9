"""CPU: several seeding candidates a read, without a GPU.  map.vote_top (the definition) against map.vote; the kernel's scheme,
restated in tests/seed_top_ref.py, against vote_top; the refusals of chiron_seed_candidates, which come before a device is looked
for; the mapping quality, the duplicate rule and the file columns of map_reads(candidates > 1); the MAPQ floor of the SAM readers;
and the planted repeat through the reference pipeline.  Every comparison is ==."""
import ctypes as C
import json

import numpy as np
import pytest

import assess_ref
import map_ref
import seed_ref
import seed_top_ref


@pytest.fixture(scope="module")
def random_cases():
    rng = np.random.default_rng(61)
    return [seed_ref.random_case(rng) for _ in range(1000)]


def test_vote_top_starts_as_vote_does(random_cases):
    """Pick 0 is vote's candidate; pick 1's votes are vote's votes_second, and there is no pick 1 when that is 0."""
    from chiron_amd import map as cmap
    seen = {"none": 0, "one": 0, "more": 0, "reverse": 0}
    for k, (index, read) in enumerate(random_cases):
        want = cmap.vote(index, read)
        got = cmap.vote_top(index, read, 4)
        if want["votes"] == 0:
            assert got == [], k
            seen["none"] += 1
            continue
        assert got[0] == {key: want[key] for key in ("votes", "strand", "delta", "g")}, k
        assert list(got[0]) == ["votes", "strand", "delta", "g"]
        if want["votes_second"] == 0:
            assert len(got) == 1, k
        else:
            assert got[1]["votes"] == want["votes_second"], k
        assert [p["votes"] for p in got] == sorted((p["votes"] for p in got), reverse=True), k
        assert cmap.vote_top(index, read, 1) == got[:1] and cmap.vote_top(index, read, 8)[:len(got)] == got, k
        seen["one" if len(got) == 1 else "more"] += 1
        seen["reverse"] += got[0]["strand"] == "reverse"
    assert seen["none"] > 100 and seen["one"] > 100 and seen["more"] > 100 and seen["reverse"] > 200, seen


def test_scheme_equals_vote_top_on_random_cases(random_cases):
    from chiron_amd import map as cmap
    for k, (index, read) in enumerate(random_cases):
        max_cand, min_score = 1 + k % 8, (1, 1, 2, 5)[k % 4]
        want = cmap.vote_top(index, read, max_cand, min_score)
        got = seed_top_ref.seed_top_all(index, [read, read], max_cand, min_score)    # twice through one workgroup: cleared once, after the picks
        assert got == [want, want], (k, want, got)


def test_scheme_and_vote_top_on_the_hand_cases():
    from chiron_amd import map as cmap
    cases = seed_top_ref.hand_cases()
    want = {}
    for name, (index, reads, max_cand, min_score) in cases.items():
        want[name] = [cmap.vote_top(index, r, max_cand, min_score) for r in reads]
        assert seed_top_ref.seed_top_all(index, reads, max_cand, min_score) == want[name], name
        assert seed_top_ref.seed_top_all(index, reads[::-1], max_cand, min_score) == want[name][::-1], name
    # the cases are what they claim to be
    lead = 256 * 20
    for picks in want["copies_at_radius"]:                                   # 3 bins apart with n // 256 + 2 = 3: suppressed
        assert [p["votes"] for p in picks[:1]] == [286] and all(p["votes"] < 15 for p in picks[1:])
    fwd, rev = want["copies_past_radius"]                                    # one bin further: the second copy is pick 1
    assert [(p["votes"], p["strand"], p["delta"]) for p in fwd[:2]] == [(286, "forward", lead), (286, "forward", lead + 256 * 4)]
    assert [(p["votes"], p["strand"]) for p in rev[:2]] == [(286, "reverse"), (286, "reverse")] and rev[0]["delta"] == lead
    fwd, rev = want["reverse_copy"]
    assert [(p["votes"], p["strand"], p["delta"]) for p in fwd[:2]] == [(286, "forward", 5000), (286, "reverse", 5000 + 300 + 6000)]
    assert [(p["votes"], p["strand"], p["delta"]) for p in rev[:2]] == [(286, "forward", 11300), (286, "reverse", 5000)]
    deltas = [3000 + 2800 * c for c in range(5)]
    assert [(p["votes"], p["delta"]) for p in want["five_copies"][0]] == [(286, d) for d in deltas[:4]]      # equal scores: the smaller bin first
    assert [p["strand"] for p in want["five_copies"][1]] == ["reverse"] * 4
    assert [(p["votes"], p["delta"]) for p in want["five_copies_all"][0][:5]] == [(286, d) for d in deltas]
    assert all(p["votes"] < 15 for p in want["five_copies_all"][0][5:])
    pal = want["equal_scores"][0]                                            # forward before reverse, then the smaller bin
    assert [(p["votes"], p["strand"], p["delta"]) for p in pal] == [(286, "forward", 4000), (286, "forward", 9300), (286, "reverse", 4000),
                                                                     (286, "reverse", 9300)]
    assert [(p["votes"], p["delta"]) for p in want["min_score_cuts"][0]] == [(286, 4000)]
    assert [(p["votes"], p["delta"]) for p in want["min_score_one"][0][:2]] == [(286, 4000), (86, 10300)]
    short = want["short_reads"]
    assert short[:3] == [[], [], []] and short[5:] == [[], []]                # shorter than K, all N, unrelated
    assert [[(p["votes"], p["delta"]) for p in picks] for picks in short[3:5]] == [[(1, 1000)], [(2, 1000)]]    # exactly K bases, K + 1
    over = want["overhang"]
    assert over[0][0]["delta"] == -200 and over[1][0]["delta"] == 6000 - 300 and over[2][0]["strand"] == "reverse"


def test_a_stale_counter_would_show():
    """The workgroup without its clearing pass: the repeat of a read meets the read's own counters."""
    from chiron_amd import map as cmap
    index, reads = seed_top_ref.hygiene_reads(300)
    want = [cmap.vote_top(index, r, 4) for r in reads]
    assert seed_top_ref.seed_top_all(index, reads, 4) == want
    assert sum(len(p) > 1 for p in want) > 50 and sum(len(p) == 0 for p in want) >= 60
    k = next(k for k in range(2, len(reads), 3) if want[k])
    assert np.array_equal(reads[k], reads[k - 1])
    wg = seed_top_ref.TopWorkgroup(index, 200)
    assert wg.seed_top(reads[k - 1], 4, clear=False) == want[k - 1]
    try:
        stale = wg.seed_top(reads[k], 4)
    except AssertionError as e:
        assert "stale" in str(e)
    else:
        assert stale != want[k] and stale[0]["votes"] == 2 * want[k][0]["votes"]


def test_the_shared_gpu_cases_are_what_they_claim():
    from chiron_amd import _lib, map as cmap
    index, reads = seed_top_ref.random_reads()
    lens = [len(r) for r in reads]
    assert len(reads) == 300 and min(lens) >= 15 and max(lens) <= 600 and 19000 < len(index[0]) <= 20000
    want = [cmap.vote_top(index, r, 4) for r in reads]
    assert sum(len(p) >= 2 and p[1]["votes"] > 20 for p in want) > 40       # the planted repeats give real second candidates
    assert sum(p[0]["delta"] < 0 for p in want if p) > 20 and sum(p[0]["strand"] == "reverse" for p in want if p) > 80
    assert sum(len(p) == 0 for p in want) > 10
    index, reads = seed_top_ref.hygiene_reads()
    assert len(reads) == 2100 > _lib.SEED_MAX_GROUPS and max(len(r) for r in reads) <= 200
    assert all(np.array_equal(reads[k], reads[k - 1]) for k in range(2, 2100, 3))
    assert all(cmap.vote_top(index, reads[k], 1) == [] for k in range(4, 2100, 5) if k % 3 != 2)


# ------------------------------------------------------------------------------------------------------------------------------
# the entry point's refusals
# ------------------------------------------------------------------------------------------------------------------------------
def _call(lib, idx_val, idx_pos, genome_len, codes, read_off, reads=None, max_cand=4, min_score=1, flags=0, ws=1, n_index=None, nulls=()):
    val, pos = np.asarray(idx_val, np.uint32), np.asarray(idx_pos, np.int32)
    off, codes = np.asarray(read_off, np.int64), np.asarray(codes, np.uint8)
    count = len(off) - 1 if reads is None else reads
    width = max(count, 1) * seed_top_ref.MAX_CANDIDATES
    out = [np.full(max(count, 1), -7, np.int32)] + [np.full(width, -7, t) for t in (np.int32, np.int32, np.int64, np.int64)]
    ptr = {"val": val.ctypes.data, "pos": pos.ctypes.data, "codes": codes.ctypes.data, "off": off.ctypes.data}
    ptr.update({"out%d" % k: o.ctypes.data for k, o in enumerate(out)})
    for name in nulls:
        ptr[name] = None
    st = lib.chiron_seed_candidates(0, ptr["val"], ptr["pos"], len(val) if n_index is None else n_index, genome_len, ptr["codes"], ptr["off"],
                                    count, max_cand, min_score, flags, *[ptr["out%d" % k] for k in range(5)], C.c_void_p(ws), None)
    return st, lib.chiron_last_error().decode(), out


def test_sizes_and_refusal_texts(built):
    from chiron_amd import _lib, map as cmap
    lib = _lib.load()
    n = C.c_size_t()
    base = (1000, 50000, 10, 400, 3000)
    up256 = lambda v: -(-v // 256) * 256
    for max_cand in range(1, 9):                                             # the seeding workspace with the larger result block
        assert cmap.seed_candidates_workspace_size(*base, max_cand) - cmap.seed_workspace_size(*base) == up256(10 * (4 + 16 * max_cand)) - up256(10 * 20)
    assert _lib.SEED_MAX_CANDIDATES == seed_top_ref.MAX_CANDIDATES == 8
    who = "chiron_seed_candidates_workspace_size"
    for max_cand in (0, 9, -1):
        assert lib.chiron_seed_candidates_workspace_size(*base, max_cand, C.byref(n)) == _lib.ERR_INVALID
        assert lib.chiron_last_error().decode() == "%s: max_cand %d outside 1 .. 8" % (who, max_cand)
    assert lib.chiron_seed_candidates_workspace_size(*base, 4, None) == _lib.ERR_INVALID
    assert lib.chiron_last_error().decode() == who + ": null bytes"
    assert lib.chiron_seed_candidates_workspace_size(1, 10, 1, _lib.INFIX_MAX_READ + 1, 1, 4, C.byref(n)) == _lib.ERR_OVERFLOW
    assert lib.chiron_last_error().decode() == "%s: a read of %d bases, the kernel takes at most %d" % (who, _lib.INFIX_MAX_READ + 1, _lib.INFIX_MAX_READ)
    assert lib.chiron_seed_candidates_workspace_size(1, _lib.SEED_MAX_GENOME + 1, 1, 10, 1, 4, C.byref(n)) == _lib.ERR_OVERFLOW
    assert "a genome of %d bases" % (_lib.SEED_MAX_GENOME + 1) in lib.chiron_last_error().decode()
    assert lib.chiron_seed_candidates_workspace_size(-1, 10, 1, 10, 1, 4, C.byref(n)) == _lib.ERR_INVALID
    assert lib.chiron_last_error().decode() == who + ": negative n_index / genome_len / reads / max_read / total_bases"

    who = "chiron_seed_candidates"
    val, pos, codes, off = [5, 9, 9], [0, 40, 7], np.zeros(40, np.uint8), [0, 20, 40]
    ok = lambda **kw: _call(lib, kw.pop("val", val), kw.pop("pos", pos), kw.pop("genome_len", 100), kw.pop("codes", codes), kw.pop("off", off), **kw)
    st, msg, out = ok(ws=0)                                                  # everything else passed: the last check before the device
    assert st == _lib.ERR_INVALID and "workspace" in msg and msg.startswith(who + ": ")
    assert all((o == -7).all() for o in out)                                 # a refusal writes nothing
    for max_cand in (0, 9):
        assert ok(max_cand=max_cand)[:2] == (_lib.ERR_INVALID, "%s: max_cand %d outside 1 .. 8" % (who, max_cand))
    for min_score in (0, -3):
        assert ok(min_score=min_score)[:2] == (_lib.ERR_INVALID, "%s: min_score %d below 1" % (who, min_score))
    assert ok(max_cand=0, reads=0)[0] == _lib.ERR_INVALID and ok(reads=0)[0] == _lib.OK
    assert ok(reads=-1)[:2] == (_lib.ERR_INVALID, who + ": reads -1")
    assert ok(n_index=-1)[:2] == (_lib.ERR_INVALID, who + ": negative n_index -1 or genome_len 100")
    assert ok(flags=2)[:2] == (_lib.ERR_INVALID, who + ": unknown flags 0x2")
    for name in ("val", "pos", "codes", "off", "out0", "out1", "out2", "out3", "out4"):
        st, msg, _ = ok(nulls=(name,))
        assert (st, msg) == (_lib.ERR_INVALID, who + (": null codes" if name == "codes" else ": null operand")), name
    st, msg, _ = ok(off=[0, _lib.INFIX_MAX_READ + 1])
    assert st == _lib.ERR_OVERFLOW and msg.startswith(who) and "bases" in msg
    st, msg, _ = ok(genome_len=_lib.SEED_MAX_GENOME + 1)
    assert (st, msg) == (_lib.ERR_OVERFLOW, "%s: a genome of %d bases, at most %d keep every diagonal in 32 bits"
                         % (who, _lib.SEED_MAX_GENOME + 1, _lib.SEED_MAX_GENOME))
    assert ok(val=[5, 9, 8])[:2] == (_lib.ERR_INVALID, who + ": the index is not sorted: idx_val[2] = 8 below its predecessor 9")
    assert ok(pos=[0, 86, 7])[:2] == (_lib.ERR_INVALID, who + ": idx_pos[1] = 86 outside the k-mer positions 0 .. 85 of the genome")
    assert ok(codes=np.full(40, 5, np.uint8))[:2] == (_lib.ERR_INVALID, who + ": code 5 at 0 of read 0 outside 0..4")
    st, msg, _ = ok(off=[0, 20, 10])
    assert st == _lib.ERR_INVALID and "predecessor" in msg
    st, _, out = ok(val=[], pos=[], ws=0, max_cand=3)                        # an empty index: no pick for any read, no device
    assert st == _lib.OK and not out[0][:2].any() and all(not o[:6].any() and (o[6:] == -7).all() for o in out[1:])
    # the batch plan of vote_reads_top uses the new size function
    lens = [300, 10, 5000, 5000, 0, 700, 20000, 20, 20, 20, 20, 300]
    one = max(cmap.seed_candidates_workspace_size(40000, 41000, 1, v, v, 8) for v in lens)
    batches = cmap.plan_seed_batches(lens, 40000, 41000, one + (1 << 19), max_cand=8)
    assert [i for b in batches for i in b] == list(range(len(lens))) and len(batches) > 1
    for b in batches:
        assert cmap.seed_candidates_workspace_size(40000, 41000, len(b), max(lens[i] for i in b), sum(lens[i] for i in b), 8) <= one + (1 << 19)
    assert callable(cmap.top_seeder_of("gpu")) and cmap.top_seeder_of("host") is None
    with pytest.raises(ValueError):
        cmap.top_seeder_of("cpu")


# ------------------------------------------------------------------------------------------------------------------------------
# map_reads with several candidates
# ------------------------------------------------------------------------------------------------------------------------------
def test_mapq_formula_and_duplicate_rule():
    from chiron_amd import map as cmap
    assert cmap.mapq_of([]) == 0 and cmap.mapq_of([37]) == 60 and cmap.mapq_of([0]) == 60
    assert cmap.mapq_of([50, 50]) == 0 and cmap.mapq_of([0, 0]) == 0                         # max(E2, 1) keeps the tie at 0 defined
    assert cmap.mapq_of([50, 54]) == 600 * 4 // 54 == 44 and cmap.mapq_of([54, 50, 90]) == 44   # the two smallest, in any order
    assert cmap.mapq_of([50, 55]) == 54 and cmap.mapq_of([50, 56]) == 60 and cmap.mapq_of([0, 1]) == 60 and cmap.mapq_of([99, 100]) == 6
    picks = [{"votes": v} for v in (100, 60, 50, 49, 3)]
    assert [r for r, _ in cmap.candidates_of(picks, 4, 0.5)] == [0, 1, 2] and [r for r, _ in cmap.candidates_of(picks, 4, 0.0)] == [0, 1, 2, 3]
    assert [r for r, _ in cmap.candidates_of(picks, 55, 0.1)] == [0, 1] and [r for r, _ in cmap.candidates_of(picks[:1], 4, 1.0)] == [0]
    assert [r for r, _ in cmap.candidates_of([{"votes": 99}, {"votes": 50}, {"votes": 49}], 4, 0.5)] == [0, 1]    # ceil(49.5) = 50
    assert cmap.candidates_of([], 4, 0.5) == []

    def cand(rank, start, end, edit, match=500, contig="c", strand="forward", status="mapped"):
        return {"rank": rank, "contig": contig, "strand": strand, "start": start, "end": end, "edit": edit, "match": match, "status": status}

    a, b, c = cand(0, 1000, 1600, 60), cand(1, 1599, 2200, 40), cand(2, 5000, 5600, 57)
    assert cmap.choose([a, b, c]) == (c, 600 * 3 // 60, 60)                 # b overlaps a by one base: a duplicate, though it is the best
    assert cmap.choose([a, cand(1, 1600, 2200, 40), c])[0]["rank"] == 1      # touching is not overlapping
    assert cmap.choose([a, cand(1, 1000, 1600, 40, strand="reverse")])[0]["rank"] == 1       # another strand is another place
    assert cmap.choose([a, cand(1, 1000, 1600, 40, contig="d")])[0]["rank"] == 1
    assert cmap.choose([a, cand(1, 3000, 3600, 60, match=501), cand(2, 7000, 7600, 60, match=501)]) == (cand(1, 3000, 3600, 60, match=501), 0, 60)
    assert cmap.choose([cand(0, 1000, 1600, 60, status="edge"), c]) == (c, 60, None)          # one mapped candidate
    assert cmap.choose([cand(0, 1000, 1600, 60, status="edge")]) == (None, 0, None)
    assert cmap.choose([cand(0, 1000, 1600, 60, status="edge"), cand(1, 1200, 1800, 10)]) == (None, 0, None)   # the edge one holds the place


@pytest.fixture(scope="module")
def two_copies():
    """A genome with a 400-base segment twice, the second copy with a substitution every 50 bases.  `first` is cut from the first
    copy.  `second` is cut from the second copy and differs from it at both neighbours of each of those six positions it covers:
    no k-mer of it holds one, so the two copies get the same votes and the vote alone takes the first copy (the smaller bin), 18
    edits away instead of 12.  Then reads from unique sequence (forward and reverse), an unrelated one and one shorter than K."""
    from chiron_amd import map as cmap
    rng = np.random.default_rng(62)
    rs = assess_ref.random_seq
    seg = rs(400, rng)
    other = list(seg)
    for at in range(20, 400, 50):
        other[at] = "ACGT"["ACGT".index(other[at]) ^ 1]
    other = "".join(other)
    g = rs(3000, rng) + seg + rs(4000, rng) + other + rs(3000, rng)
    genome = cmap.Genome([("chr", g)])
    second = list(other[40:360])
    for at in range(70, 360, 50):
        for k in (at - 1 - 40, at + 1 - 40):
            second[k] = "ACGT"["ACGT".index(second[k]) ^ 2]
    reads = {"first": seg[40:360], "second": "".join(second), "unique": g[1000:1400], "unique_rc": map_ref.revcomp(g[8500:8900]),
             "noise": rs(300, rng), "tiny": g[100:110]}
    aligner = lambda rs_, ws, band0: map_ref.infix_rows(rs_, ws, band0, cmap.INFIX_DTYPE)
    return genome, reads, aligner


def decode_at(genome, lo, hi):
    return "".join("ACGTN"[c] for c in genome.codes[lo:hi])


def test_map_reads_with_candidates_records_and_files(two_copies, tmp_path):
    from chiron_amd import map as cmap
    genome, reads, aligner = two_copies
    one = cmap.map_reads(reads, genome, aligner=aligner)
    assert cmap.map_reads(reads, genome, aligner=aligner, candidates=1, second_ratio=0.9) == one          # today's path, today's records
    assert all("mapq" not in r for r in one["reads"]) and "ambiguity" not in one
    got = cmap.map_reads(reads, genome, aligner=aligner, candidates=4)
    by = {r["name"]: r for r in got["reads"]}
    base = {r["name"]: r for r in one["reads"]}
    for name in ("unique", "unique_rc", "noise", "tiny"):                    # one place or none: the single-candidate record plus four fields
        extra = {"mapq": 60, "candidates": 1, "edit_second": None, "seed_rank": 0} if base[name]["status"] == "mapped" else \
                {"mapq": 0, "candidates": 0, "edit_second": None, "seed_rank": None}
        assert by[name] == dict(base[name], **extra), name
    assert [base[n]["status"] for n in ("unique", "unique_rc", "noise", "tiny")] == ["mapped", "mapped", "unmapped", "unmapped"]
    f, s = by["first"], by["second"]
    assert (f["start"], f["end"], f["edit"], f["edit_second"], f["candidates"], f["seed_rank"]) == (3040, 3360, 0, 6, 2, 0)
    far = map_ref.full_table(reads["second"], decode_at(genome, 2800, 3600))[0]       # what the first copy costs, by the reference
    assert 12 < far <= 18 and map_ref.full_table(reads["second"], decode_at(genome, 7200, 8000))[0] == 12
    assert (s["start"], s["end"], s["edit"], s["edit_second"], s["candidates"], s["seed_rank"]) == (7440, 7760, 12, far, 2, 1)
    assert f["mapq"] == 60 and s["mapq"] == min(60, 600 * (far - 12) // far)
    assert s["votes"] == s["votes_second"] == 320 - 14 - 6 * 17
    assert (base["second"]["start"], base["second"]["edit"]) == (3040, far)   # the vote alone puts it on the first copy
    assert got["references"]["second"] == decode_at(genome, 7440, 7760) and got["references"]["unique_rc"] == reads["unique_rc"]
    assert sorted(got["references"]) == ["first", "second", "unique", "unique_rc"]
    assert got["ambiguity"] == {"mapq0": 2, "mapq1_59": 0, "mapq60": 4, "won_by_later_pick": 1}
    assert got["totals"]["mapped"] == 4 and got["totals"]["edit"] == 12 and got["unmapped"] == ["noise", "tiny"]
    # second_ratio 1.0 keeps the tied second copy; a min_votes above every score maps nothing
    tight = {r["name"]: r for r in cmap.map_reads(reads, genome, aligner=aligner, candidates=2, second_ratio=1.0)["reads"]}
    assert tight["second"] == s and (f["votes"], f["votes_second"]) == (306, 306 - 6 * 15)
    assert tight["first"] == dict(f, candidates=1, edit_second=None)        # 216 votes of 306: not aligned, and mapq 60 says less
    none = cmap.map_reads(reads, genome, aligner=aligner, candidates=4, min_votes=1000)
    assert none["totals"]["mapped"] == 0 and all(r["mapq"] == 0 and r["candidates"] == 0 for r in none["reads"])
    assert [r["votes"] for r in none["reads"]] == [r["votes"] for r in one["reads"]]                         # the record is today's
    for bad in (dict(candidates=0), dict(candidates=9), dict(candidates=2, second_ratio=1.5)):
        with pytest.raises(ValueError):
            cmap.map_reads(reads, genome, aligner=aligner, **bad)
    # a top_seeder gets every read once, with the arguments of vote_top
    calls = []

    def top_seeder(index, codes, max_cand, min_score):
        calls.append((len(codes), max_cand, min_score))
        return seed_top_ref.seed_top_all(index, codes, max_cand, min_score)

    assert cmap.map_reads(reads, genome, aligner=aligner, candidates=4, top_seeder=top_seeder,
                          seeder=lambda index, codes: seed_ref.seed_all(index, codes)) == got
    assert calls == [(6, 4, cmap.MIN_VOTES)]
    # the files
    tracer = lambda rs_, fs: [np.zeros(len(r), np.uint8) for r in rs_]
    traced = cmap.add_cigars(got, reads, genome, tracer=tracer)
    paf = [ln.split("\t") for ln in cmap.paf_lines(traced, genome)]
    assert [(c[0], c[11], c[12:]) for c in paf] == [("first", "60", ["e2:i:6", "cg:Z:320="]), ("second", str(s["mapq"]), ["e2:i:%d" % far, "cg:Z:320="]),
                                                     ("unique", "60", ["cg:Z:400="]), ("unique_rc", "60", ["cg:Z:400="])]
    sam = [ln.split("\t") for ln in cmap.sam_lines(traced, reads, genome) if not ln.startswith("@")]
    assert [(c[0], c[1], c[3], c[4], c[11:]) for c in sam] == [("first", "0", "3041", "60", ["NM:i:0", "e2:i:6"]),
                                                                ("second", "0", "7441", str(s["mapq"]), ["NM:i:12", "e2:i:%d" % far]),
                                                                ("unique", "0", "1001", "60", ["NM:i:0"]), ("unique_rc", "16", "8501", "60", ["NM:i:0"])]
    old = cmap.add_cigars(one, reads, genome, tracer=tracer)
    assert all(ln.split("\t")[11] == "255" and "e2:i" not in ln for ln in cmap.paf_lines(old, genome))
    assert all(ln.split("\t")[4] == "255" for ln in cmap.sam_lines(old, reads, genome) if not ln.startswith("@"))
    report = cmap.write_outputs(str(tmp_path / "out"), traced, genome, {"candidates": 4, "second_ratio": 0.5}, reads)
    on_disk = json.loads((tmp_path / "out" / "map_report.json").read_text())
    assert on_disk == json.loads(json.dumps(report))
    assert [on_disk[key] for key in ("candidates", "second_ratio", "mapq0", "mapq1_59", "mapq60", "won_by_later_pick")] == [4, 0.5, 2, 0, 4, 1]
    assert "mapq0" not in cmap.write_outputs(str(tmp_path / "old"), old, genome, {}, reads)


def test_two_exact_copies_tie_at_mapq_zero(two_copies):
    """Two exact copies: mapq 0, and the first pick keeps the read."""
    from chiron_amd import map as cmap
    genome, reads, aligner = two_copies
    rng = np.random.default_rng(63)
    seg = assess_ref.random_seq(500, rng)
    g = assess_ref.random_seq(2000, rng) + seg + assess_ref.random_seq(3000, rng) + seg + assess_ref.random_seq(2000, rng)
    got = cmap.map_reads({"tie": seg[50:450]}, cmap.Genome([("chr", g)]), aligner=aligner, candidates=4)["reads"][0]
    assert (got["mapq"], got["edit"], got["edit_second"], got["seed_rank"], got["start"], got["candidates"]) == (0, 0, 0, 0, 2050, 2)


def test_sam_readers_drop_and_count_records_below_min_mapq(tmp_path):
    from chiron_amd import map as cmap, pileup, polish
    rng = np.random.default_rng(64)
    g = assess_ref.random_seq(2000, rng)
    genome = cmap.Genome([("chr", g)])
    rows = [("r%d" % k, 16 if k % 2 else 0, 100 + 150 * k, mapq) for k, mapq in enumerate((0, 1, 29, 30, 31, 60, 255))]
    rows.append(("sec", 0x100, 1500, 60))
    path = tmp_path / "m.sam"
    path.write_text("@HD\tVN:1.6\n@SQ\tSN:chr\tLN:2000\n" + "".join(
        "\t".join(str(v) for v in (name, flag, "chr", pos, mapq, "100=", "*", 0, 0, g[pos - 1:pos + 99], "*", "NM:i:0")) + "\n"
        for name, flag, pos, mapq in rows))
    for floor, names in ((0, ["r0", "r1", "r2", "r3", "r4", "r5", "r6"]), (1, ["r1", "r2", "r3", "r4", "r5", "r6"]), (30, ["r3", "r4", "r5", "r6"]),
                         (31, ["r4", "r5", "r6"]), (61, ["r6"]), (255, ["r6"]), (1000, ["r6"])):                 # 255: not available, always passes
        src = pileup.read_sam(str(path), genome, min_mapq=floor)
        assert src["names"] == names and src["low_mapq"] == 7 - len(names) and src["used"] == len(names), floor
        assert src["skipped"]["secondary"] == 1 and sum(src["skipped"].values()) == 1
        source, reads = polish.reads_from_sam(str(path), genome, min_mapq=floor)
        assert [r["name"] for r in reads] == names and source["low_mapq"] == 7 - len(names)
        assert [s[0] for s in polish.read_strands(str(path), floor)] == names
        assert [r["reverse"] for r in reads] == [int(n[1:]) % 2 == 1 for n in names]
    assert pileup.read_sam(str(path), genome)["names"] == pileup.read_sam(str(path), genome, 0)["names"]
    assert polish.reads_from_sam(str(path), genome)[0]["low_mapq"] == 0
    from chiron_amd import entry
    parser = entry.build_parser()
    for cmd in (["pileup", "-i", "x", "-g", "g", "-o", "o"], ["polish", "-i", "x", "-s", "s", "-g", "g", "-o", "o"],
                ["squiggle", "-i", "x", "-s", "s", "-g", "g", "-o", "o"]):
        assert parser.parse_args(cmd).min_mapq == 0 and parser.parse_args(cmd + ["--min-mapq", "20"]).min_mapq == 20
    for cmd in (["map", "-i", "x", "-g", "g", "-o", "o"], ["assess", "-i", "x", "-g", "g", "-o", "o"], ["label", "-i", "x", "-g", "g", "-o", "o"]):
        args = parser.parse_args(cmd)
        assert (args.candidates, args.second_ratio) == (1, 0.5)
        args = parser.parse_args(cmd + ["--candidates", "4", "--second-ratio", "0.7"])
        assert (args.candidates, args.second_ratio) == (4, 0.7)


# ------------------------------------------------------------------------------------------------------------------------------
# the planted repeat
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_planted_repeat_needs_more_than_one_candidate():
    """A 3 kb segment copied 10 kb downstream at 1 % substitutions; 100 reads of 600 bases at 12 % errors cut from the second copy,
    20 controls cut from unique sequence; host seeding and the reference aligner.  Observed with seed_top_ref.REPEAT_SEED: 13 reads
    on the wrong copy at candidates=1, 0 at candidates=4, 13 reads won by a later pick."""
    from chiron_amd import map as cmap
    contigs, reads, truth = seed_top_ref.repeat_case()
    genome = cmap.Genome(contigs)
    aligner = lambda rs, ws, band0: map_ref.infix_rows(rs, ws, band0, cmap.INFIX_DTYPE)
    index = cmap.build_index(genome.codes)
    one = {r["name"]: r for r in cmap.map_reads(reads, genome, aligner=aligner, index=index)["reads"]}
    res = cmap.map_reads(reads, genome, aligner=aligner, index=index, candidates=4)
    four = {r["name"]: r for r in res["reads"]}
    rep = [n for n in sorted(reads) if n.startswith("rep")]
    ctl = [n for n in sorted(reads) if n.startswith("ctl")]
    assert len(rep) == 100 and len(ctl) == 20
    wrong1 = [n for n in rep if seed_top_ref.on_wrong_copy(one[n], truth[n])]
    wrong4 = [n for n in rep if seed_top_ref.on_wrong_copy(four[n], truth[n])]
    print("wrong copy at candidates=1: %d, at candidates=4: %d; %s" % (len(wrong1), len(wrong4), res["ambiguity"]))
    assert len(wrong1) >= 5                                                   # the case has power
    assert len(wrong4) <= 2 and all(four[n]["mapq"] == 0 for n in wrong4)
    assert all(four[n]["status"] == "mapped" and four[n]["candidates"] >= 2 for n in rep)
    for n in ctl:
        assert four[n]["mapq"] == 60 and one[n]["status"] == "mapped"
        assert all(four[n][key] == one[n][key] for key in ("contig", "strand", "start", "end", "edit", "match"))
    assert res["ambiguity"]["won_by_later_pick"] >= len(wrong1) - len(wrong4)
