"""CPU: the seeding of the read mapper without a GPU.  The kernel's counting scheme, restated in tests/seed_ref.py, against the
definition chiron_amd.map.vote; the argument checks of chiron_seed_reads, which happen before a device is looked for; the
workspace formula and the batch plan of map.vote_reads."""
import ctypes as C
import os

import numpy as np
import pytest

import seed_ref


def test_lookup_and_rolling_kmers_equal_numpy():
    rng = np.random.default_rng(51)
    val = np.sort(rng.integers(0, 40, 300)).astype(np.int64)               # long runs, at both ends too
    for v in range(-1, 42):
        lo = int(np.searchsorted(val, v, side="left"))
        assert seed_ref.lookup(val, v) == (lo, int(np.searchsorted(val, v, side="right")) - lo), v
    assert seed_ref.lookup(np.zeros(0, np.int64), 3) == (0, 0)
    assert seed_ref.lookup(np.full(1000, 7, np.int64), 7) == (0, 1000) and seed_ref.lookup(np.array([7]), 7) == (0, 1)
    from chiron_amd import assess, map as cmap
    codes = rng.integers(0, 4, 500).astype(np.uint8)
    codes[[20, 21, 300, 499]] = 4
    fwd, rev, ok = seed_ref.kmer_values(codes)
    want_val, want_pos = cmap.kmers(codes)
    assert fwd[ok].tolist() == want_val.tolist() and np.nonzero(ok)[0].tolist() == want_pos.tolist()
    rc_val, rc_pos = cmap.kmers(assess.reverse_complement(codes))
    nk = len(fwd)
    assert rev[ok][::-1].tolist() == rc_val.tolist() and (nk - 1 - np.nonzero(ok)[0])[::-1].tolist() == rc_pos.tolist()
    for p0, p1 in ((0, nk), (0, 1), (7, 8), (100, 350), (nk - 1, nk), (nk, nk), (5, 5)):   # a thread's chunk, from any start
        got = seed_ref.roll(codes, p0, p1)
        assert [t[0] for t in got] == list(range(p0, p1))
        assert [t[1:] for t in got] == [(int(fwd[p]), int(rev[p]), bool(ok[p])) for p in range(p0, p1)]
    assert seed_ref.rank_find([0] * 511 + [3], 2) == (511, 2) and seed_ref.rank_find([2] + [0] * 511, 1) == (0, 1)
    assert seed_ref.rank_find([1, 2, 3] + [0] * 509, 3) == (2, 0) and seed_ref.rank_find([1] * 512, 512) == (-1, 0)


def test_scheme_equals_vote_on_random_cases():
    """About 1000 cases: genomes of 2 .. 20 kb with planted repeats and N's, reads of 0 .. 600 bases on both strands."""
    from chiron_amd import map as cmap
    rng = np.random.default_rng(52)
    seen = {"forward": 0, "reverse": 0, "none": 0, "second": 0}
    for k in range(1000):
        index, read = seed_ref.random_case(rng)
        want = cmap.vote(index, read)
        got = seed_ref.seed_all(index, [read, read])                         # twice through one workgroup: the counters were cleared
        assert got == [want, want], (k, want, got)
        seen[want["strand"] if want["votes"] else "none"] += 1
        seen["second"] += int(want["votes_second"] > 0)
    assert seen["forward"] > 200 and seen["reverse"] > 200 and seen["none"] > 100 and seen["second"] > 50, seen


def test_scheme_equals_vote_on_the_hand_cases():
    from chiron_amd import map as cmap
    cases, extra = seed_ref.hand_cases()
    want = {name: [cmap.vote(index, r) for r in reads] for name, (index, reads) in cases.items()}
    for name, (index, reads) in cases.items():
        assert seed_ref.seed_all(index, reads) == want[name], name
        assert seed_ref.seed_all(index, reads[::-1]) == want[name][::-1], name
    # the cases are what they claim to be
    assert all(v["votes"] == 0 and v["delta"] is None for v in want["degenerate_reads"][:3] + want["degenerate_reads"][5:7])
    assert [v["votes"] for v in want["degenerate_reads"][3:5]] == [1, 2]
    assert want["degenerate_reads"][7]["votes"] == 300 - 14 - 15 and want["degenerate_reads"][8]["votes"] == 286
    assert want["degenerate_reads"][9]["strand"] == "reverse"
    assert all(v["votes"] == 0 for v in want["empty_index"]) and len(cases["empty_index"][0][0]) == 0
    assert [v["votes"] for v in want["nothing_matches"]] == [0, 0, 286]
    t, e = want["ties"], extra["ties"]
    assert (t[0]["strand"], t[0]["delta"], t[0]["votes_second"]) == ("forward", e["two_copies_delta"], t[0]["votes"] == 286 and 286)
    assert (t[1]["strand"], t[1]["delta"]) == ("reverse", e["reverse_delta"])
    assert t[2]["delta"] == e["overhang_start_delta"] == -300 and t[3]["delta"] == e["overhang_end_delta"]
    pal = want["palindrome"][0]
    assert pal["strand"] == "forward" and pal["votes_second"] == pal["votes"] == 286
    b = want["bin_boundaries"]
    assert [b[k]["delta"] for k in (0, 2, 4)] == [256 * 20 - 1, 256 * 20, 256 * 20 + 1]
    assert b[6]["votes"] == 2 * 286 and b[6]["delta"] == extra["bin_boundaries"]["deletion"][0]     # the lower median: the first half's last hit
    assert b[8]["votes"] == 2 * 186 and b[8]["delta"] == extra["bin_boundaries"]["tie_delta"]       # bins (40, 41) and (41, 42) tie
    assert [v["votes_second"] for v in want["second_copy_near"]] == [0, 0]
    assert [v["votes_second"] for v in want["second_copy_far"]] == [286, 286]
    assert want["repeats_occ64"][0]["votes"] > 1000 and want["repeats_occ8"][0]["votes"] == 0
    assert min(want["repeats_occ64"][k]["votes"] for k in (8, 9, 10, 11)) >= 36                      # poly-A, poly-T: 6 k-mers, each at 6 places or more
    two = extra["two_contigs"]
    for v, contig in zip(want["two_contigs"], two["contigs"]):
        assert (v["votes"] == 0) if contig is None else (two["genome"].contig_of(v["g"]) == contig)


def test_counters_stay_clean_over_many_reads_and_a_stale_one_would_show():
    from chiron_amd import map as cmap
    index, reads = seed_ref.hygiene_case(400)
    want = [cmap.vote(index, r) for r in reads]
    assert seed_ref.seed_all(index, reads) == want
    # the same workgroup without its clearing pass, on a read and its repeat: the stale counters double the repeat's votes
    assert np.array_equal(reads[2], reads[1]) and want[1]["votes"] > 0
    wg = seed_ref.Workgroup(index, 400)
    assert wg.seed(reads[1], clear=False) == want[1]
    try:
        stale = wg.seed(reads[2])
    except AssertionError as e:
        assert "stale" in str(e)
    else:
        assert stale["votes"] == 2 * want[2]["votes"]


def test_scheme_equals_vote_at_long_reads_and_a_stale_counter_would_show():
    """Reads of 4 k to 131072 bases: a thread's chunk of phase 1 far above 8 positions, phase 4's counters beyond the first eight
    and, for tail_hit, beyond number 255, where rank_find passes thread 127's pair."""
    from chiron_amd import _lib, map as cmap
    index, reads = seed_ref.long_read_cases()
    assert sorted({len(r) for r in reads.values()}) == [4095, 4096, 4097, 65535, 65536, 65537, 73000, _lib.INFIX_MAX_READ]
    assert 390000 < len(index[0]) <= 400000
    names, codes = list(reads), list(reads.values())
    want = [cmap.vote(index, r) for r in codes]
    by = dict(zip(names, want))
    assert seed_ref.seed_all(index, codes) == want
    for name in names:                                                       # the cases are what they claim to be
        v, n = by[name], len(reads[name])
        assert v["strand"] == ("reverse" if name.endswith("_rc") else "forward") or name.startswith("unrelated"), name
        if name.startswith("cut"):
            assert v["votes"] > n // 4 and v["votes_second"] < 10, (name, v)
        elif name.startswith("unrelated"):
            assert v["votes"] < 10, (name, v)
        else:
            assert v["votes"] == 3000 - cmap.K + 1 and v["votes_second"] < 10, (name, v)
    tail, head = by["tail_hit"], by["head_hit"]
    assert tail["g"] - tail["delta"] >= 65536 and (tail["g"] - tail["delta"]) // seed_ref.BIN >= 273      # the read position of the candidate
    assert (head["g"] - head["delta"]) // seed_ref.BIN < 8
    assert max(by[n]["g"] - by[n]["delta"] for n in names if n.startswith("cut")) // seed_ref.BIN >= 8
    # one workgroup without its clearing pass: the second strand of a read meets the first one's counters
    wg = seed_ref.Workgroup(index, max(len(r) for r in codes))
    wrong = 0
    for r, v in zip(codes, want):
        try:
            wrong += wg.seed(r, clear=False) != v
        except AssertionError as e:
            assert "stale" in str(e)
            wrong += 1
    assert wrong >= 1


def test_the_mixed_batch_is_a_long_read_among_short_ones_that_hit():
    from chiron_amd import _lib, map as cmap
    index, long, short = seed_ref.mixed_batch()
    assert len(long) == _lib.INFIX_MAX_READ and len(short) == 300 and max(len(r) for r in short) <= 450
    want = [cmap.vote(index, r) for r in [long] + short]
    assert seed_ref.seed_all(index, [long] + short) == want and seed_ref.seed_all(index, short + [long]) == want[1:] + want[:1]
    assert sum(v["votes"] > 20 for v in want[1:]) > 200 and sum(v["votes"] == 0 for v in want[1:]) > 10
    assert all(185000 - 400 <= v["delta"] <= 215000 for v in want[1:] if v["votes"] > 20)      # in the embedded 30 kb


def _call(lib, idx_val, idx_pos, genome_len, codes, read_off, reads=None, flags=0, ws=1, n_index=None, nulls=()):
    val, pos = np.asarray(idx_val, np.uint32), np.asarray(idx_pos, np.int32)
    off, codes = np.asarray(read_off, np.int64), np.asarray(codes, np.uint8)
    count = len(off) - 1 if reads is None else reads
    out = [np.zeros(max(count, 1), np.int32) for _ in range(3)] + [np.zeros(max(count, 1), np.int64) for _ in range(2)]
    ptr = {"val": val.ctypes.data, "pos": pos.ctypes.data, "codes": codes.ctypes.data, "off": off.ctypes.data}
    ptr.update({"out%d" % k: o.ctypes.data for k, o in enumerate(out)})
    for name in nulls:
        ptr[name] = None
    st = lib.chiron_seed_reads(0, ptr["val"], ptr["pos"], len(val) if n_index is None else n_index, genome_len, ptr["codes"], ptr["off"], count,
                               flags, *[ptr["out%d" % k] for k in range(5)], C.c_void_p(ws), None)
    return st, lib.chiron_last_error(), out


def test_abi_sizes_and_argument_errors(built):
    from chiron_amd import _lib, map as cmap
    lib = _lib.load()
    n = C.c_size_t()
    base = (1000, 50000, 10, 400, 3000)
    size = cmap.seed_workspace_size(*base)
    assert size >= 8 * 1000 + 3000 + 10 * 36 + 10 * (16 * 400 + 8 * (50000 // 256))
    for k in range(5):                                                     # grows with every argument
        more = list(base)
        more[k] *= 4
        assert cmap.seed_workspace_size(*more) > size, k
    assert cmap.seed_workspace_size(1000, 50000, 3000, 400, 3000 * 300) - cmap.seed_workspace_size(1000, 50000, 2048, 400, 2048 * 300) < 1 << 20
    assert lib.chiron_seed_workspace_size(0, 0, 0, 0, 0, C.byref(n)) == _lib.OK
    assert lib.chiron_seed_workspace_size(1, _lib.SEED_MAX_GENOME, 1, _lib.INFIX_MAX_READ, 1, C.byref(n)) == _lib.OK
    for args, word in (((1, 10, 1, _lib.INFIX_MAX_READ + 1, 1), b"bases"), ((1, _lib.SEED_MAX_GENOME + 1, 1, 10, 1), b"genome"),
                       ((1, 10, (1 << 24) + 1, 10, 1), b"reads"), ((1 << 31, 10, 1, 10, 1), b"index")):
        assert lib.chiron_seed_workspace_size(*args, C.byref(n)) == _lib.ERR_OVERFLOW and word in lib.chiron_last_error(), args
    for k in range(5):
        args = [1, 100, 1, 10, 10]
        args[k] = -1
        assert lib.chiron_seed_workspace_size(*args, C.byref(n)) == _lib.ERR_INVALID and b"negative" in lib.chiron_last_error()
    assert lib.chiron_seed_workspace_size(1, 1, 1, 1, 1, None) == _lib.ERR_INVALID
    with pytest.raises(_lib.ChironError) as ei:
        cmap.seed_workspace_size(1, _lib.SEED_MAX_GENOME + 1, 1, 1, 1)
    assert ei.value.status == _lib.ERR_OVERFLOW
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "chiron_amd.h")).read()
    for name, value in (("K", "15"), ("BIN", "256"), ("THREADS", "256"), ("MAX_GROUPS", "2048"), ("MAX_GENOME", "0x7FFC0000")):
        assert "#define CHIRON_SEED_%s %s" % (name, value) in header and getattr(_lib, "SEED_" + name) == eval(value)
    assert (cmap.K, cmap.BIN) == (_lib.SEED_K, _lib.SEED_BIN)

    val, pos, codes, off = [5, 9, 9], [0, 40, 7], np.zeros(40, np.uint8), [0, 20, 40]
    ok = lambda **kw: _call(lib, kw.pop("val", val), kw.pop("pos", pos), kw.pop("genome_len", 100), kw.pop("codes", codes), kw.pop("off", off), **kw)
    st, msg, _ = ok(ws=0)
    assert st == _lib.ERR_INVALID and b"workspace" in msg                  # everything else passed: the last check before the device
    assert ok(reads=0)[0] == _lib.OK
    st, msg, _ = ok(off=[0, _lib.INFIX_MAX_READ + 1])
    assert st == _lib.ERR_OVERFLOW and b"bases" in msg                      # from the offsets alone, before a code is read
    st, msg, _ = ok(genome_len=_lib.SEED_MAX_GENOME + 1)
    assert st == _lib.ERR_OVERFLOW and b"genome" in msg
    st, msg, _ = ok(val=[5, 9, 8])
    assert st == _lib.ERR_INVALID and b"not sorted" in msg
    for bad in ([0, 86, 7], [0, -1, 7]):                                   # genome_len - 15 = 85 is the last k-mer position
        st, msg, _ = ok(pos=bad)
        assert st == _lib.ERR_INVALID and b"outside" in msg
    assert ok(pos=[0, 85, 7], ws=0)[1].find(b"workspace") >= 0
    st, msg, _ = ok(reads=-1)
    assert st == _lib.ERR_INVALID and b"reads" in msg
    for kw in (dict(n_index=-1), dict(genome_len=-1)):
        st, msg, _ = ok(**kw)
        assert st == _lib.ERR_INVALID and b"negative" in msg
    for name in ("val", "pos", "codes", "off", "out0", "out1", "out2", "out3", "out4"):
        st, msg, _ = ok(nulls=(name,))
        assert st == _lib.ERR_INVALID and b"null" in msg, name
    st, msg, _ = ok(flags=1)
    assert st == _lib.ERR_INVALID and b"flags" in msg
    st, msg, _ = ok(off=[0, 20, 10])
    assert st == _lib.ERR_INVALID and b"predecessor" in msg
    assert ok(off=[-1, 20, 40])[0] == _lib.ERR_INVALID
    st, msg, _ = ok(codes=np.full(40, 5, np.uint8))
    assert st == _lib.ERR_INVALID and b"outside 0..4" in msg
    st, _, out = ok(val=[], pos=[], ws=0)                                   # an empty index: votes 0 for every read, no device
    assert st == _lib.OK and all(not o.any() for o in out)


def test_vote_reads_plans_its_batches_within_the_budget(built):
    from chiron_amd import map as cmap
    lens = [300, 10, 5000, 5000, 0, 700, 20000, 20, 20, 20, 20, 300]
    n_index, genome_len = 40000, 41000
    one = max(cmap.seed_workspace_size(n_index, genome_len, 1, n, n) for n in lens)
    for budget in (one, one + (1 << 19), 3 * one, 1 << 40):
        batches = cmap.plan_seed_batches(lens, n_index, genome_len, budget)
        assert [i for b in batches for i in b] == list(range(len(lens)))   # consecutive, each read once
        for b in batches:
            need = cmap.seed_workspace_size(n_index, genome_len, len(b), max(lens[i] for i in b), sum(lens[i] for i in b))
            assert need <= budget, (budget, b)
        for b, nxt in zip(batches, batches[1:]):                           # as few calls as the budget allows: the next read did not fit
            grown = b + nxt[:1]
            assert cmap.seed_workspace_size(n_index, genome_len, len(grown), max(lens[i] for i in grown), sum(lens[i] for i in grown)) > budget
    assert len(cmap.plan_seed_batches(lens, n_index, genome_len, 1 << 40)) == 1
    assert cmap.plan_seed_batches(lens, n_index, genome_len, 1) == [[i] for i in range(len(lens))]    # a single read always forms a batch
    assert cmap.plan_seed_batches([], n_index, genome_len, 1) == []
    with pytest.raises(ValueError):
        cmap.seeder_of("cpu")
    assert cmap.seeder_of("host") is None and callable(cmap.seeder_of("gpu"))


def test_map_reads_takes_a_seeder_and_reports_the_seed(tmp_path):
    """map_reads(seeder=...) gives the seeder every read `seeds` does not cover, once, and maps as the per-read vote does."""
    import assess_ref
    import map_ref
    from chiron_amd import map as cmap
    rng = np.random.default_rng(53)
    contigs = [("c1", assess_ref.random_seq(4000, rng)), ("c2", assess_ref.random_seq(3000, rng))]
    g = cmap.Genome(contigs)
    reads = {"fwd": assess_ref.mutate(contigs[0][1][1000:1600], 0.05, rng), "rev": map_ref.revcomp(contigs[1][1][500:1200]),
             "junk": assess_ref.random_seq(500, rng), "given": contigs[0][1][2000:2300]}
    aligner = lambda rs, ws, band0: map_ref.infix_rows(rs, ws, band0, cmap.INFIX_DTYPE)
    seeds = {"given": {"strand": "forward", "delta": 2000, "contig": 0}}
    calls = []

    def seeder(index, codes):
        calls.append(len(codes))
        return seed_ref.seed_all(index, codes)

    want = cmap.map_reads(reads, g, aligner=aligner, seeds=seeds)
    got = cmap.map_reads(reads, g, aligner=aligner, seeds=seeds, seeder=seeder)
    assert got == want and calls == [3]
    assert [r["status"] for r in got["reads"]] == ["mapped", "mapped", "unmapped", "mapped"]


def test_a_library_without_a_bound_symbol_asks_for_a_rebuild(built, tmp_path):
    """The ABI version stays 7 while symbols are added: a library of that version from before them must give the "rebuild it"
    ImportError, not an AttributeError."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r)\nfrom chiron_amd import _lib\n"
            "_lib.SYMBOLS.append(('chiron_no_such_symbol', None, []))\n"
            "try:\n    _lib.load()\nexcept ImportError as e:\n    print('ImportError', e)\n" % root)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ImportError") and "chiron_no_such_symbol" in r.stdout and "rebuild it" in r.stdout, r.stdout + r.stderr
