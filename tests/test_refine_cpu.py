"""CPU: refinement without a GPU -- the three restatements of chiron_signal_refine's definition (tests/refine_ref.py) against each
other, the brute force included; the refusals of the two entry points and the calls that need no device; the host walk under a
sanitizer; the host rules of chiron_amd.squiggle (table, expected levels, items, planner); and the planted case with jittered
borders, refined by the reference alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import refine_cases as cases
import refine_ref as ref
import squiggle_cases
import squiggle_ref
from chiron_amd import _lib, squiggle
from test_weight_pack_cpu import rocm_prefix

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ----------------------------------------------------------------------------------------------------------------------------
# the references
# ----------------------------------------------------------------------------------------------------------------------------
def test_reference_against_brute_force():
    """Every strictly increasing assignment enumerated, at half-widths 1 .. 3: cost and borders equal, so the tie rule is checked
    too.  Both sample ranges, feasible and infeasible cases."""
    rng = np.random.default_rng(4000)
    feasible = infeasible = ties = 0
    seen = set()
    for k in range(700):
        x, e, a, half = cases.small_case(rng, infeasible=k % 4 == 3)
        want = ref.brute_item(x, e, a, half)
        assert ref.refine_item(x, e, a, half) == want, (k, want)
        assert ref.refine_item_numpy(x, e, a, half) == want, (k, want)
        seen.add((half, bool(np.abs(x).max(initial=0) > 100)))
        if want[1] == ref.INFEASIBLE:
            infeasible += 1
            assert want[0] == a.tolist()
        else:
            feasible += 1
            assert ref.cost_of(x, e, want[0]) == want[1]
            ties += int(want[1] == 0 and len(e) > 1)
    print("brute force: %d feasible, %d infeasible, %d with zero cost" % (feasible, infeasible, ties))
    assert feasible >= 300 and infeasible >= 30 and len(seen) == 6


def test_reference_formulations_at_the_library_width():
    """The plain-Python recurrence against the numpy rows at half-width 32, on the GPU tests' random items; the cost is the cost of
    the starts it comes with and is never above that of strictly increasing initial starts."""
    rng = np.random.default_rng(4001)
    signals, levels, starts = cases.random_items(rng, 60, max_bases=25)
    for spans in ([0, 0, 0, 0, 0, 2], [9] + [0] * 69 + [9]):                            # bases that crowd: no solution
        x, e, a = cases.item_of(rng, spans, 1, 1)
        signals, levels, starts = signals + [x], levels + [e], starts + [a]
    got, cost = ref.refine(signals, levels, starts)
    plain, plain_cost = ref.refine_plain(signals, levels, starts)
    assert np.array_equal(cost, plain_cost) and all(np.array_equal(a, b) for a, b in zip(got, plain))
    assert (cost == ref.INFEASIBLE).any() and (cost != ref.INFEASIBLE).sum() > 30
    for x, e, a, s, c in zip(signals, levels, starts, got, cost):
        if c == ref.INFEASIBLE:
            assert np.array_equal(s, a)
            continue
        assert ref.cost_of(x, e, s) == c and (np.diff(s) > 0).all() and s[0] == a[0] and s[-1] == a[-1]
        assert (np.abs(s - a)[1:-1] <= 32).all() and ((s - a)[1:-1] <= 31).all()
        if (np.diff(a) > 0).all():
            assert c <= ref.cost_of(x, e, a)
    assert ref.HALF == squiggle.REFINE_HALF == 32 and ref.INFEASIBLE == squiggle.INFEASIBLE == (1 << 63) - 1


# ----------------------------------------------------------------------------------------------------------------------------
# the entry points without a device
# ----------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_limits_are_bound(built):
    lib = _lib.load()
    names = {n for n, _, _ in _lib.SYMBOLS}
    assert {"chiron_signal_refine_workspace_size", "chiron_signal_refine"} <= names and hasattr(lib, "chiron_signal_refine")
    header = open(os.path.join(ROOT, "include", "chiron_amd.h")).read()
    INT64_MAX = (1 << 63) - 1  # noqa: F841  the header's word for INFEASIBLE
    for name in ("HALF", "INFEASIBLE", "THREADS", "MAX_GROUPS"):
        text = header.split("#define CHIRON_REFINE_%s " % name)[1].split("\n")[0].split("/*")[0].strip()
        assert eval(text) == getattr(_lib, "REFINE_" + name), name
    assert lib.chiron_abi_version() == 7


def test_workspace_size_rules(built):
    lib = _lib.load()
    up = lambda v: (v + 255) // 256 * 256
    assert squiggle.refine_workspace_size(3, 1000, 100) == 2 * up(32) + up(2000) + up(400) + 2 * up(412) + up(800) + up(24)
    assert squiggle.refine_workspace_size(0, 0, 0) == 0
    assert squiggle.refine_workspace_size(7, 0, 0) == 2 * up(64) + 2 * up(28) + up(56)
    n = C.c_size_t()
    for k in range(3):
        args = [1, 1, 1]
        args[k] = -1
        assert lib.chiron_signal_refine_workspace_size(*args, C.byref(n)) == _lib.ERR_INVALID and b"negative" in lib.chiron_last_error()
    assert lib.chiron_signal_refine_workspace_size(1, 1, 1, None) == _lib.ERR_INVALID and b"null bytes" in lib.chiron_last_error()
    for args, word in (((1 << 31, 1, 1), "items"), ((1, _lib.SIGNAL_MAX_SAMPLES + 1, 1), "samples"), ((1, 1, 1 << 31), "bases")):
        with pytest.raises(_lib.ChironError) as ei:
            squiggle.refine_workspace_size(*args)
        assert ei.value.status == _lib.ERR_OVERFLOW and word in str(ei.value), args
    assert squiggle.refine_workspace_size((1 << 31) - 1, _lib.SIGNAL_MAX_SAMPLES, (1 << 31) - 1) > 1 << 35
    # monotone in every argument: what the planner's bisection rests on
    base = squiggle.refine_workspace_size(5, 5000, 500)
    assert all(squiggle.refine_workspace_size(5 + a, 5000 + 300 * b, 500 + 70 * c) > base for a, b, c in ((70, 0, 0), (0, 1, 0), (0, 0, 1)))


def _call(lib, samples=(1, 2, 3, 4, 5, 6), sample_off=(0, 4, 6), level=(10, -10, 0), start=(0, 2, 4, 1, 2), base_off=(0, 2, 3), items=2, flags=0,
          out=True, cost=True, ws=0):
    """Two items of 4 and 2 samples and 2 and 1 bases.  With ws = 0 a call that passes every check ends at the null workspace."""
    arr = lambda v, t: None if v is None else np.ascontiguousarray(np.asarray(v, dtype=t))
    a = [arr(samples, np.int16), arr(sample_off, np.int64), arr(level, np.int32), arr(start, np.int32), arr(base_off, np.int64)]
    o = np.full(8, 77, np.int32)                 # a refused call writes nothing, whatever it was promised
    c = np.full(8, 77, np.int64)
    p = [None if x is None else x.ctypes.data for x in a]
    st = lib.chiron_signal_refine(0, p[0], p[1], p[2], p[3], p[4], items, flags, o.ctypes.data if out else None, c.ctypes.data if cost else None, ws, None)
    return st, lib.chiron_last_error().decode(), o, c


def test_every_refusal_comes_before_a_device(built):
    lib = _lib.load()
    INVALID, OVERFLOW = _lib.ERR_INVALID, _lib.ERR_OVERFLOW
    st, msg, o, c = _call(lib)
    assert st == INVALID and "chiron_signal_refine: null workspace" in msg            # everything else passed: the last check before the device
    assert (o == 77).all() and (c == 77).all()
    for kw, status, text in (
            (dict(flags=2), INVALID, "unknown flags 0x2"),
            (dict(items=-1), INVALID, "negative size"),
            (dict(items=1 << 31), OVERFLOW, "items in one call"),
            (dict(sample_off=None), INVALID, "null sample_off / base_off / start_in"),
            (dict(base_off=None), INVALID, "null sample_off / base_off / start_in"),
            (dict(start=None), INVALID, "null sample_off / base_off / start_in"),
            (dict(out=False), INVALID, "null start_out / cost_out"),
            (dict(cost=False), INVALID, "null start_out / cost_out"),
            (dict(level=None), INVALID, "null level"),
            (dict(samples=None), INVALID, "null samples"),
            (dict(sample_off=(-1, 4, 6)), INVALID, "sample_off[0] = -1 is negative"),
            (dict(sample_off=(0, 4, 3)), INVALID, "sample_off[2] = 3 below its predecessor 4"),
            (dict(base_off=(-2, 2, 3)), INVALID, "base_off[0] = -2 is negative"),
            (dict(base_off=(0, 2, 1)), INVALID, "base_off[2] = 1 below its predecessor 2"),
            (dict(sample_off=(0, 4, 4 + _lib.SIGNAL_MAX_SAMPLES)), OVERFLOW, "samples in one call"),
            (dict(base_off=(0, 2, 2 + (1 << 31))), OVERFLOW, "bases in one call"),
            (dict(start=(0, 2, 5, 1, 2)), INVALID, "start entry 2 of item 0 = 5 outside 0..4"),
            (dict(start=(-1, 2, 4, 1, 2)), INVALID, "start entry 0 of item 0 = -1 outside 0..4"),
            (dict(start=(0, 2, 4, 3, 2)), INVALID, "start entry 0 of item 1 = 3 outside 0..2"),
            (dict(start=(0, 3, 2, 1, 2)), INVALID, "start entry 2 of item 0 = 2 below its predecessor"),
            (dict(start=(0, 2, 4, 2, 1)), INVALID, "start entry 1 of item 1 = 1 below its predecessor"),
            (dict(level=(10, 32768, 0)), INVALID, "level 32768 of base 1 of item 0 outside -32767..32767"),
            (dict(level=(10, -10, -32768)), INVALID, "level -32768 of base 0 of item 1 outside -32767..32767"),
            (dict(level=(squiggle.UNKNOWN, 0, 0)), INVALID, "level -2147483648 of base 0 of item 0 outside -32767..32767")):
        st, msg, o, c = _call(lib, **kw)
        assert st == status and text in msg and msg.startswith("chiron_signal_refine: "), (kw, st, msg)
        assert (o == 77).all() and (c == 77).all(), kw
    # what is legal: the extreme levels, equal starts, samples nobody owns; each ends at the workspace check
    for kw in (dict(level=(32767, -32767, 0)), dict(start=(4, 4, 4, 0, 0)), dict(start=(1, 1, 3, 2, 2))):
        st, msg, _, _ = _call(lib, **kw)
        assert st == INVALID and "null workspace" in msg, (kw, msg)
    with pytest.raises(ValueError):
        squiggle.refine_call([np.zeros(3, np.int16)], [np.zeros(2, np.int32)], [np.array([0, 1], np.int32)])


def test_calls_that_need_no_device(built):
    lib = _lib.load()
    st, _, o, c = _call(lib, items=0)
    assert st == _lib.OK and (o == 77).all() and (c == 77).all()                      # no item: nothing is written
    st, _, o, c = _call(lib, base_off=(5, 5, 5), start=(9, 9, 9, 9, 9, 3, 1), level=None)
    assert st == _lib.OK and o.tolist() == [3, 1] + [77] * 6 and c.tolist() == [0, 0] + [77] * 6
    got, cost = squiggle.refine_call([], [], [])
    assert got == [] and cost.shape == (0,) and cost.dtype == np.int64
    got, cost = squiggle.refine_call([np.arange(5), np.zeros(0)], [np.zeros(0)] * 2, [[3], [0]])
    assert [g.tolist() for g in got] == [[3], [0]] and got[0].dtype == np.int32 and cost.tolist() == [0, 0]
    want, want_cost = ref.refine([np.arange(5), np.zeros(0)], [np.zeros(0)] * 2, [[3], [0]])
    assert [w.tolist() for w in want] == [[3], [0]] and want_cost.tolist() == [0, 0]


def test_host_walk_under_sanitizers(tmp_path):
    """tests/native/refine_pack_check.cpp, built with the ROCm host compiler under AddressSanitizer + UndefinedBehaviorSanitizer:
    csrc/refine_pack.h on items of 0, 1, 63, 64, 65, 257 and random numbers of bases in buffers of exactly the stated size, each
    kind of fault at the last place it can sit."""
    exe = str(tmp_path / "refine_pack_check")
    cmd = [os.path.join(rocm_prefix(), "llvm", "bin", "clang++"), "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", os.path.join(HERE, "native", "refine_pack_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "refine pack OK" in r.stdout


# ----------------------------------------------------------------------------------------------------------------------------
# the host side
# ----------------------------------------------------------------------------------------------------------------------------
def test_level_table_reader(tmp_path):
    planes = np.zeros((4, 64), dtype=np.int64)
    planes[:, 6] = [9, 80, 9 * 300 + 4, 9 * 300 * 300 + 5000]                          # ACG: 9 events around 300.44
    planes[:, 27] = [4, 30, -4 * 700, 4 * 700 * 700]                                   # CGT: 4 events at -700
    planes[:, 63] = [5, 30, 5 * 32767, 5 * 32767 * 32767]                              # TTT: at the largest level
    path = tmp_path / "kmer_levels.tsv"
    path.write_text("".join(squiggle.kmer_lines(planes, 3)))
    k, table = squiggle.load_level_table(str(path), 5)
    assert k == 3 and table.dtype == np.int32 and table.shape == (64,)
    want = np.full(64, squiggle.UNKNOWN, np.int32)
    want[6], want[63] = 300, 32767                                                     # rint(rint(300.44 / 256, 5 decimals) * 256)
    assert np.array_equal(table, want)
    assert squiggle.load_level_table(str(path), 4)[1][27] == -700 and squiggle.load_level_table(str(path), 10)[1][6] == squiggle.UNKNOWN
    assert np.array_equal(squiggle.table_of(planes, 5), want) and squiggle.table_of(planes, 4)[27] == -700
    assert squiggle.UNKNOWN == squiggle.EMPTY and abs(int(squiggle.UNKNOWN)) > 32767
    for text in ("", "kmer\tevents\n", "\t".join(squiggle.KMER_COLUMNS) + "\n", "\t".join(squiggle.KMER_COLUMNS) + "\nACG\t9\t1\t1\t1\nAC\t9\t1\t1\t1\n",
                 "\t".join(squiggle.KMER_COLUMNS) + "\nACN\t9\t1\t1\t1\n"):
        path.write_text(text)
        with pytest.raises(ValueError):
            squiggle.load_level_table(str(path))


def test_expected_levels_against_the_walk():
    rng = np.random.default_rng(4002)
    codes = rng.integers(0, 4, 120).astype(np.uint8)
    codes[[17, 60, 61]] = 4
    genome = squiggle_cases.PlainGenome(codes)
    kinds = set()
    for k in range(1, 7):
        table = rng.integers(-3000, 3000, 4 ** k).astype(np.int32)
        table[rng.random(4 ** k) < 0.2] = squiggle.UNKNOWN
        for j in range(25):
            read = squiggle_cases.random_read(rng, 120, reverse=bool(j % 2), pos=0 if j < 2 else None)
            if j % 5 == 0:
                read["called"][int(rng.integers(0, len(read["called"])))] = 4          # a called N
            got = squiggle.expected_levels(read, genome, table, k)
            want = ref.expected_levels(read, codes, table, k, squiggle.UNKNOWN)
            assert got.dtype == np.int32 and np.array_equal(got, want), (k, j)
            on = np.zeros(len(got), bool)
            on[[idx for _, idx in squiggle_ref.walk_columns(read)]] = True
            kinds |= {(bool(o), bool(v != squiggle.UNKNOWN)) for o, v in zip(on, got)}
            runs = squiggle.refine_items(got)
            known = got != squiggle.UNKNOWN
            assert sum(b - a for a, b in runs) == known.sum() and all(known[a:b].all() for a, b in runs)
            assert all(a == 0 or not known[a - 1] for a, _ in runs) and all(b == len(got) or not known[b] for _, b in runs)
    assert kinds == {(True, True), (True, False), (False, True), (False, False)}
    # a forward read over ACGTA.. with an inserted base: the column bases take the genome's 3-mers, the inserted one the read's own
    g = squiggle_cases.PlainGenome(np.array([0, 1, 2, 3, 0], np.uint8))
    table = np.arange(64, dtype=np.int32)
    read = {"pos": 0, "ops": np.array([0, 0, 2, 0, 0, 0], np.uint8), "reverse": False, "lead": 0, "called": np.array([0, 1, 3, 2, 3, 0], np.uint8)}
    assert squiggle.expected_levels(read, g, table, 3).tolist() == [squiggle.UNKNOWN, 6, 1 * 16 + 3 * 4 + 2, 27, 44, squiggle.UNKNOWN]
    with pytest.raises(ValueError):
        squiggle.expected_levels(read, g, table, 2)
    assert squiggle.refine_items([]) == [] and squiggle.refine_items([squiggle.UNKNOWN]) == [] and squiggle.refine_items([5, 5]) == [(0, 2)]
    assert squiggle.refine_items([1, squiggle.UNKNOWN, 2, 3, squiggle.UNKNOWN, squiggle.UNKNOWN, 4]) == [(0, 1), (2, 4), (6, 7)]


def _reads_for_refine(rng, count, genome_len):
    reads = []
    for k in range(count):
        r = squiggle_cases.random_read(rng, genome_len, name="r%d" % k, columns=int(rng.integers(30, 120)))
        r["starts"] = (int(rng.integers(0, 30)) + np.concatenate([[0], np.cumsum(rng.integers(0, 25, len(r["called"])))])).astype(np.int32)
        r["signal"] = rng.integers(-3000, 3000, int(r["starts"][-1]) + 5).astype(np.int16)
        reads.append(r)
    return reads


def test_refine_keeps_what_is_outside_the_items_and_plans_its_calls(built):
    rng = np.random.default_rng(4003)
    genome = squiggle_cases.PlainGenome(rng.integers(0, 4, 400))
    table = rng.integers(-3000, 3000, 64).astype(np.int32)
    table[rng.random(64) < 0.15] = squiggle.UNKNOWN
    reads = _reads_for_refine(rng, 30, 400)
    before = [r["starts"].copy() for r in reads]
    calls = []

    def refiner(signals, levels, starts):
        calls.append((len(signals), sum(len(s) for s in signals), sum(len(e) for e in levels)))
        assert all(len(s) == a[-1] and a[0] == 0 and len(a) == len(e) + 1 for s, e, a in zip(signals, levels, starts))
        return ref.refine(signals, levels, starts)
    one = [dict(r) for r in reads]
    got = squiggle.refine(one, genome, table, 3, refiner=refiner)
    assert got["calls"] == len(calls) == 1 and got["items"] == calls[0][0] > 30 and got["bases"] == calls[0][2]
    assert set(got) == set(squiggle.REFINE_COUNTS) | {"calls"} and 0 < got["infeasible"] < got["items"] and got["moved"] > 0.5 * got["borders"] > 500
    assert 0 < got["mean_move"] <= 32 and got["cost"] > 0
    total = moved = 0
    for r, new, old in zip(reads, one, before):
        lv = squiggle.expected_levels(r, genome, table, 3)
        inside = np.zeros(len(old), bool)
        for a, b in squiggle.refine_items(lv):
            inside[a + 1:b] = True
            x, e, s = new["signal"][old[a]:old[b]], lv[a:b], new["starts"][a:b + 1] - old[a]
            want, cost = ref.refine_item_numpy(x, e, old[a:b + 1] - old[a])
            assert s.tolist() == want
            total += 0 if cost == ref.INFEASIBLE else cost
        assert new["starts"].dtype == np.int32 and np.array_equal(new["starts"][~inside], old[~inside])      # borders outside the items, and the items' ends
        assert np.array_equal(r["starts"], old)                                                              # the caller's reads are dicts of their own
        moved += int((new["starts"] != old).sum())
    assert total == got["cost"] and moved == got["moved"]
    # the same reads in planned calls: a budget that holds a handful of reads
    counts = [calls[0]]
    budget = squiggle.refine_workspace_size(30, 3000, 250)
    del calls[:]
    many = [dict(r) for r in reads]
    again = squiggle.refine(many, genome, table, 3, workspace_mb=budget / (1 << 20), refiner=refiner)
    assert again["calls"] == len(calls) >= 4 and all(squiggle.refine_workspace_size(*c) <= budget for c in calls)
    assert dict(again, calls=1) == got and all(np.array_equal(a["starts"], b["starts"]) for a, b in zip(one, many))
    assert tuple(np.sum(calls, axis=0).tolist()) == counts[0]
    runs = squiggle.plan_refine_batches([(5, 700, 90)] * 10, squiggle.refine_workspace_size(15, 2100, 270))
    assert runs == [(0, 3), (3, 6), (6, 9), (9, 10)]
    assert squiggle.plan_refine_batches([(5, 700, 90)] * 3, 1) == [(0, 1), (1, 2), (2, 3)]               # a read that alone exceeds the budget
    # no read, and reads without a known level
    assert squiggle.refine([], genome, table, 3, refiner=refiner)["items"] == 0
    none = squiggle.refine([dict(r) for r in reads], genome, np.full(64, squiggle.UNKNOWN, np.int32), 3, refiner=refiner)
    assert none["items"] == none["borders"] == 0 and none["mean_move"] == 0.0


def test_sample_defaults_and_the_command_line():
    import inspect
    from chiron_amd import entry
    names = list(inspect.signature(squiggle.sample).parameters)
    assert names[-2:] == ["refine", "refiner"] and names[-3] == "kmer"
    assert all(inspect.signature(squiggle.sample).parameters[n].default is None for n in names[-2:])
    base = ["squiggle", "-i", "m", "-s", "c", "-g", "g.fa", "-o", "out"]
    args = entry.build_parser().parse_args(base)
    assert args.refine is None and args.refine_min_events == 5
    args = entry.build_parser().parse_args(base + ["--refine", "kmer_levels.tsv", "--refine-min-events", "8", "--kmer", "5"])
    assert args.refine == "kmer_levels.tsv" and args.refine_min_events == 8 and args.kmer == 5


# ----------------------------------------------------------------------------------------------------------------------------
# the planted case with jittered borders, on the reference alone
# ----------------------------------------------------------------------------------------------------------------------------
def _exact_share(reads, truth):
    hit = total = off = 0
    for r, t in zip(reads, truth):
        s, want = np.asarray(r["starts"][:-1], dtype=np.int64), np.asarray(t["true_starts"], dtype=np.int64)
        hit, total, off = hit + int((s == want).sum()), total + len(want), off + int(np.abs(s - want).sum())
    return hit / total, off / total


def _median_sd(planes):
    n, _, var = squiggle.moments(planes.transpose(1, 0, 2))
    return float(np.median(np.sqrt(var[n >= 5])))


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_planted_borders_are_found_again(seed):
    """squiggle_cases.planted(seed) with every border jittered by up to 6 samples; the table is the control's at its true borders,
    at least 5 events a k-mer; the DP is the numpy reference.  In both samples at least half of the borders land exactly on the
    planted ones, and the control's median per-position level sd is at most half the jittered run's.
    Measured with the reference, seeds 1 .. 5: exact share 0.10 to 0.12 jittered and 0.66 to 0.75 refined; mean |error| 2.7 samples
    jittered and 1.0 to 1.6 refined; the control's median sd 108 to 125 jittered and 31.4 to 35.5 refined, 33.8 to 38.9 at the true
    borders.  Nothing is asserted of `compare` at the planted modification: a canonical table pulls the borders wrong there
    (DESIGN 20)."""
    case = cases.planted(seed)
    genome = case["genome"]
    run = lambda reads, **kw: squiggle.sample(reads, genome, squiggle_cases.SEGMENT_LEN, squiggle_cases.RATIO, reducer=squiggle_ref.reduce_numpy,
                                              frame_aligner=squiggle_cases.frame_aligner_of(reads), **kw)
    control = run(case["b"], kmer=5)
    table = squiggle.table_of(control["kmer_planes"], 5)
    assert (table != squiggle.UNKNOWN).sum() > 300
    sd = {}
    for s in "ab":
        rough, fine = run(case[s + "_jit"]), run(case[s + "_jit"], refine=(table, 5), refiner=ref.refine)
        assert "refine" not in rough["report"] and fine["report"]["refine"]["bases"] > 5000
        (share0, off0), (share1, off1) = _exact_share(rough["reads"], case[s]), _exact_share(fine["reads"], case[s])
        sd[s] = (_median_sd(rough["planes"]), _median_sd(fine["planes"]))
        print("planted seed %d sample %s: exact borders %.3f -> %.3f, mean |error| %.2f -> %.2f samples, median level sd %.1f -> %.1f (true borders %.1f); %s"
              % (seed, s, share0, share1, off0, off1, sd[s][0], sd[s][1], _median_sd(control["planes"]) if s == "b" else float("nan"),
                 fine["report"]["refine"]))
        assert share0 < 0.2 and share1 >= 0.5
        assert fine["report"]["events"] >= rough["report"]["events"]                       # every base of a feasible item has a sample
    assert sd["b"][1] <= 0.5 * sd["b"][0]
