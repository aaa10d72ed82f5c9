"""CPU: squiggle without a GPU -- the plain-Python restatement of chiron_signal_levels (tests/squiggle_ref.py) against its numpy
formulation, the rounding rule, the host rules of chiron_amd.squiggle (bins, normalisation, starts, tiles, statistics), the refusals
of the two entry points, all decided before a device is needed, and the planted sample-compare case on the reference alone."""
import ctypes as C
import os

import numpy as np
import pytest

import squiggle_cases as cases
import squiggle_ref as ref
from chiron_amd import _lib, squiggle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------------------------------------------------------
# the references
# ----------------------------------------------------------------------------------------------------------------------------
def test_reference_against_its_second_formulation():
    rng = np.random.default_rng(1900)
    bases = events = 0
    for k in range(200):
        signals, starts, bins, n_bins = cases.random_set(rng)
        planes, levels = ref.reduce(signals, starts, bins, n_bins)
        planes2, levels2 = ref.reduce_numpy(signals, starts, bins, n_bins)
        assert planes.shape == planes2.shape == (4, n_bins) and np.array_equal(planes, planes2), k
        assert len(levels) == len(levels2) and all(np.array_equal(a, b) for a, b in zip(levels, levels2)), k
        bases += sum(len(b) for b in bins)
        events += int(planes[0].sum())
    assert bases > 5000 and events > 2000


def test_rounding_rule():
    """The mean to nearest, halves up, by floor division: at negative sums, exact halves, one sample, and the lowest sample value."""
    want = {(-1, -2): -1, (1, 2): 2, (-1,): -1, (-3, -4): -3, (3, 4): 4, (-32768,): -32768, (-32768, -32768, -32768): -32768,
            (-32768, -32767): -32767, (32767, 32767): 32767, (0, -1): 0, (0, 1): 1, (-5, -5, -6): -5, (-5, -6, -6): -6, (1, 1, 2): 1, (7,): 7}
    for samples, level in want.items():
        assert ref.level_of(samples) == level, samples
        sig = [np.array(samples, dtype=np.int16)]
        for fn in (ref.reduce, ref.reduce_numpy):
            planes, levels = fn(sig, [np.array([0, len(samples)], np.int32)], [np.array([0], np.int32)], 1)
            assert levels[0].tolist() == [level] and planes[:, 0].tolist() == [1, len(samples), level, level * level], (fn.__name__, samples)
    # C's truncating division would give 0 for [-1, -2] ... and an empty span is EMPTY and adds nothing
    planes, levels = ref.reduce_numpy([np.array([5], np.int16)], [np.array([0, 0, 1, 1], np.int32)], [np.array([0, 0, 0], np.int32)], 1)
    assert levels[0].tolist() == [ref.EMPTY, 5, ref.EMPTY] and planes[:, 0].tolist() == [1, 1, 5, 25]
    assert ref.EMPTY == squiggle.EMPTY == -(1 << 31)


# ----------------------------------------------------------------------------------------------------------------------------
# bins
# ----------------------------------------------------------------------------------------------------------------------------
def test_genome_bins_against_the_column_walk():
    rng = np.random.default_rng(1901)
    seen = set()
    for k in range(300):
        read = cases.random_read(rng, 200, reverse=bool(k % 2), lead=0 if k % 3 == 0 else None)
        m = int((read["ops"] != 2).sum())
        tiles = [(0, 200), (read["pos"], read["pos"] + m), (read["pos"] + 1, read["pos"] + max(m - 1, 1)), (0, read["pos"]),
                 (read["pos"] + m, 200), (read["pos"] + m // 2, read["pos"] + m // 2 + 1)]
        for g0, g1 in tiles:
            if g1 < g0:
                continue
            got = squiggle.genome_bins(read, g0, g1)
            assert got.dtype == np.int32 and np.array_equal(got, ref.genome_bins(read, g0, g1)), (k, g0, g1)
            assert got.max(initial=-1) < 2 * (g1 - g0)
        seen |= set(read["ops"].tolist())
        whole = squiggle.genome_bins(read, 0, 200)
        assert int((whole >= 0).sum()) == int((read["ops"] <= 1).sum())               # every '=' and 'X' column, nothing else
        assert np.all((whole[whole >= 0] >= 200) == read["reverse"])
    assert seen == {0, 1, 2, 3}
    with pytest.raises(ValueError):
        squiggle.genome_bins(dict(cases.random_read(rng, 50), lead=1000), 0, 50)


def test_tiles_sum_to_the_single_tile():
    """The planes of `levels` do not depend on how the genome was cut: a budget that forces many tiles, with reads over their edges."""
    rng = np.random.default_rng(1902)
    genome = cases.PlainGenome(rng.integers(0, 4, 300))
    reads = []
    for k in range(25):
        r = cases.random_read(rng, 300, name="r%d" % k, columns=int(rng.integers(20, 90)))
        n = len(r["called"])
        spans = rng.integers(0, 12, n)
        r["starts"] = (3 + np.concatenate([[0], np.cumsum(spans)])).astype(np.int32)
        r["signal"] = rng.integers(-3000, 3000, int(r["starts"][-1]) + 2).astype(np.int16)
        reads.append(r)
    one = squiggle.levels(reads, genome, reducer=ref.reduce)
    assert one["tiles"] == 1 and one["planes"].shape == (2, 4, 300) and one["planes"][:, 0].sum() > 500
    cut = squiggle.levels(reads, genome, reducer=ref.reduce_numpy, max_tile=37)
    assert cut["tiles"] == 9 and np.array_equal(cut["planes"], one["planes"])
    budget = squiggle.workspace_size(8, 8 * 600, 8 * 90, 2 * 40)
    planned = squiggle.plan_tiles(reads, 300, budget)
    assert len(planned) > 3 and planned[0][0] == 0 and planned[-1][1] == 300
    assert all(a[1] == b[0] for a, b in zip(planned, planned[1:])) and all(t[3] <= budget or t[1] - t[0] == 1 for t in planned)
    assert sum(len(t[2]) for t in planned) > len(reads)                               # some read went to two tiles
    small = squiggle.levels(reads, genome, workspace_mb=budget / (1 << 20), reducer=ref.reduce_numpy)
    assert small["tiles"] == len(planned) and np.array_equal(small["planes"], one["planes"])
    for a, b, c in zip(one["levels"], cut["levels"], small["levels"]):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    # the forward plane against a direct count of the columns
    events = np.zeros((2, 300), np.int64)
    for r in reads:
        for g, idx in ref.walk_columns(r):
            events[int(r["reverse"]), g] += int(r["starts"][idx + 1] > r["starts"][idx])
    assert np.array_equal(events, one["planes"][:, 0])


def test_kmer_bins_against_the_column_walk():
    rng = np.random.default_rng(1903)
    codes = rng.integers(0, 4, 120).astype(np.uint8)
    codes[[17, 60, 61]] = 4
    genome = cases.PlainGenome(codes)
    for k in range(1, 11):
        for j in range(12):
            read = cases.random_read(rng, 120, reverse=bool(j % 2), pos=0 if j < 2 else None)
            got = squiggle.kmer_bins(read, genome, k)
            want = ref.kmer_bins(read, codes, k)
            assert got.dtype == np.int32 and np.array_equal(got, want), (k, j)
            assert got.max(initial=-1) < 4 ** k
    # a forward read over ACGTA..: the 3-mer around position 1 is ACG; the reverse read over it sees CGT there
    g = cases.PlainGenome(np.array([0, 1, 2, 3, 0], np.uint8))
    fwd = {"pos": 0, "ops": np.zeros(5, np.uint8), "reverse": False, "lead": 0, "called": np.zeros(5, np.uint8)}
    assert squiggle.kmer_bins(fwd, g, 3).tolist() == [-1, 0 * 16 + 1 * 4 + 2, 1 * 16 + 2 * 4 + 3, 2 * 16 + 3 * 4 + 0, -1]
    assert squiggle.kmer_bins(dict(fwd, reverse=True), g, 3).tolist() == [-1, 3 * 16 + 0 * 4 + 1, 0 * 16 + 1 * 4 + 2, 1 * 16 + 2 * 4 + 3, -1]
    for bad in (0, 11):
        with pytest.raises(ValueError):
            squiggle.kmer_bins(fwd, g, bad)


# ----------------------------------------------------------------------------------------------------------------------------
# samples and starts
# ----------------------------------------------------------------------------------------------------------------------------
def test_normalise_and_the_flat_signal_drop():
    rng = np.random.default_rng(1904)
    x = rng.normal(500, 40, 2001)
    got = squiggle.normalise(x)
    m = np.median(x)
    d = np.median(np.abs(x - m)) / 0.6744897501960817
    assert got.dtype == np.int16 and np.array_equal(got, np.clip(np.rint((x - m) / d * 256), -32767, 32767).astype(np.int16))
    assert abs(float(np.median(got))) <= 1 and 150 < np.median(np.abs(got.astype(np.float64))) < 190     # MAD * 0.6745 * 256 = 172.7
    x[7] = 1e9                                                                       # an outlier is clipped, not wrapped
    assert squiggle.normalise(x)[7] == 32767 and squiggle.normalise(-x)[7] == -32767
    assert squiggle.normalise(np.full(50, 3.0)) is None and squiggle.normalise(np.zeros(0)) is None
    assert squiggle.normalise(np.array([1, 1, 1, 1, 9.0])) is None                   # more than half of the samples equal: MAD 0
    assert squiggle.normalise([1.5, 2.5, -0.5, 40000, -40000], "none").tolist() == [2, 2, 0, 32767, -32767]    # rint: halves to even
    with pytest.raises(ValueError):
        squiggle.normalise(x, "mean")
    # the drop is counted by prepare, before any alignment is asked for
    flat = {"name": "flat", "called": np.zeros(4, np.uint8), "logits": np.zeros((8, 5), np.float32), "raw": np.full(8, 2.0), "seq_lens": [8]}
    kept, drops = squiggle.prepare([flat, dict(flat, logits=None), dict(flat, called=np.array([0, 4], np.uint8))], 400, 1.0,
                                   frame_aligner=lambda *a: {"start": [], "status": []})
    assert kept == [] and drops == dict({k: 0 for k in squiggle.READ_DROPS}, flat_signal=1, no_signal=1, outside_acgt=1)


def test_base_starts():
    # two windows of 400 samples and 80 + 60 frames at ratio 5: frame 79 of window 0 starts at 395, frame 0 of window 1 at 400
    got = squiggle.base_starts([0, 3, 3, 79, 80, 139], [80, 60], 400, 5.0, 690)
    assert got.dtype == np.int32 and got.tolist() == [0, 15, 15, 395, 400, 690, 690]      # capped at signal_len; empty spans are legal
    assert squiggle.base_starts([], [80], 400, 5.0, 400).tolist() == [400]
    with pytest.raises(ValueError):
        squiggle.base_starts([140], [80, 60], 400, 5.0, 690)


# ----------------------------------------------------------------------------------------------------------------------------
# statistics
# ----------------------------------------------------------------------------------------------------------------------------
def test_compare_against_explicit_lists():
    rng = np.random.default_rng(1905)
    n_bins = 40
    lists = {s: [[int(v) for v in rng.normal(rng.normal(0, 300), 80, int(rng.integers(0, 30))).round()] for _ in range(n_bins)] for s in "ab"}
    lists["a"][3], lists["b"][3] = [5, 5, 5, 5, 5], [5, 5, 5, 5, 5, 5]              # no spread, same mean: t = 0
    lists["a"][4], lists["b"][4] = [7, 7, 7, 7, 7], [5, 5, 5, 5, 5, 5]              # no spread, different means: t = +inf
    planes = {}
    for s in "ab":
        planes[s] = np.array([[len(x) for x in lists[s]], [9 * len(x) for x in lists[s]], [sum(x) for x in lists[s]],
                              [sum(v * v for v in x) for x in lists[s]]], dtype=np.int64)
    got = squiggle.compare(planes["a"], planes["b"], 5)
    kept = 0
    for b in range(n_bins):
        xa, xb = lists["a"][b], lists["b"][b]
        assert bool(got["keep"][b]) == (len(xa) >= 5 and len(xb) >= 5)
        if not got["keep"][b]:
            assert all(np.isnan(got[k][b]) for k in ("mean_a", "var_b", "t", "df", "effect"))
            continue
        if b == 3:
            assert got["t"][b] == 0 and got["effect"][b] == 0 and np.isnan(got["df"][b])
            continue
        if b == 4:
            assert got["t"][b] == np.inf and got["effect"][b] == 2 / 256
            continue
        kept += 1
        want = ref.welch(xa, xb, 256)
        mine = [got[k][b] for k in ("mean_a", "var_a", "mean_b", "var_b", "t", "df", "effect")]
        # float64 on sums below 2^40: the variance from the sums loses at most a few units in 1e-10 of it
        assert np.allclose(mine, want, rtol=1e-9, atol=1e-9), (b, mine, want)
        assert got["events_a"][b] == len(xa) and got["events_b"][b] == len(xb)
    assert kept > 15
    assert not squiggle.compare(planes["a"], planes["b"], 0)["keep"][[b for b in range(n_bins) if len(lists["a"][b]) < 2]].any()
    with pytest.raises(ValueError):
        squiggle.compare(planes["a"], planes["b"][:, :5])


# ----------------------------------------------------------------------------------------------------------------------------
# the entry points' refusals
# ----------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_limits_are_bound(built):
    lib = _lib.load()
    names = {n for n, _, _ in _lib.SYMBOLS}
    assert {"chiron_signal_workspace_size", "chiron_signal_levels"} <= names and hasattr(lib, "chiron_signal_levels")
    header = open(os.path.join(ROOT, "include", "chiron_amd.h")).read()
    INT32_MIN = -(1 << 31)  # noqa: F841  the header's word for EMPTY
    for name in ("PLANES", "EMPTY", "MAX_SAMPLES", "MAX_BINS", "THREADS", "MAX_GROUPS"):
        text = header.split("#define CHIRON_SIGNAL_%s " % name)[1].split("\n")[0].split("/*")[0].strip()
        assert eval(text) == getattr(_lib, "SIGNAL_" + name), name
    assert (squiggle.THREADS, squiggle.MAX_GROUPS, squiggle.SCALE) == (256, 2048, 256)


def test_workspace_size_rules(built):
    lib = _lib.load()
    up = lambda v: (v + 255) // 256 * 256
    assert squiggle.workspace_size(3, 1000, 100, 50) == up(1600) + up(2000) + up(400) + up(1600)
    assert squiggle.workspace_size(3, 1000, 100, 50, False) == up(1600) + up(2000) + up(1600)
    assert squiggle.workspace_size(0, 0, 0, 0) == 0 and squiggle.workspace_size(10 ** 9, 0, 0, 1) == 256     # reads take no room
    n = C.c_size_t()
    for k in range(4):
        args = [1, 1, 1, 1]
        args[k] = -1
        assert lib.chiron_signal_workspace_size(*args, 1, C.byref(n)) == _lib.ERR_INVALID and b"negative" in lib.chiron_last_error()
    assert lib.chiron_signal_workspace_size(1, 1, 1, 1, 1, None) == _lib.ERR_INVALID and b"null bytes" in lib.chiron_last_error()
    for args, word in (((1, _lib.SIGNAL_MAX_SAMPLES + 1, 1, 1), "samples"), ((1, 1, 1 << 31, 1), "bases"), ((1, 1, 1, _lib.SIGNAL_MAX_BINS + 1), "bins")):
        with pytest.raises(_lib.ChironError) as ei:
            squiggle.workspace_size(*args)
        assert ei.value.status == _lib.ERR_OVERFLOW and word in str(ei.value), args
    assert squiggle.workspace_size(1, _lib.SIGNAL_MAX_SAMPLES, (1 << 31) - 1, _lib.SIGNAL_MAX_BINS) > 1 << 35


def _call(lib, samples=(1, 2, 3, 4, 5, 6), sample_off=(0, 4, 6), start=(0, 2, 4, 1, 2), base_off=(0, 2, 3), bins=(0, -1, 1), reads=2, n_bins=2,
          flags=0, planes=True, levels=True, ws=0):
    """Two reads of 4 and 2 samples and 2 and 1 bases.  With ws = 0 a call that passes every check ends at the null workspace."""
    arr = lambda v, t: None if v is None else np.ascontiguousarray(np.asarray(v, dtype=t))
    a = [arr(samples, np.int16), arr(sample_off, np.int64), arr(start, np.int32), arr(base_off, np.int64), arr(bins, np.int32)]
    p = np.full((4, min(max(n_bins, 1), 8)), 77, np.int64)             # a refused call writes nothing, whatever it was promised
    lv = np.full(8, 77, np.int32)
    st = lib.chiron_signal_levels(0, *[None if x is None else x.ctypes.data for x in a], reads, n_bins, flags, p.ctypes.data if planes else None,
                                  lv.ctypes.data if levels else None, ws, None)
    return st, lib.chiron_last_error().decode(), p, lv


def test_every_refusal_comes_before_a_device(built):
    lib = _lib.load()
    INVALID, OVERFLOW = _lib.ERR_INVALID, _lib.ERR_OVERFLOW
    st, msg, p, lv = _call(lib)
    assert st == INVALID and "chiron_signal_levels: null workspace" in msg            # everything else passed: the last check before the device
    assert (p == 77).all() and (lv == 77).all()
    for kw, status, text in (
            (dict(flags=4), INVALID, "unknown flags 0x4"),
            (dict(reads=-1), INVALID, "negative size"),
            (dict(n_bins=-2), INVALID, "negative size"),
            (dict(n_bins=_lib.SIGNAL_MAX_BINS + 1, bins=(-1, -1, -1)), OVERFLOW, "bins in one call"),
            (dict(planes=False), INVALID, "null planes_out with 2 bins"),
            (dict(sample_off=None), INVALID, "null sample_off / base_off / start"),
            (dict(base_off=None), INVALID, "null sample_off / base_off / start"),
            (dict(start=None), INVALID, "null sample_off / base_off / start"),
            (dict(bins=None), INVALID, "null bin"),
            (dict(samples=None), INVALID, "null samples"),
            (dict(sample_off=(-1, 4, 6)), INVALID, "sample_off[0] = -1 is negative"),
            (dict(sample_off=(0, 4, 3)), INVALID, "sample_off[2] = 3 below its predecessor 4"),
            (dict(base_off=(-2, 2, 3)), INVALID, "base_off[0] = -2 is negative"),
            (dict(base_off=(0, 2, 1)), INVALID, "base_off[2] = 1 below its predecessor 2"),
            (dict(sample_off=(0, 4, 4 + _lib.SIGNAL_MAX_SAMPLES)), OVERFLOW, "samples in one call"),
            (dict(base_off=(0, 2, 2 + (1 << 31))), OVERFLOW, "bases in one call"),
            (dict(start=(0, 2, 5, 1, 2)), INVALID, "start entry 2 of read 0 = 5 outside 0..4"),
            (dict(start=(-1, 2, 4, 1, 2)), INVALID, "start entry 0 of read 0 = -1 outside 0..4"),
            (dict(start=(0, 2, 4, 3, 2)), INVALID, "start entry 0 of read 1 = 3 outside 0..2"),
            (dict(start=(0, 3, 2, 1, 2)), INVALID, "start entry 2 of read 0 = 2 below its predecessor"),
            (dict(start=(0, 2, 4, 2, 1)), INVALID, "start entry 1 of read 1 = 1 below its predecessor"),
            (dict(bins=(0, -2, 1)), INVALID, "bin -2 of base 1 of read 0 outside -1..1"),
            (dict(bins=(0, -1, 2)), INVALID, "bin 2 of base 0 of read 1 outside -1..1"),
            (dict(n_bins=0, planes=False), INVALID, "bin 0 of base 0 of read 0 outside -1..-1")):
        st, msg, p, lv = _call(lib, **kw)
        assert st == status and text in msg and msg.startswith("chiron_signal_levels: "), (kw, st, msg)
        assert (p == 77).all() and (lv == 77).all(), kw
    # what is legal: no planes without bins, no levels, equal starts, samples nobody owns; each ends at the workspace check
    for kw in (dict(n_bins=0, planes=False, bins=(-1, -1, -1)), dict(levels=False), dict(start=(4, 4, 4, 0, 0)), dict(start=(1, 1, 3, 2, 2))):
        st, msg, _, _ = _call(lib, **kw)
        assert st == INVALID and "null workspace" in msg, (kw, msg)
    # nothing to compute and nothing to clear: no device is touched, whatever the workspace
    assert _call(lib, reads=0, n_bins=0, planes=False)[0] == _lib.OK
    assert _call(lib, base_off=(0, 0, 0), start=(0, 1), bins=(), n_bins=0, planes=False)[0] == _lib.OK
    st, msg, _, _ = _call(lib, reads=0)                                               # planes to clear: a device is needed
    assert st == INVALID and "null workspace" in msg
    with pytest.raises(ValueError):
        squiggle.reduce_call([np.zeros(3, np.int16)], [np.array([0, 1], np.int32)], [np.array([0, 0], np.int32)], 1)


# ----------------------------------------------------------------------------------------------------------------------------
# the planted case, on the reference alone
# ----------------------------------------------------------------------------------------------------------------------------
def test_planted_modification_is_found(built):
    """cases.planted(): the five largest |t| of compare are exactly forward 298 .. 302.  No GPU: the forced alignment is the case's
    own and the reduction is the plain-Python reference."""
    case = cases.planted()
    got = {}
    for s in "ab":
        got[s] = squiggle.sample(case[s], case["genome"], cases.SEGMENT_LEN, cases.RATIO, frame_aligner=cases.frame_aligner_of(case[s]),
                                 reducer=ref.reduce, kmer=5 if s == "b" else 0)
        rd = got[s]["report"]["reads"]
        assert rd["total"] == rd["used"] == 30 and sum(rd["dropped"].values()) == 0
        assert got[s]["report"]["events"] == got[s]["report"]["bases"] == sum(len(r["called"]) for r in case[s])
    result = squiggle.compare(got["a"]["planes"].transpose(1, 0, 2), got["b"]["planes"].transpose(1, 0, 2), 5)
    t = np.where(result["keep"], np.abs(result["t"]), -1.0).reshape(-1)
    order = np.argsort(-t)
    print("planted: fifth |t| = %.2f, sixth = %.2f" % (t[order[4]], t[order[5]]))
    assert sorted(order[:5].tolist()) == [298, 299, 300, 301, 302]                       # strand 0 (forward) occupies 0 .. 599
    assert result["keep"].sum() > 400 and (result["effect"][0, 298:303] > 0.5).all()
    # the control's k-mer table follows the planted one: per read gain and offset are gone after normalisation
    km = got["b"]["kmer_planes"]
    seen = km[0] >= 8
    _, mean, _ = squiggle.moments(km)
    assert seen.sum() > 50 and np.corrcoef(mean[seen], case["table"][seen])[0, 1] > 0.98
    # the writers' columns
    lines = squiggle.level_lines(got["a"]["planes"], case["genome"])
    assert lines[0].rstrip("\n").split("\t") == list(squiggle.LEVEL_COLUMNS) and len(lines) == 1 + int((got["a"]["planes"][:, 0] > 0).sum())
    assert all(len(ln.split("\t")) == len(squiggle.LEVEL_COLUMNS) for ln in lines)
    lines = squiggle.compare_lines(result, case["genome"])
    assert lines[0].rstrip("\n").split("\t") == list(squiggle.COMPARE_COLUMNS) and len(lines) == 1 + int(result["keep"].sum())
    lines = squiggle.kmer_lines(km, 5)
    assert lines[0].rstrip("\n").split("\t") == list(squiggle.KMER_COLUMNS) and len(lines) == 1 + int((km[0] > 0).sum()) and len(lines[1].split("\t")[0]) == 5
    r = got["a"]["reads"][1]
    lines = squiggle.event_lines(r, got["a"]["levels"][1], case["genome"])
    assert lines[0].rstrip("\n").split("\t") == list(squiggle.EVENT_COLUMNS) and len(lines) == 1 + len(r["called"])
    first = lines[1].rstrip("\n").split("\t")
    assert first[3] == "ctg" and int(first[4]) == r["pos"] + len(r["called"]) and int(first[0]) == r["starts"][0]     # a reverse read starts at its last position
