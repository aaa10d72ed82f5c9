"""CPU: `locate --events` without a GPU -- the restatements of chiron_signal_events and chiron_event_locate (tests/event_ref.py)
against each other, the brute force included; the library's host-only detector against them; the truth on noise-free steps; the
refusals of the three entry points and the calls that need no device; the host code under a sanitizer; the host rules of
chiron_amd.locate under events=; and the planted case, located by the reference alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import event_ref as ref
import locate_cases as cases
import locate_ref
from chiron_amd import _lib, locate
from test_weight_pack_cpu import rocm_prefix

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
W, RADIUS, THR, PENALTY = 3, 2, 768, 150               # the defaults: window, radius, 256 x t^2 = 3, skip penalty


# ----------------------------------------------------------------------------------------------------------------------------
# the references
# ----------------------------------------------------------------------------------------------------------------------------
def test_dp_reference_against_brute_force():
    """Every path with moves of 0, 1 and 2 columns enumerated for Q <= 6 and R <= 8: cost and start per end column equal in all
    three forms, with breaks, at P = 0, 1, 150 and 65534, and with ties: equal levels, and P = 0 so that skip and move tie."""
    rng = np.random.default_rng(8000)
    with_break = tied = skipped = 0
    for k in range(800):
        Q, R = int(rng.integers(1, 7)), int(rng.integers(1, 9))
        P = (0, 1, 150, 65534)[k % 4]
        x = rng.integers(-6, 7, Q)
        e = rng.integers(-6, 7, R).astype(np.int64)
        e[rng.random(R) < (0.25 if k % 3 == 1 else 0.0)] = ref.BREAK
        if k % 5 == 0:                                   # a constant signal on a constant reference: the tie rule alone decides
            x[:] = 3
            e[e != ref.BREAK] = 3
        want = ref.columns_brute(x, e, P)
        assert ref.columns_plain(x, e, P) == want, (k, x, e, P)
        assert ref.columns_numpy(x, e, P) == want, (k, x, e, P)
        assert np.array_equal(ref.blocks_of(want), ref.blocks_numpy(x, e, P))
        assert np.array_equal(ref.blocks_of(want, 2), ref.blocks_numpy(x, e, P, 2))
        with_break += int((e == ref.BREAK).any())
        for j, (d, s) in enumerate(want):
            assert (d == ref.NONE) == (e[j] == ref.BREAK) and (d == ref.NONE or j - 2 * (Q - 1) <= s <= j)
        skipped += int(want != locate_ref.columns_brute(x, e))
        if k % 5 == 0 and not (e == ref.BREAK).any():
            tied += 1                                    # all paths cost 0 (P = 0) or the skip never pays: the smallest start there is
            step = 2 if P == 0 else 1
            assert want == [(0, max(j - step * (Q - 1), 0)) for j in range(R)], (k, P)
    assert with_break > 150 and tied > 80 and skipped > 80


def test_dp_reference_formulations_at_the_library_block():
    """The plain-Python recurrence against the numpy rows across a block edge, with breaks, and at the extreme values."""
    rng = np.random.default_rng(8001)
    for R, Q, breaks, wide, P in ((1030, 9, 0.0, False, 150), (1025, 40, 0.05, False, 0), (2049, 5, 0.3, True, 65534), (70, 300, 0.02, True, 1)):
        e, x = cases.random_reference(rng, R, breaks, wide), cases.random_query(rng, Q, wide)
        assert ref.columns_plain(x, e, P) == ref.columns_numpy(x, e, P)
        assert np.array_equal(ref.locate([x], e, P), ref.locate_plain([x], e, P))
    Q = 8192
    got = ref.locate([np.full(Q, -32768, np.int16)], np.array([32767, ref.BREAK], np.int32), 65534)
    assert got.tolist() == [[[Q * 65535, 0, 0]]] and Q * (65535 + 65534) < 1 << 30
    assert ref.locate([np.zeros(3, np.int16)], np.full(5, ref.BREAK, np.int32), 7).tolist() == [[[ref.NONE] * 3]]
    assert ref.locate([], np.zeros(1500, np.int32), 7).shape == (0, 2, 3) and ref.locate([np.zeros(2, np.int16)], np.zeros(0, np.int32), 7).shape == (1, 0, 3)
    # a skip never crosses a break: 5 -> 9 over the break costs nothing without it and is impossible with it
    e = np.array([5, ref.BREAK, 9], np.int32)
    assert ref.columns_numpy([5, 9], e, 1) == [(4, 0), (ref.NONE, ref.NONE), (4, 2)]
    assert ref.columns_numpy([5, 9], np.array([5, 0, 9], np.int32), 1) == [(4, 0), (9, 0), (1, 0)]


def test_skip_dp_equals_the_sample_dp_where_no_skip_can_pay():
    """P = 65534, levels and events within +-300 and Q <= 100: a path without a skip to any column costs at most 100 x 600 < P (stay
    there), so no cheapest path holds a skip and the result is chiron_signal_locate's, every column."""
    rng = np.random.default_rng(8002)
    for R, Q, breaks in ((40, 100, 0.0), (1030, 64, 0.1), (300, 7, 0.3), (2049, 33, 0.02)):
        e, x = cases.random_reference(rng, R, breaks), cases.random_query(rng, Q)
        assert Q * 600 < 65534
        assert ref.columns_numpy(x, e, 65534) == locate_ref.columns_numpy(x, e)
        assert np.array_equal(ref.locate([x], e, 65534), locate_ref.locate([x], e))
        assert not np.array_equal(ref.locate([x], e, 0), locate_ref.locate([x], e))      # and at P = 0 it is not


def _signals(rng):
    """Random step signals with noise, constant ones (V = 0 throughout), and ones shorter than two windows."""
    for k in range(240):
        w, r = int(rng.integers(2, 17)), int(rng.integers(1, 17))
        thr = int(rng.integers(1, 3000))
        if k % 6 == 0:
            x = np.full(int(rng.integers(1, 80)), int(rng.integers(-32768, 32768)), np.int16)
        elif k % 6 == 1:
            x = rng.integers(-500, 500, int(rng.integers(1, 2 * w))).astype(np.int16)
        else:
            n = int(rng.integers(2 * w, 400))
            steps = np.repeat(rng.integers(-700, 700, n), rng.integers(1, 15, n))[:n]
            x = (steps + rng.integers(-40, 41, n) * (k % 3)).astype(np.int16)
        yield k, x, w, r, thr, (int(rng.integers(1, 12)) if k % 4 == 0 else 1 << 17)


def test_the_detector_in_its_two_forms_and_the_library(built):
    """segment_plain, segment_numpy and chiron_signal_events (through locate.events_of) give the same levels, borders and truncation
    on random step signals, on constant signals, on signals shorter than two windows, and at the extreme sample values."""
    rng = np.random.default_rng(8003)
    one = several = cut = 0
    for k, x, w, r, thr, cap in _signals(rng):
        a, b = ref.segment_plain(x, w, r, thr, cap), ref.segment_numpy(x, w, r, thr, cap)
        c = locate.events_of(x, w, thr, r, cap)
        for other in (b, c):
            assert np.array_equal(a[0], other[0]) and np.array_equal(a[1], other[1]) and a[2] == other[2], (k, w, r, thr, cap)
            assert other[0].dtype == np.int16 and other[1].dtype == np.int32
        assert a[1][0] == 0 and (a[2] or a[1][-1] == len(x)) and len(a[0]) == len(a[1]) - 1 <= cap
        if len(x) < 2 * w or x.min() == x.max():
            assert len(a[0]) == 1 and not a[2]
        one += len(a[0]) == 1
        several += len(a[0]) > 3
        cut += a[2]
    assert one > 60 and several > 80 and cut > 20
    x = np.tile(np.repeat(np.array([32767, -32768], np.int16), 16), 8)                # the largest numerator there is, V = 0
    assert ref.statistic_plain(x, 16)[16] == 16 * (16 * 65535) ** 2 * 256 < 1 << 52
    a, c = ref.segment_plain(x, 16, 16, 1 << 52), locate.events_of(x, 16, 1 << 52, 16)
    assert len(a[0]) == 1 and len(c[0]) == 1
    a, b, c = ref.segment_plain(x, 16, 1, 1), ref.segment_numpy(x, 16, 1, 1), locate.events_of(x, 16, 1, 1)
    assert a[1].tolist() == b[1].tolist() == c[1].tolist() == list(range(0, 257, 16)) and a[0].tolist() == c[0].tolist() == [32767, -32768] * 8


def test_several_items_in_one_call(built):
    """chiron_signal_events on several items from a first offset above 0: where each item's borders and levels lie in the outputs,
    and that entries past an item's count are left as they were."""
    rng = np.random.default_rng(8004)
    xs = [x for _, x, _, _, _, _ in _signals(rng)][:40]
    off = (np.concatenate([[0], np.cumsum([len(x) for x in xs])]) + 7).astype(np.int64)
    samples = np.ascontiguousarray(np.concatenate([np.zeros(7, np.int16)] + xs))
    n, items = int(off[-1] - off[0]), len(xs)
    count, trunc = np.full(items, -5, np.int32), np.full(items, 9, np.uint8)
    border, level = np.full(n + items, -5, np.int32), np.full(n, -5, np.int16)
    lib = _lib.load()
    _lib.check(lib.chiron_signal_events(samples.ctypes.data, off.ctypes.data, items, 4, 3, 900, 6, 0, count.ctypes.data, border.ctypes.data, level.ctypes.data,
                                        trunc.ctypes.data))
    for i, x in enumerate(xs):
        lv, bd, cut = ref.segment_numpy(x, 4, 3, 900, 6)
        at = int(off[i] - off[0])
        assert count[i] == len(lv) and trunc[i] == int(cut)
        assert np.array_equal(level[at:at + len(lv)], lv) and (level[at + len(lv):at + len(x)] == -5).all()
        assert np.array_equal(border[at + i:at + i + len(bd)], bd) and (border[at + i + len(bd):at + i + len(x) + 1] == -5).all()
    assert trunc.sum() > 3


def test_noise_free_steps_are_recovered_exactly_and_placed_at_cost_zero():
    """Truth for the detector and the DP together: a walk over consecutive columns of a reference of distinct levels, every dwell
    at least 2 w samples and no noise.  The detector at the defaults (w = 3, r = 2, thr = 768) finds every border and every level
    exactly -- at a border T is 6912 d^2 at least, one sample off it is 1536 and within the radius, two off 384 and below the
    threshold -- and the DP puts the events on the planted columns at cost 0 with the right start."""
    rng = np.random.default_rng(8005)
    for k in range(200):
        R = int(rng.integers(30, 90))
        e = rng.permutation(np.arange(-60, 60, dtype=np.int32) * int(rng.integers(1, 40)))[:R]
        first, m = int(rng.integers(0, R - 12)), int(rng.integers(1, 12))
        dwell = rng.integers(2 * W, 2 * W + 9, m)
        x = np.repeat(e[first:first + m], dwell).astype(np.int16)
        for seg in (ref.segment_plain, ref.segment_numpy):
            lv, bd, cut = seg(x, W, RADIUS, THR)
            assert bd.tolist() == np.concatenate([[0], np.cumsum(dwell)]).tolist() and lv.tolist() == e[first:first + m].tolist() and not cut, k
        cols = ref.columns_numpy(lv, e, PENALTY)
        assert cols[first + m - 1] == (0, first) and sum(1 for d, _ in cols if d == 0) == 1
        assert ref.columns_plain(lv, e, PENALTY) == cols


# ----------------------------------------------------------------------------------------------------------------------------
# the entry points without a device
# ----------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_limits_are_bound(built):
    lib = _lib.load()
    names = {n for n, _, _ in _lib.SYMBOLS}
    assert {"chiron_signal_events", "chiron_event_locate_workspace_size", "chiron_event_locate"} <= names and hasattr(lib, "chiron_event_locate")
    header = open(os.path.join(ROOT, "include", "chiron_amd.h")).read()
    for name in ("MAX_SAMPLES", "MAX_WINDOW", "MAX_RADIUS", "MAX_THRESHOLD", "MAX_QUERY", "MAX_PENALTY", "CHUNK", "HALO"):
        text = header.split("#define CHIRON_EVENT_%s " % name)[1].split("\n")[0].split("/*")[0].strip().replace("ll", "")
        assert eval(text) == getattr(_lib, "EVENT_" + name), name
    assert lib.chiron_abi_version() == 7 and _lib.EVENT_MAX_QUERY * (65535 + _lib.EVENT_MAX_PENALTY) < 1 << 30


def test_workspace_size_rules(built):
    lib = _lib.load()
    up = lambda v: (v + 255) // 256 * 256
    assert locate.workspace_size_events(3, 1000, 2049) == up(32) + up(2000) + up(4 * 2049) + up(3 * 3 * 12) + 2 * up(3 * 3072 * 8)
    assert locate.workspace_size_events(3, 1000, 2049) == locate.workspace_size(3, 1000, 2049)
    assert locate.workspace_size_events(0, 0, 0) == 0 and locate.workspace_size_events(1, 1, 1) == 3 * 256 + up(12) + 2 * 8192
    n = C.c_size_t()
    for k in range(3):
        args = [1, 1, 1]
        args[k] = -1
        assert lib.chiron_event_locate_workspace_size(*args, C.byref(n)) == _lib.ERR_INVALID and b"negative size" in lib.chiron_last_error()
    assert lib.chiron_event_locate_workspace_size(1, 1, 1, None) == _lib.ERR_INVALID and b"chiron_event_locate_workspace_size: null bytes" in lib.chiron_last_error()
    for args, word in (((1 << 31, 1, 1), "items in one call"), ((1, _lib.SIGNAL_MAX_SAMPLES + 1, 1), "events in one call"),
                       ((1, 1, _lib.LOCATE_MAX_REF + 1), "ref_len"), ((1 << 20, 1, 1 << 21), "row cells")):
        with pytest.raises(_lib.ChironError) as ei:
            locate.workspace_size_events(*args)
        assert ei.value.status == _lib.ERR_OVERFLOW and word in str(ei.value), args
    base = locate.workspace_size_events(5, 5000, 3000)
    assert all(locate.workspace_size_events(5 + a, 5000 + 300 * b, 3000 + 100 * c) > base for a, b, c in ((1, 0, 0), (0, 1, 0), (0, 0, 1)))
    assert locate.plan_batches([400] * 10, 3000, locate.workspace_size_events(3, 1200, 3000), locate.workspace_size_events) == [(0, 3), (3, 6), (6, 9), (9, 10)]


def _call(lib, events=(1, 2, 3, 4, 5, 6), event_off=(0, 4, 6), items=2, level=(10, -10, 0), ref_len=3, penalty=150, out=True, ws=0, ws_bytes=0, flags=0):
    """Two queries of 4 and 2 events on three columns.  With ws = 0 a call that passes every check ends at the null workspace."""
    arr = lambda v, t: None if v is None else np.ascontiguousarray(np.asarray(v, dtype=t))
    a = [arr(events, np.int16), arr(event_off, np.int64), arr(level, np.int32)]
    o = np.full(24, 77, np.int32)                # a refused call writes nothing, whatever it was promised
    p = [None if x is None else x.ctypes.data for x in a]
    st = lib.chiron_event_locate(0, p[0], p[1], items, p[2], ref_len, penalty, o.ctypes.data if out else None, ws, ws_bytes, flags, None)
    return st, lib.chiron_last_error().decode(), o


def test_every_refusal_of_the_dp_comes_before_a_device(built):
    lib = _lib.load()
    INVALID, OVERFLOW = _lib.ERR_INVALID, _lib.ERR_OVERFLOW
    st, msg, o = _call(lib)
    assert st == INVALID and "chiron_event_locate: null workspace" in msg            # everything else passed: the last check before the device
    assert (o == 77).all()
    long_off = (0, 4, 4 + _lib.EVENT_MAX_QUERY + 1)
    for kw, status, text in (
            (dict(flags=4), INVALID, "unknown flags 0x4"),
            (dict(penalty=-1), INVALID, "penalty -1 outside 0..65534"),
            (dict(penalty=65535), INVALID, "penalty 65535 outside 0..65534"),
            (dict(items=-1), INVALID, "negative size"),
            (dict(ref_len=-1), INVALID, "negative size"),
            (dict(items=1 << 31), OVERFLOW, "items in one call"),
            (dict(ref_len=_lib.LOCATE_MAX_REF + 1), OVERFLOW, "ref_len 268435457, at most 268435456"),
            (dict(event_off=None), INVALID, "null events / event_off"),
            (dict(events=None), INVALID, "null events / event_off"),
            (dict(level=None), INVALID, "null ref_level"),
            (dict(out=False), INVALID, "null block_out"),
            (dict(event_off=(-1, 4, 6)), INVALID, "event_off[0] = -1 is negative"),
            (dict(event_off=(0, 4, 3)), INVALID, "event_off[2] = 3 below its predecessor 4"),
            (dict(event_off=(0, 4, 4)), INVALID, "query 1 is empty"),
            (dict(event_off=(2, 2, 6)), INVALID, "query 0 is empty"),
            (dict(event_off=long_off, events=np.zeros(long_off[-1], np.int16)), OVERFLOW, "query 1 has 8193 events, at most 8192"),
            (dict(level=(10, 32768, 0)), INVALID, "level 32768 of column 1 outside -32767..32767 and not the break value"),
            (dict(level=(10, -10, -32768)), INVALID, "level -32768 of column 2 outside -32767..32767 and not the break value"),
            (dict(level=(-(1 << 31) + 1, 0, 0)), INVALID, "level -2147483647 of column 0 outside")):
        st, msg, o = _call(lib, **kw)
        assert st == status and text in msg and msg.startswith("chiron_event_locate: "), (kw, st, msg)
        assert (o == 77).all(), kw
    # what is legal: the extreme levels and penalties, break columns, a query at the cap, offsets that start above 0
    cap = (3, 3 + _lib.EVENT_MAX_QUERY, 4 + _lib.EVENT_MAX_QUERY)
    for kw in (dict(level=(32767, -32767, locate.BREAK)), dict(level=(locate.BREAK,) * 3), dict(event_off=cap, events=np.zeros(cap[-1], np.int16)),
               dict(penalty=0), dict(penalty=65534)):
        st, msg, _ = _call(lib, **kw)
        assert st == INVALID and "null workspace" in msg, (kw, msg)


def test_dp_calls_that_need_no_device(built):
    lib = _lib.load()
    st, _, o = _call(lib, items=0)
    assert st == _lib.OK and (o == 77).all()                                            # no item: nothing is written
    st, _, o = _call(lib, items=0, events=None, event_off=None, level=None, out=False)
    assert st == _lib.OK
    st, _, o = _call(lib, ref_len=0, level=None, out=False)
    assert st == _lib.OK                                                                # no column: no block to fill
    st, msg, _ = _call(lib, ref_len=0, level=None, event_off=(0, 4, 4))
    assert st == _lib.ERR_INVALID and "query 1 is empty" in msg                         # the queries are still checked
    st, msg, _ = _call(lib, items=0, penalty=70000)
    assert st == _lib.ERR_INVALID and "penalty 70000" in msg                            # and so is the penalty
    assert locate.event_locate_call([], np.zeros(1500, np.int32)).shape == (0, 2, 3)
    got = locate.event_locate_call([np.zeros(3, np.int16)], np.zeros(0, np.int32), 7)
    assert got.shape == (1, 0, 3) and got.dtype == np.int32


def _events(lib, samples=(1, 2, 3, 40, 50, 60, 70, 80), sample_off=(0, 5, 8), items=2, window=3, radius=2, threshold=768, max_events=100, flags=0,
            null=()):
    arr = lambda v, t: None if v is None else np.ascontiguousarray(np.asarray(v, dtype=t))
    a = [arr(samples, np.int16), arr(sample_off, np.int64)]
    outs = [np.full(4, 77, np.int32), np.full(24, 77, np.int32), np.full(24, 77, np.int16), np.full(4, 77, np.uint8)]
    p = [None if x is None else x.ctypes.data for x in a] + [None if k in null else o.ctypes.data for k, o in enumerate(outs)]
    st = lib.chiron_signal_events(p[0], p[1], items, window, radius, threshold, max_events, flags, p[2], p[3], p[4], p[5])
    return st, lib.chiron_last_error().decode(), outs


def test_every_refusal_of_the_detector_comes_before_a_write(built):
    lib = _lib.load()
    INVALID, OVERFLOW = _lib.ERR_INVALID, _lib.ERR_OVERFLOW
    st, _, outs = _events(lib)
    assert st == _lib.OK and outs[0][:2].tolist() == [1, 1] and outs[1][:5].tolist() == [0, 5, 77, 77, 77] and outs[1][6:8].tolist() == [0, 3]
    assert outs[2][:2].tolist() == [19, 77] and outs[2][5:7].tolist() == [70, 77] and outs[3][:3].tolist() == [0, 0, 77]
    long_off = (0, 5, 5 + _lib.EVENT_MAX_SAMPLES + 1)
    for kw, status, text in (
            (dict(flags=2), INVALID, "unknown flags 0x2"),
            (dict(items=-1), INVALID, "negative size (items -1)"),
            (dict(items=1 << 31), OVERFLOW, "items in one call"),
            (dict(window=1), INVALID, "window 1 outside 2..16"),
            (dict(window=17), INVALID, "window 17 outside 2..16"),
            (dict(radius=0), INVALID, "radius 0 outside 1..16"),
            (dict(radius=17), INVALID, "radius 17 outside 1..16"),
            (dict(threshold=0), INVALID, "threshold 0 outside 1..2^52"),
            (dict(threshold=(1 << 52) + 1), INVALID, "threshold 4503599627370497 outside 1..2^52"),
            (dict(max_events=0), INVALID, "max_events 0 outside 1..131072"),
            (dict(max_events=131073), INVALID, "max_events 131073 outside 1..131072"),
            (dict(samples=None), INVALID, "null samples / sample_off"),
            (dict(sample_off=None), INVALID, "null samples / sample_off"),
            (dict(null=(0,)), INVALID, "null count_out / border_out / level_out / truncated_out"),
            (dict(null=(1,)), INVALID, "null count_out"),
            (dict(null=(2,)), INVALID, "null count_out"),
            (dict(null=(3,)), INVALID, "null count_out"),
            (dict(sample_off=(-2, 5, 8)), INVALID, "sample_off[0] = -2 is negative"),
            (dict(sample_off=(0, 5, 4)), INVALID, "sample_off[2] = 4 below its predecessor 5"),
            (dict(sample_off=(0, 5, 5)), INVALID, "item 1 is empty"),
            (dict(sample_off=long_off, samples=np.zeros(long_off[-1], np.int16)), OVERFLOW, "item 1 has 131073 samples, at most 131072")):
        st, msg, outs = _events(lib, **kw)
        assert st == status and text in msg and msg.startswith("chiron_signal_events: "), (kw, st, msg)
        assert all((o == 77).all() for o in outs), kw
    st, _, outs = _events(lib, items=0, samples=None, sample_off=None, null=(0, 1, 2, 3))
    assert st == _lib.OK                                                                # no item: nothing is needed and nothing written
    for kw in (dict(window=2), dict(window=16), dict(radius=16), dict(threshold=1 << 52), dict(max_events=131072), dict(max_events=1)):
        assert _events(lib, **kw)[0] == _lib.OK, kw


def test_host_code_under_sanitizers(tmp_path):
    """tests/native/event_pack_check.cpp, built with the ROCm host compiler under AddressSanitizer + UndefinedBehaviorSanitizer:
    csrc/event_pack.h's offset walk and detector in buffers of exactly the stated size."""
    exe = str(tmp_path / "event_pack_check")
    cmd = [os.path.join(rocm_prefix(), "llvm", "bin", "clang++"), "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", os.path.join(HERE, "native", "event_pack_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "event pack OK" in r.stdout


# ----------------------------------------------------------------------------------------------------------------------------
# the host side
# ----------------------------------------------------------------------------------------------------------------------------
def test_locate_with_events_words_its_rows(built):
    """locate(events=...) with the reference as locator=: the locator gets the detector's levels, a row carries its events, cost and
    margin are per event, the second locus lies more than 2 x events columns away, truncation is counted, and the file gains one
    column.  Without events= nothing changes."""
    rng = np.random.default_rng(8006)
    e = rng.permutation(np.arange(-1500, 1500, dtype=np.int32) * 8)[:2600]
    cmap = locate.ColumnMap(["c"], [1300])
    e[1300] = locate.BREAK
    e = e[:cmap.columns]
    reads, firsts = [], []
    for k in range(6):
        first = int(rng.integers(10, 600)) + (1301 if k % 2 else 0)
        x, _ = cases.walk_query(rng, e, first, 900, noise=6, mean_dwell=9.0)
        reads.append(("r%d" % k, x.astype(np.float32)))
        firsts.append(first)
    seen = []

    def locator(queries, level):
        seen.append([np.asarray(q) for q in queries])
        return ref.locate(queries, level, 40)
    ev = {"window": 3, "threshold": 4.0, "radius": 2, "penalty": 40}
    got = locate.locate(reads, e, cmap, prefix=900, mode="none", min_samples=100, locator=locator, events=ev)
    assert len(seen) == 1 and got["truncated"] == 0 and got["batches"] == 1 and len(got["rows"]) == 6
    total = 0
    for row, (name, x), q, first in zip(got["rows"], reads, seen[0], firsts):
        lv, _, _ = ref.segment_numpy(np.rint(x).astype(np.int16), 3, 2, 1024)
        assert np.array_equal(q, lv) and row["events"] == len(lv) and row["samples"] == 900 and q.dtype == np.int16
        s = locate.summarise(ref.locate([lv], e, 40)[0], 2 * len(lv))
        assert row["cost_per_sample"] == s["best"][0] / len(lv) and (row["end_column"], row["start_column"]) == s["best"][1:]
        assert row["margin"] == (None if s["second"] is None else (s["second"] - s["best"][0]) / len(lv))
        assert abs(row["start_column"] - first) <= 3 and row["strand"] == "+-"[first > 1300]
        total += len(lv)
    assert got["samples_per_event"] == 6 * 900 / total and 4 < got["samples_per_event"] < 12
    lines = locate.located_lines(got["rows"], events=True)
    assert lines[0].split("\t")[:4] == ["read", "samples", "events", "contig"] and lines[1].split("\t")[2] == str(got["rows"][0]["events"])
    assert len(lines[1].split("\t")) == len(locate.LOCATED_COLUMNS) + 1
    # a read of more events than a query may have keeps the first 8192 and is counted
    x = np.repeat(np.tile(np.array([-4000, 4000], np.float32), 4200), 6)
    got = locate.locate([("long", x)], e, cmap, prefix=len(x), mode="none", locator=lambda q, lv: np.full((len(q), 3, 3), locate.NONE, np.int32), events={})
    assert got["truncated"] == 1 and got["rows"][0]["events"] == 8192 and got["rows"][0]["samples"] == len(x) and got["rows"][0]["status"] == "unplaced"
    with pytest.raises(ValueError):
        locate.locate(reads, e, cmap, prefix=20000, locator=locator)                    # without events the prefix keeps its cap
    with pytest.raises(ValueError):
        locate.locate(reads, e, cmap, prefix=(1 << 17) + 1, locator=locator, events={})
    with pytest.raises(ValueError):
        locate.locate(reads, e, cmap, locator=locator, events={"windw": 3})
    plain = locate.locate(reads, e, cmap, prefix=900, mode="none", min_samples=100, locator=locate_ref.locate)
    assert sorted(plain) == ["batches", "dropped", "rows", "status"] and "events" not in plain["rows"][0]
    assert locate.event_threshold(3.0) == 768 and locate.event_threshold(0.002) == 1


def test_the_command_line():
    from chiron_amd import entry
    base = ["locate", "-s", "sig", "-g", "g.fa", "--table", "kmer_levels.tsv", "-o", "out"]
    args = entry.build_parser().parse_args(base)
    assert (args.events, args.event_window, args.event_threshold, args.event_radius, args.skip_penalty) == (False, 3, 3.0, 2, 150)
    d = locate.EVENT_DEFAULTS
    assert (d["window"], d["threshold"], d["radius"], d["penalty"]) == (args.event_window, args.event_threshold, args.event_radius, args.skip_penalty)
    args = entry.build_parser().parse_args(base + ["--events", "--event-window", "5", "--event-threshold", "2.5", "--event-radius", "4", "--skip-penalty", "90",
                                                   "--prefix", "50000"])
    assert (args.events, args.event_window, args.event_threshold, args.event_radius, args.skip_penalty, args.prefix) == (True, 5, 2.5, 4, 90, 50000)


# ----------------------------------------------------------------------------------------------------------------------------
# the planted case, on the reference alone
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", cases.SEEDS)
def test_planted_reads_are_found_again_by_their_events(seed, monkeypatch):
    """locate_cases.planted(seed): 30 control reads, the first 1000 samples of each cut into events at the defaults (window 3, t^2 3,
    radius 2) and placed with a skip penalty of 150 on the 1201 columns; the DP is the numpy reference and the detector the numpy
    one, put in the library's place, so the figures are properties of the definitions.
    Measured with the reference, seeds 1 .. 5: 150 of 150 reads on the true strand and within 32 bases of the
    true position of the last used sample (the largest error 13, 4, 20, 6, 3 bases); 139 within 3 (28, 29, 24, 28, 30 of 30);
    170.1, 171.5, 170.0, 171.8, 170.4 events a read in the mean (150 at least, 192 at most), 5.8 to 5.9 samples an event; cost per
    event 53.5 to 61.5 in the median; none truncated.  A path spans at most 2 x events columns, about 340, so 85 of the 150 reads
    have a second locus (19, 18, 16, 15, 17 a seed), with margins per event of 2.6 at least.  The bar is what the reference
    attains: every read on its true strand within 32 bases, and no margin at or below 0."""
    case = cases.planted(seed)
    level, cmap = locate.reference_levels(case["genome"], case["table"], case["k"])
    monkeypatch.setattr(locate, "events_of", lambda q, window, threshold, radius, max_events: ref.segment_numpy(q, window, radius, threshold, max_events))
    got = locate.locate(case["reads"], level, cmap, skip=cases.SKIP, prefix=cases.PREFIX, locator=ref.locator(PENALTY), events={})
    assert len(got["rows"]) == 30 and got["status"] == {"placed": 30, "ambiguous": 0, "unplaced": 0} and got["truncated"] == 0
    errors, margins, on_strand = [], [], 0
    for row, truth in zip(got["rows"], case["truth"]):
        pos, strand = cases.true_locus(truth, row["samples"] - 1)
        _, at, s = cmap.column_to_locus(row["end_column"])
        on_strand += int(s == strand)
        errors.append(abs(at - pos))
        assert row["start"] <= at < row["end"] and row["contig"] == "ctg" and row["samples"] == 1000 and 100 < row["events"] < 250
        if row["margin"] is not None:
            margins.append(row["margin"])
    print("planted seed %d by events: %d of 30 on the true strand, %d within 3 bases, %d within 32, largest error %d; %.1f events a read, %.2f samples an "
          "event; %d margins, least %.1f; median cost per event %.1f"
          % (seed, on_strand, sum(e <= 3 for e in errors), sum(e <= 32 for e in errors), max(errors), float(np.mean([r["events"] for r in got["rows"]])),
             got["samples_per_event"], len(margins), min(margins) if margins else float("nan"), float(np.median([r["cost_per_sample"] for r in got["rows"]]))))
    assert on_strand == 30
    assert sum(e <= 32 for e in errors) == 30
    assert all(m > 0 for m in margins)
