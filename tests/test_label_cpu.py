"""CPU: the host side of `label` (chiron_amd/label.py) and the reference the GPU tests hold chiron_ctc_align to.  The numpy
restatement of the alignment (tests/ctc_align_ref.py) against a brute-force enumeration of every path on tiny cases with real
ties; the host-only size function's argument checks; frame -> sample mapping, spans and the .label round trip; batching; the
subcommand's arguments.  No kernel is launched here."""
import ctypes as C
import os

import numpy as np
import pytest

from chiron_amd import _lib, labelled

import ctc_align_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_equals_brute_force_on_tiny_cases_with_ties():
    """Integer scores in -3..3 (sums are exact, ties are common): the full table, and banded passes that double up to it, give
    the brute-force optimum; L = 0 and infeasible rows included."""
    rng = np.random.default_rng(11)
    n = infeasible = empty = 0
    for _ in range(260):
        F = int(rng.integers(0, 8))
        L = int(rng.integers(0, 4))
        lab = rng.integers(0, 2 if rng.random() < 0.5 else 4, size=L).astype(np.uint8)    # half the cases: many repeats
        x = rng.integers(-3, 4, size=(F, 5)).astype(np.float32)
        want = ref.brute_force(x, lab)
        start, score, band, status = ref.align_one(x, lab, 0, 0)
        if want is None:
            assert status == 1 and score == -np.inf and np.all(start == -1)
            infeasible += 1
        else:
            assert status == 0 and score == want, (F, L, lab, score, want)
            assert band == 0
            if L:
                assert start[0] >= 0 and np.all(np.diff(start) > 0) and start[-1] < F
                rep = lab[1:] == lab[:-1]
                assert np.all(np.diff(start)[rep] >= 2)                  # a blank frame between equal neighbours
            # a banded run ends at the full table at the latest and never beats the optimum
            s1, sc1, b1, st1 = ref.align_one(x, lab, 1, 0)
            assert st1 == 0 and sc1 <= want and b1 >= 1
            if b1 >= 2 * L:
                assert sc1 == want
        empty += L == 0
        n += 1
    assert n >= 200 and infeasible >= 10 and empty >= 10


def test_reference_tie_order_on_all_zero_scores():
    """All scores equal, bases A C C, nine frames.  Stay wins every tie and the end prefers S-1, so the traceback stays in the last
    blank back to the first frame that state can be reached at: A at 0, C at 1, the blank the repeat needs at 2, C at 3, the
    last blank from 4 on.  By hand, not from the code."""
    x = np.zeros((9, 5), dtype=np.float32)
    start, score, band, status = ref.align_one(x, np.array([0, 1, 1], np.uint8), 0, 0)
    assert (start.tolist(), score, band, status) == ([0, 1, 3], 0.0, 0, 0)
    # one unit for C at the last frame: the path ends in the last base (S-2) instead, which it still enters at frame 3
    x[8, 1] = 1.0
    start, score, _, _ = ref.align_one(x, np.array([0, 1, 1], np.uint8), 0, 0)
    assert score == 1.0 and start.tolist() == [0, 1, 3]


def test_symbols_are_bound(built):
    lib = _lib.load()
    names = {n for n, _, _ in _lib.SYMBOLS}
    assert {"chiron_ctc_align_workspace_size", "chiron_ctc_align"} <= names
    assert hasattr(lib, "chiron_ctc_align") and hasattr(lib, "chiron_ctc_align_workspace_size")
    header = open(os.path.join(ROOT, "include", "chiron_amd.h")).read()
    for macro, value in (("CHIRON_LABEL_MAX_FRAMES", _lib.LABEL_MAX_FRAMES), ("CHIRON_LABEL_MAX_BASES", _lib.LABEL_MAX_BASES),
                         ("CHIRON_LABEL_THREADS", _lib.LABEL_THREADS), ("CHIRON_LABEL_LDS_SLOTS", _lib.LABEL_LDS_SLOTS),
                         ("CHIRON_LABEL_MAX_GROUPS", _lib.LABEL_MAX_GROUPS)):
        text = header.split("#define %s " % macro)[1].split("\n")[0].split("/*")[0].strip()
        assert eval(text) == value, macro


def _size(frames, bases, band0, max_band):
    lib = _lib.load()
    fo = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
    lo = np.concatenate([[0], np.cumsum(bases)]).astype(np.int64)
    n = C.c_size_t(12345)
    st = lib.chiron_ctc_align_workspace_size(len(frames), fo.ctypes.data, lo.ctypes.data, band0, max_band, C.byref(n))
    return st, n.value


def test_workspace_size_errors(built):
    lib = _lib.load()
    n = C.c_size_t()
    good = np.array([0, 10, 30], np.int64)
    bad = np.array([0, 30, 10], np.int64)
    neg = np.array([-1, 10, 30], np.int64)
    for fo, lo in ((bad, good), (good, bad), (neg, good)):
        assert lib.chiron_ctc_align_workspace_size(2, fo.ctypes.data, lo.ctypes.data, 8, 0, C.byref(n)) == _lib.ERR_INVALID
    assert b"ctc_align" in lib.chiron_last_error()
    assert _size([100], [10], 16, 8)[0] == _lib.ERR_INVALID                     # max_band below band0
    assert _size([100], [10], -1, 0)[0] == _lib.ERR_INVALID
    assert _size([100], [10], 4, -1)[0] == _lib.ERR_INVALID
    assert _size([100], [10], 16, 16)[0] == _lib.OK
    assert _size([100], [10], 0, 8)[0] == _lib.OK                               # band0 = 0: the full table, max_band has nothing to bound
    assert _size([_lib.LABEL_MAX_FRAMES + 1], [10], 8, 0)[0] == _lib.ERR_OVERFLOW
    assert _size([100], [_lib.LABEL_MAX_BASES + 1], 8, 0)[0] == _lib.ERR_OVERFLOW
    assert _size([_lib.LABEL_MAX_FRAMES], [_lib.LABEL_MAX_BASES], 8, 64)[0] == _lib.OK
    assert lib.chiron_ctc_align_workspace_size(1, good.ctypes.data, good.ctypes.data, 8, 0, None) == _lib.ERR_INVALID
    # the aligning call checks its arguments before it looks for a device
    x = np.zeros((30, 5), np.float32)
    lab = np.array([0, 1, 2, 7] + [0] * 26, np.uint8)
    out_i = np.zeros(64, np.int32)
    out_d = np.zeros(4, np.float64)
    args = lambda fo, lo, b0, mb: lib.chiron_ctc_align(0, x.ctypes.data, fo.ctypes.data, lab.ctypes.data, lo.ctypes.data, 2, b0, mb, 0,
                                                       out_i.ctypes.data, out_d.ctypes.data, out_i.ctypes.data, out_i.ctypes.data, None, None)
    assert args(bad, good, 8, 0) == _lib.ERR_INVALID
    assert args(good, good, 8, 4) == _lib.ERR_INVALID
    assert args(good, good, 8, 0) == _lib.ERR_INVALID and b"code 7" in lib.chiron_last_error()
    assert lib.chiron_ctc_align(0, None, None, None, None, 0, 8, 0, 0, None, None, None, None, None, None) == _lib.OK     # reads == 0


def test_workspace_size_is_monotone_in_max_band_and_zero_for_no_reads(built):
    assert _size([], [], 8, 0) == (_lib.OK, 0)
    frames, bases = [3000, 9000, 500, 0], [300, 4000, 500, 0]
    prev = 0
    for mb in (4, 7, 8, 16, 100, 512, 1024, 4096, 8192, 1 << 20):
        st, n = _size(frames, bases, 4, mb)
        assert st == _lib.OK and n >= prev, (mb, n, prev)
        prev = n
    st, unbounded = _size(frames, bases, 4, 0)
    assert st == _lib.OK and unbounded >= prev
    assert _size(frames, bases, 0, 0) == (st, unbounded)                         # both can reach the full table of every read
    # the back-pointers dominate: F rows of ceil(width / 4) bytes at the widest band, 2 * 1024 + 1 states here for the long read
    st, n = _size([9000], [4000], 4, 1024)
    assert 9000 * 513 <= n < 9000 * 513 + 9000 * 20 + 4000 * 5 + 8192


def test_frames_to_samples():
    from chiron_amd.label import frames_to_samples
    # ratio 1: three windows of 400, 400 and 200 frames; the frame index is the sample index
    f = np.array([0, 1, 399, 400, 401, 999])
    assert frames_to_samples(f, [400, 400, 200], 400, 1.0, 1000).tolist() == f.tolist()
    # ratio 500 / 72: window k starts at 500 k, local frame f at round-half-even(f * 500 / 72)
    sl = [72, 72, 30]
    f = np.array([0, 1, 9, 18, 71, 72, 73, 144, 173])
    ratio = 500 / 72
    want = [0, 7, 62, 125, 493, 500, 507, 1000, 1000 + int(np.round(29 * ratio))]
    assert frames_to_samples(f, sl, 500, ratio, 1208).tolist() == want
    assert frames_to_samples([173], sl, 500, ratio, 1150).tolist() == [1150]      # capped at the signal's length
    assert frames_to_samples([3], [10], 10, 2.5, 25).tolist() == [8] and frames_to_samples([1], [10], 10, 2.5, 25).tolist() == [2]   # 7.5 -> 8, 2.5 -> 2
    with pytest.raises(ValueError):
        frames_to_samples([174], sl, 500, ratio, 1208)
    assert frames_to_samples([], sl, 500, ratio, 1208).tolist() == []


def test_spans_and_label_round_trip(tmp_path):
    from chiron_amd.label import spans, write_label
    starts = [3, 10, 11, 40]
    sp = spans(starts, 57)
    assert sp == [(3, 10), (10, 11), (11, 40), (40, 57)]
    bases = np.array([0, 3, 3, 2], np.uint8)
    path = str(tmp_path / "r.label")
    write_label(path, sp, bases)
    assert open(path).read() == "3 10 A\n10 11 T\n11 40 T\n40 57 G\n"
    back = labelled.read_label(path, skip_start=0)
    assert back.start == starts and back.length == [7, 1, 29, 17] and back.base == [0, 3, 3, 2]
    with pytest.raises(ValueError):
        spans([3, 10, 10, 40], 57)                    # two bases start in one sample
    with pytest.raises(ValueError):
        spans([3, 10, 57], 57)                        # the last base starts at the signal's end
    with pytest.raises(ValueError):
        write_label(path, sp, bases[:3])
    assert spans([], 57) == []


def test_plan_batches(built):
    from chiron_amd.label import plan_batches, workspace_size
    frames = [900, 1800, 900, 40000, 900, 900, 2700]
    bases = [100, 200, 100, 4000, 100, 100, 300]
    one = [workspace_size([f], [b], 16, 64) for f, b in zip(frames, bases)]
    budget = one[1] + one[2] + one[0]
    assert one[3] > budget
    got = plan_batches(frames, bases, 16, 64, budget)
    assert [i for b in got for i in b] == list(range(7))                # order kept, every read once
    assert [3] in got                                                   # the oversize read alone
    for b in got:
        assert b == [3] or workspace_size([frames[i] for i in b], [bases[i] for i in b], 16, 64) <= budget
    assert len(got) < 7                                                 # and it does batch
    assert plan_batches(frames, bases, 16, 64, 1 << 40) == [list(range(7))]
    assert plan_batches([], [], 16, 64, 1 << 20) == []


def test_label_subcommand_parses():
    from chiron_amd import entry
    p = entry.build_parser()
    a = p.parse_args(["label", "-i", "in", "-o", "out"])
    assert (a.band, a.max_band, a.workspace_mb, a.segment_len, a.batch_size, a.mode, a.dtype, a.device) == (256, 8192, 4096, 400, 1100, "dna", "fp32", 0)
    assert a.reference is None and a.synthetic_weights is False and a.func is entry.label and a.model.endswith("DNA_default")
    a = p.parse_args(["label", "-i", "in", "-r", "refs.fa", "-o", "out", "-m", "mdl", "-l", "500", "-b", "64", "--band", "0", "--max-band", "0",
                      "--workspace-mb", "128", "--mode", "rna", "--dtype", "fp16", "--device", "2", "--synthetic-weights"])
    assert (a.reference, a.model, a.segment_len, a.batch_size, a.band, a.max_band, a.workspace_mb, a.mode, a.dtype, a.device,
            a.synthetic_weights) == ("refs.fa", "mdl", 500, 64, 0, 0, 128, "rna", "fp16", 2, True)
    with pytest.raises(SystemExit):
        p.parse_args(["label", "-i", "in"])
