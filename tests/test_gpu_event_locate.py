"""GPU: chiron_event_locate (csrc/event_locate.hip) through chiron_amd.locate against tests/event_ref.py's numpy rows (which
tests/test_event_cpu.py holds to the plain-Python recurrence and to a brute force), and `locate --events` end to end.  Every result
is a property of the inputs: every block triple is compared with ==."""
import json
import os

import numpy as np
import pytest

from chiron_amd import _lib, locate

import event_ref as ref
import locate_cases as cases
from ws_guard import FILLS, Recorder

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = locate.BREAK
C = _lib.EVENT_CHUNK
R_EDGES = [1, 2, 3, 15, 16, 17, 1023, 1024, 1025, 2049]    # lane, tile and block edges
Q_EDGES = [1, 2, 3, C - 1, C, C + 1, 2 * C + 1]             # chunk edges and the parity of the buffer swap
PENALTIES = [0, 1, 150, 65534]


def _check(queries, e, P):
    """One call against the reference, every triple.  -> the GPU's blocks."""
    got = locate.event_locate_call(queries, e, P)
    want = ref.locate(queries, e, P)
    assert got.dtype == np.int32 and got.shape == want.shape == (len(queries), (len(e) + 1023) // 1024, 3)
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, (P, bad[:5].tolist(), [got[i, b].tolist() for i, b in bad[:5]], [want[i, b].tolist() for i, b in bad[:5]])
    return got


def _distinct_levels(rng, R):
    """R distinct levels, 20 apart at least: a sample at a column's level costs 20 or more at any other column."""
    return rng.permutation(np.arange(-R // 2, R - R // 2, dtype=np.int32) * 20)[:R]


def _skips_taken(queries, e, P):
    """How many of the queries are cheaper with the skip than without it (P = 65534 on levels within +-300 never pays)."""
    with_skip, without = ref.locate(queries, e, P), ref.locate(queries, e, 65534)
    return int((with_skip[:, :, 0].min(axis=1) < without[:, :, 0].min(axis=1)).sum())


def test_constants_agree_with_the_header(built):
    header = open(os.path.join(ROOT, "include", "chiron_amd.h")).read()
    for name in ("MAX_QUERY", "MAX_PENALTY", "CHUNK", "HALO"):
        assert int(header.split("#define CHIRON_EVENT_%s " % name)[1].split()[0]) == getattr(_lib, "EVENT_" + name)
    assert C == 64 and _lib.EVENT_HALO == 2 * C and locate.EVENT_MAX_QUERY == 8192


@pytest.mark.parametrize("R", R_EDGES)
def test_reference_and_query_edges(built, R):
    """Every Q of Q_EDGES, each in a call of its own and all in one call, on a reference of R columns, at every penalty: narrow
    levels, where the skip pays at the small penalties, and levels over the whole range with a fifth of the columns breaks."""
    rng = np.random.default_rng(7000 + R)
    for k, P in enumerate(PENALTIES):
        breaks, wide = ((0.0, False), (0.2, True))[k % 2]
        e = cases.random_reference(rng, R, breaks, wide)
        queries = [cases.random_query(rng, Q, wide) for Q in Q_EDGES]
        together = _check(queries, e, P)
        if P in (0, 150):                                                           # one call an item at two of the penalties
            for i, q in enumerate(queries):
                assert np.array_equal(_check([q], e, P)[0], together[i])           # a result does not depend on what else the call holds
    if R >= 15:
        e = cases.random_reference(rng, R)
        queries = [cases.random_query(rng, Q) for Q in Q_EDGES]
        assert _skips_taken(queries, e, 1) >= 4                                     # the skip is not idle in these cases


@pytest.mark.parametrize("R", [17, 1025, 2049])
def test_the_two_kernels_agree_where_no_skip_can_pay(built, R):
    """event_locate_kernel and locate_kernel are one sweep at two reaches (csrc/locate_sweep.h); this holds them to each other.  P =
    65534, levels and queries within +-300 and Q <= 100: a path without a skip to any column costs at most 100 x 600 < P, so no
    cheapest path holds a skip and chiron_event_locate gives chiron_signal_locate's triples, every one.  At P = 0 it does not."""
    rng = np.random.default_rng(7700 + R)
    for breaks in (0.0, 0.1):
        e = cases.random_reference(rng, R, breaks)
        queries = [cases.random_query(rng, Q) for Q in (1, C - 1, C, C + 1, 100)]
        assert all(len(q) * 600 < 65534 for q in queries)
        by_samples = locate.locate_call(queries, e)
        assert np.array_equal(locate.event_locate_call(queries, e, 65534), by_samples)
        assert not np.array_equal(locate.event_locate_call(queries, e, 0), by_samples)


def _path_query(e, cols):
    return e[np.asarray(cols)].astype(np.int16)


SKIP_EDGES = [(14, 16), (15, 17), (1022, 1024), (1023, 1025), (1038, 1040), (1039, 1041)]    # lane edges of tile 0 and 1, the tile edge


def test_skips_across_lane_and_tile_edges(built):
    """Queries that are the reference's own levels along a path with exactly one skip, a -> a + 2 for every pair of SKIP_EDGES, at
    every row of a short query and across a chunk edge: the cheapest path costs the penalty alone.  Then the same with a break at
    the skipped column, which forbids the skip: equality with the reference, and a cost above the penalty."""
    rng = np.random.default_rng(7100)
    e = _distinct_levels(rng, 2100)
    P = 7
    queries, want, edge = [], [], []
    for a, b in SKIP_EDGES:
        for before, after in ((1, 1), (3, 2), (C - 1, 1), (C, 1), (C + 1, 3), (2 * C, 2)):      # the skip at row `before`
            cols = list(range(a - before + 1, a + 1)) + list(range(b, b + after))
            if cols[0] < 0:
                continue
            queries.append(_path_query(e, cols))
            want.append([P, cols[-1], cols[0]])
            edge.append(a)
    got = _check(queries, e, P)
    for g, w in zip(got, want):
        assert g[w[1] // 1024].tolist() == w
    for a, b in SKIP_EDGES:
        eb = e.copy()
        eb[a + 1] = B
        sub = [q for q, at in zip(queries, edge) if at == a]
        assert len(sub) >= 2
        got = _check(sub, eb, P)
        assert (got[:, :, 0].min(axis=1) > P).all()
    # a break elsewhere on the path's stretch does not forbid it: one column past the end, one before the start
    eb = e.copy()
    eb[[9, 20, 1019, 1030]] = B
    got = _check([_path_query(e, [12, 13, 14, 16, 17]), _path_query(e, [1021, 1022, 1024, 1025])], eb, P)
    assert got[0, 0].tolist() == [P, 17, 12] and got[1, 1].tolist() == [P, 1025, 1021]


def test_the_halo_is_wide_enough(built):
    """Paths that skip at every row, two columns a row: the furthest a path can come from.  Into owned column 1024 of tile 1 -- in
    launch 0 from column 1024 - 2 * 63 = 898, the halo's column 2, over 63 steps; in launch 1 from the halo's column 0 (896), where
    the path stands at the launch's start, over 64 steps -- and the same one column on (1025), one row more (a stay at the end) and
    one row fewer.  Each costs its skips alone.  A break on a skipped column of such a path must forbid it."""
    rng = np.random.default_rng(7200)
    e = _distinct_levels(rng, 2300)
    P = 1
    queries, want = [], []
    for end in (1024, 1025, 1026, 2048, 2049):
        for Q in (C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1):
            cols = [end - 2 * (Q - 1 - t) for t in range(Q)]
            queries.append(_path_query(e, cols))
            want.append([P * (Q - 1), end, cols[0]])
            queries.append(_path_query(e, cols + [end]))                            # one stay at the end
            want.append([P * (Q - 1), end, cols[0]])
    got = _check(queries, e, P)
    for g, w in zip(got, want):
        assert g[w[1] // 1024].tolist() == w, (g.tolist(), w)
    for at in (897, 899, 1023, 961):                                                # skipped columns of the paths that end at 1024
        eb = e.copy()
        eb[at] = B
        got = _check(queries[:24], eb, P)
        assert sum(1 for g, w in zip(got, want[:24]) if g[1].tolist() != w) >= 6


def test_uneven_items_in_one_call(built):
    """Q = 1, 64, 65 and 200 together, in every order of first and last: items idle in later launches, each reduced in its own."""
    rng = np.random.default_rng(7300)
    e = cases.random_reference(rng, 2049, 0.02)
    lens = [1, C, C + 1, 200]
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 0, 3, 1]):
        _check([cases.random_query(rng, lens[k]) for k in order], e, 150)
    walk = [cases.walk_query(rng, np.where(e == B, 0, e), first, Q, mean_dwell=1.2)[0][::2] for first, Q in ((3, 400), (900, 130), (1500, 128), (2040, 2))]
    _check(walk, e, 40)


def test_breaks(built):
    """Breaks at columns 0, 1, 1022, 1023, 1024 and R - 1, runs of breaks longer than the halo on either side of a tile edge, single
    breaks that a skip would cross, and an all-break reference, where every triple is NONE."""
    rng = np.random.default_rng(7400)
    queries = [cases.random_query(rng, Q) for Q in (1, 2, C, C + 1, 2 * C + 1, 200)]
    R = 2300
    for at in ([0], [1], [1022], [1023], [1024], [R - 1], [0, 1023, 1024, R - 1], list(range(1024 - 140, 1024)), list(range(1024, 1024 + 140)),
               list(range(1024 - 70, 1024 + 70)), list(range(0, 1024)), list(range(1024, 2048)), list(range(5, R)), list(range(1, R, 2)), list(range(0, R, 3))):
        e = cases.random_reference(rng, R)
        e[at] = B
        _check(queries, e, 3)
    for R in (1, 1024, 1025, 2049):
        got = _check(queries, np.full(R, B, np.int32), 0)
        assert (got == locate.NONE).all()
    got = _check(queries, np.concatenate([np.full(1024, B, np.int32), cases.random_reference(rng, 30)]), 0)
    assert (got[:, 0] == locate.NONE).all() and (got[:, 1] != locate.NONE).all()


@pytest.mark.parametrize("R,Q", [(17, 2), (1025, C + 1), (2049, 2 * C + 1)])
def test_ties(built, R, Q):
    """A constant signal on a constant reference at P = 0: every path costs the same, skip and move tie, and the tie rule alone
    decides -- the smallest end of a block, and the smallest start: as far left as Q - 1 skips reach."""
    for x, lv in ((7, 7), (7, 3)):
        got = _check([np.full(Q, x, np.int16), np.full(1, x, np.int16)], np.full(R, lv, np.int32), 0)
        for b in range(got.shape[1]):
            assert got[0, b].tolist() == [abs(x - lv) * Q, 1024 * b, max(1024 * b - 2 * (Q - 1), 0)] and got[1, b].tolist() == [abs(x - lv), 1024 * b, 1024 * b]
    got = _check([np.full(Q, 7, np.int16)], np.full(R, 7, np.int32), 1)              # at P = 1 a skip no longer ties: one column a row
    assert got[0, -1].tolist() == [0, 1024 * (got.shape[1] - 1), max(1024 * (got.shape[1] - 1) - (Q - 1), 0)]


def test_the_32_bit_bound(built):
    """Events and levels at the ends of their range with Q = 8192, P = 65534, on R = 70: the largest costs there are stay below the
    kernel's 2^30, through 128 launches."""
    Q = locate.EVENT_MAX_QUERY
    x = np.full(Q, 32767, np.int16)
    e = np.full(70, -32767, np.int32)
    e[[10, 40]] = B
    e[50:] = 32767
    got = _check([x, (-x).astype(np.int16), x[:Q - 1]], e, 65534)
    assert got[0, 0].tolist() == [0, 50, 50] and got[1, 0].tolist() == [0, 0, 0]
    e[50:] = -32767
    got = _check([x, np.full(Q, -32768, np.int16)], np.where(e == B, B, -e).astype(np.int32), 65534)
    assert got[1, 0].tolist() == [Q * 65535, 0, 0] and Q * (65535 + 65534) < 1 << 30
    # a path that has to pay the penalty at every row but the first to stay cheap: alternate columns match
    e = np.full(2 * 40 + 1, -32767, np.int32)
    e[0::2] = 32767
    q = np.full(41, 32767, np.int16)
    q[1::2] = 32766
    got = _check([q], e, 65534)


def test_more_units_than_waves(built):
    """More (item, tile) units than a launch has waves, so that waves take a second unit: 4100 queries on two tiles, some of them
    with a second launch."""
    waves = _lib.LOCATE_THREADS // 64 * _lib.LOCATE_MAX_GROUPS
    rng = np.random.default_rng(7500)
    items = 4100
    assert 2 * items > waves
    e = cases.random_reference(rng, 1030, 0.02)
    lens = np.where(np.arange(items) % 41 == 0, C + 2, rng.integers(1, 4, items))
    lens[-1] = C + 1
    _check([cases.random_query(rng, int(Q)) for Q in lens], e, 150)


def test_workspace_contract(built, monkeypatch):
    """"Caller's memory" of include/chiron_amd.h for chiron_event_locate: under each fill of tests/ws_guard.py the workspace is
    exactly the size function's bytes between two guards and holds the fill on entry, and so does the host output.  The guards are
    intact afterwards, the result equals the reference under all three (which an element left unwritten cannot), and the three
    results are the same bytes.  A workspace said to be one byte short is refused before anything is written."""
    import torch
    rng = np.random.default_rng(7600)
    e = cases.random_reference(rng, 2049 + 600, 0.03)
    e[1000:1100] = B
    queries = [cases.random_query(rng, Q) for Q in (1, C - 1, C, C + 1, 2 * C + 1, 200, 2)]
    queries.append(cases.walk_query(rng, np.where(e == B, 0, e), 1900, 300, mean_dwell=1.2)[0][::2])
    P = 150
    event_off = np.concatenate([[0], np.cumsum([len(q) for q in queries])]).astype(np.int64) + 5
    events = np.ascontiguousarray(np.concatenate([np.zeros(5, np.int16)] + queries))
    items, blocks = len(queries), (len(e) + 1023) // 1024
    need = locate.workspace_size_events(items, int(event_off[-1] - event_off[0]), len(e))
    want = ref.locate(queries, e, P)
    assert (want[:, 0] == locate.NONE).sum() == 0 and blocks == 3
    results = []
    for fill in FILLS:
        rec = Recorder(fill)
        monkeypatch.setattr(_lib, "alloc_hook", rec)
        try:
            lib, ws, stream = _lib.device_workspace(need, 0, "test", "event locate kernel")
            out = np.full((items, blocks, 3), fill * 0x01010101, dtype=np.uint32).view(np.int32)
            before = out.copy()
            st = lib.chiron_event_locate(0, events.ctypes.data, event_off.ctypes.data, items, e.ctypes.data, len(e), P, out.ctypes.data, ws.data_ptr(), need - 1, 0, stream)
            assert st == _lib.ERR_INVALID and ("a workspace of %d bytes, %d are needed" % (need - 1, need)) in lib.chiron_last_error().decode()
            assert np.array_equal(out, before)
            _lib.check(lib.chiron_event_locate(0, events.ctypes.data, event_off.ctypes.data, items, e.ctypes.data, len(e), P, out.ctypes.data, ws.data_ptr(), need, 0, stream))
        finally:
            monkeypatch.setattr(_lib, "alloc_hook", None)
        torch.cuda.synchronize()
        rec.check()
        assert rec.sizes == [need]
        assert np.array_equal(out, want), fill
        results.append(out.tobytes())
    assert len(results) == 3 and results[0] == results[1] == results[2]


def test_planted_case_through_the_command(built, tmp_path):
    """The planted case as files through `chiron locate --events --prefix 1000`, once on the GPU and once with locator= set to the
    reference: located.tsv is the same bytes and the reports are equal.  Where the reads land is the reference's business
    (tests/test_event_cpu.py); the GPU's bar is equality with it."""
    from chiron_amd import entry, squiggle
    case = cases.planted()
    codes = case["genome"].codes
    (tmp_path / "genome.fa").write_text(">ctg\n%s\n" % "".join("ACGT"[v] for v in codes))
    rows = ["\t".join(squiggle.KMER_COLUMNS) + "\n"]
    for code, lv in enumerate(case["table"].tolist()):
        rows.append("%s\t9\t9.000\t%.5f\t0.10000\n" % ("".join("ACGT"[(code >> (2 * (4 - j))) & 3] for j in range(5)), lv / squiggle.SCALE))
    (tmp_path / "kmer_levels.tsv").write_text("".join(rows))
    (tmp_path / "sig").mkdir()
    for name, raw in case["reads"]:
        (tmp_path / "sig" / (name + ".signal")).write_text(" ".join(str(int(v)) for v in np.rint(raw)))
    argv = ["locate", "-s", str(tmp_path / "sig"), "-g", str(tmp_path / "genome.fa"), "--table", str(tmp_path / "kmer_levels.tsv"), "--prefix",
            str(cases.PREFIX), "--skip", str(cases.SKIP), "--targets", "ctg:1-300", "--events"]
    got = entry.main(argv + ["-o", str(tmp_path / "gpu")])
    args = entry.build_parser().parse_args(argv + ["-o", str(tmp_path / "ref")])
    want = locate.locate_command(args, locator=ref.locator(args.skip_penalty))
    assert (tmp_path / "gpu" / "located.tsv").read_bytes() == (tmp_path / "ref" / "located.tsv").read_bytes()
    on_disk = json.loads((tmp_path / "gpu" / "locate_report.json").read_text())
    assert got == want == on_disk == json.loads((tmp_path / "ref" / "locate_report.json").read_text())
    assert got["reads"] == {"total": 30, "used": 30, "dropped": {"too_short": 0, "flat_signal": 0}} and sum(got["status"].values()) == 30
    assert got["columns"] == 1201 and got["batches"] == 1
    ev = got["events"]
    assert (ev["window"], ev["threshold"], ev["threshold_int"], ev["radius"], ev["skip_penalty"], ev["truncated"]) == (3, 3.0, 768, 2, 150, 0)
    assert 3.0 < ev["samples_per_event"] < 9.0
    lines = [ln.split("\t") for ln in (tmp_path / "gpu" / "located.tsv").read_text().splitlines()]
    assert tuple(lines[0]) == locate.LOCATED_COLUMNS[:2] + ("events",) + locate.LOCATED_COLUMNS[2:] + ("target",) and len(lines) == 31
    assert all(0 < int(f[2]) < int(f[1]) == 1000 and f[3] == "ctg" for f in lines[1:])
