"""GPU: chiron_signal_locate (csrc/locate.hip) through chiron_amd.locate against tests/locate_ref.py's numpy rows (which
tests/test_locate_cpu.py holds to the plain-Python recurrence and to a brute force), and the `locate` command end to end.  Every
result is a property of the inputs: every block triple is compared with ==."""
import json
import os

import numpy as np
import pytest

from chiron_amd import _lib, locate

import locate_cases as cases
import locate_ref as ref
from ws_guard import FILLS, Recorder

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = locate.BREAK
R_EDGES = [1, 15, 16, 17, 1023, 1024, 1025, 2049]          # lane, tile and block edges
Q_EDGES = [1, 2, 63, 64, 65, 129]                           # chunk edges and the parity of the buffer swap


def _check(queries, e):
    """One call against the reference, every triple.  -> the GPU's blocks."""
    got = locate.locate_call(queries, e)
    want = ref.locate(queries, e)
    assert got.dtype == np.int32 and got.shape == want.shape == (len(queries), (len(e) + 1023) // 1024, 3)
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, (bad[:5].tolist(), [got[i, b].tolist() for i, b in bad[:5]], [want[i, b].tolist() for i, b in bad[:5]])
    return got


@pytest.mark.parametrize("R", R_EDGES)
def test_reference_and_query_edges(built, R):
    """Every Q of Q_EDGES, each in a call of its own and all in one call, on a reference of R columns: narrow levels, levels over
    the whole range, and a fifth of the columns breaks."""
    rng = np.random.default_rng(6000 + R)
    for breaks, wide in ((0.0, False), (0.2, True)):
        e = cases.random_reference(rng, R, breaks, wide)
        queries = [cases.random_query(rng, Q, wide) for Q in Q_EDGES]
        together = _check(queries, e)
        for k, q in enumerate(queries):
            assert np.array_equal(_check([q], e)[0], together[k])                   # a result does not depend on what else the call holds


def test_uneven_items_in_one_call(built):
    """Q = 1, 64, 65 and 200 together, in every order of first and last: items idle in later launches, each reduced in its own."""
    rng = np.random.default_rng(6100)
    e = cases.random_reference(rng, 2049, 0.02)
    lens = [1, 64, 65, 200]
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 0, 3, 1]):
        _check([cases.random_query(rng, lens[k]) for k in order], e)
    walk = [cases.walk_query(rng, np.where(e == B, 0, e), first, Q)[0] for first, Q in ((3, 200), (900, 65), (1500, 64), (2040, 1))]
    _check(walk, e)


def test_breaks(built):
    """Breaks at columns 0, 1023, 1024 and R - 1, runs of breaks longer than the halo on either side of a tile edge, and an
    all-break reference, where every triple is NONE."""
    rng = np.random.default_rng(6200)
    queries = [cases.random_query(rng, Q) for Q in (1, 64, 65, 129, 200)]
    R = 2300
    for at in ([0], [1023], [1024], [R - 1], [0, 1023, 1024, R - 1], list(range(1024 - 100, 1024)), list(range(1024, 1024 + 100)),
               list(range(1024 - 70, 1024 + 70)), list(range(0, 1024)), list(range(1024, 2048)), list(range(5, R))):
        e = cases.random_reference(rng, R)
        e[at] = B
        _check(queries, e)
    for R in (1, 1024, 1025, 2049):
        got = _check(queries, np.full(R, B, np.int32))
        assert (got == locate.NONE).all()
    got = _check(queries, np.concatenate([np.full(1024, B, np.int32), cases.random_reference(rng, 30)]))
    assert (got[:, 0] == locate.NONE).all() and (got[:, 1] != locate.NONE).all()


def test_paths_across_a_tile_edge(built):
    """A query that is the reference's own levels, 8 samples a column, from column 1016 on: it leaves tile 0 for tile 1 exactly at
    the chunk edge (sample 64).  Cost 0, the end in block 1, the start 1016 in block 0.  And random walks across every tile edge of
    a longer reference, started up to 60 columns before it."""
    rng = np.random.default_rng(6300)
    e = rng.permutation(np.arange(-1500, 1500, dtype=np.int32) * 20)                 # 3000 distinct levels, 20 apart at least
    cols = 1016 + np.arange(128) // 8
    got = _check([e[cols].astype(np.int16), e[cols[:65]].astype(np.int16), e[cols[:64]].astype(np.int16)], e)
    assert got[0, 1].tolist() == [0, 1031, 1016] and got[1, 1].tolist() == [0, 1024, 1016] and got[2, 0].tolist() == [0, 1023, 1016]
    queries = []
    for edge in (1024, 2048):
        for back in (1, 30, 60):
            for Q in (65, 129, 300):
                queries.append(cases.walk_query(rng, e, edge - back, Q, noise=3, mean_dwell=1.5)[0])
    got = _check(queries, e)
    s = [locate.summarise(b, len(q)) for b, q in zip(got, queries)]
    assert sum(1 for v in s if v["best"][1] // 1024 > v["best"][2] // 1024) >= 12         # the start a tile left of the end


@pytest.mark.parametrize("R,Q", [(17, 2), (1025, 65), (2049, 129)])
def test_ties(built, R, Q):
    """A constant signal on a constant reference: every path costs the same, the tie rule alone decides -- the smallest end of a
    block, and the smallest start: as far left as Q - 1 moves reach."""
    for x, lv in ((7, 7), (7, 3)):
        got = _check([np.full(Q, x, np.int16), np.full(1, x, np.int16)], np.full(R, lv, np.int32))
        for b in range(got.shape[1]):
            assert got[0, b].tolist() == [abs(x - lv) * Q, 1024 * b, max(1024 * b - (Q - 1), 0)] and got[1, b].tolist() == [abs(x - lv), 1024 * b, 1024 * b]


def test_the_32_bit_bound(built):
    """Samples and levels at +-32767 with Q = 16384 on R = 70: the largest cost there is, 16384 x 65534, stays below the kernel's
    2^30, through 256 launches."""
    x = np.full(locate.MAX_QUERY, 32767, np.int16)
    e = np.full(70, -32767, np.int32)
    e[[10, 40]] = B
    e[50:] = 32767
    got = _check([x, (-x).astype(np.int16), x[:16383]], e)
    assert got[0, 0].tolist() == [0, 50, 50] and got[1, 0].tolist() == [0, 0, 0]
    e[50:] = -32767
    got = _check([x], e)
    assert got[0, 0].tolist() == [16384 * 65534, 0, 0] and 16384 * 65534 < 1 << 30


def test_more_units_than_waves(built):
    """More (item, tile) units than a launch has waves, so that waves take a second unit: 4100 queries on two tiles, some of them
    with a second launch."""
    waves = _lib.LOCATE_THREADS // 64 * _lib.LOCATE_MAX_GROUPS
    header = open(os.path.join(ROOT, "include", "chiron_amd.h")).read()
    for name in ("THREADS", "MAX_GROUPS", "CHUNK", "BLOCK"):
        assert int(header.split("#define CHIRON_LOCATE_%s " % name)[1].split()[0]) == getattr(_lib, "LOCATE_" + name)
    rng = np.random.default_rng(6400)
    items = 4100
    assert 2 * items > waves
    e = cases.random_reference(rng, 1030, 0.02)
    lens = np.where(np.arange(items) % 41 == 0, 66, rng.integers(1, 4, items))
    lens[-1] = 65
    _check([cases.random_query(rng, int(Q)) for Q in lens], e)


def test_workspace_contract(built, monkeypatch):
    """"Caller's memory" of include/chiron_amd.h for chiron_signal_locate: under each fill of tests/ws_guard.py the workspace is
    exactly the size function's bytes between two guards and holds the fill on entry, and so does the host output.  The guards are
    intact afterwards, the result equals the reference under all three (which an element left unwritten cannot), and the three
    results are the same bytes.  A workspace said to be one byte short is refused before anything is written."""
    import torch
    rng = np.random.default_rng(6500)
    e = cases.random_reference(rng, 2049 + 600, 0.03)
    e[1000:1100] = B
    queries = [cases.random_query(rng, Q) for Q in (1, 63, 64, 65, 129, 200, 2)]
    queries.append(cases.walk_query(rng, np.where(e == B, 0, e), 1990, 300)[0])
    sample_off = np.concatenate([[0], np.cumsum([len(q) for q in queries])]).astype(np.int64) + 5
    samples = np.ascontiguousarray(np.concatenate([np.zeros(5, np.int16)] + queries))
    items, blocks = len(queries), (len(e) + 1023) // 1024
    need = locate.workspace_size(items, int(sample_off[-1] - sample_off[0]), len(e))
    want = ref.locate(queries, e)
    assert (want[:, 0] == locate.NONE).sum() == 0 and blocks == 3
    results = []
    for fill in FILLS:
        rec = Recorder(fill)
        monkeypatch.setattr(_lib, "alloc_hook", rec)
        try:
            lib, ws, stream = _lib.device_workspace(need, 0, "test", "locate kernel")
            out = np.full((items, blocks, 3), fill * 0x01010101, dtype=np.uint32).view(np.int32)
            before = out.copy()
            st = lib.chiron_signal_locate(0, samples.ctypes.data, sample_off.ctypes.data, items, e.ctypes.data, len(e), out.ctypes.data, ws.data_ptr(), need - 1, 0, stream)
            assert st == _lib.ERR_INVALID and ("a workspace of %d bytes, %d are needed" % (need - 1, need)) in lib.chiron_last_error().decode()
            assert np.array_equal(out, before)
            _lib.check(lib.chiron_signal_locate(0, samples.ctypes.data, sample_off.ctypes.data, items, e.ctypes.data, len(e), out.ctypes.data, ws.data_ptr(), need, 0, stream))
        finally:
            monkeypatch.setattr(_lib, "alloc_hook", None)
        torch.cuda.synchronize()
        rec.check()
        assert rec.sizes == [need]
        assert np.array_equal(out, want), fill
        results.append(out.tobytes())
    assert len(results) == 3 and results[0] == results[1] == results[2]


def test_planted_case_through_the_command(built, tmp_path):
    """The planted case as files -- genome.fa, kmer_levels.tsv, one .signal a read -- through `chiron locate --prefix 1000`, once on
    the GPU and once with locator= set to the reference: located.tsv is the same bytes and the reports are equal.  Where the reads
    land is the reference's business (tests/test_locate_cpu.py); the GPU's bar is equality with it."""
    from chiron_amd import entry, squiggle
    case = cases.planted()
    codes = case["genome"].codes
    (tmp_path / "genome.fa").write_text(">ctg\n%s\n" % "".join("ACGT"[v] for v in codes))
    rows = ["\t".join(squiggle.KMER_COLUMNS) + "\n"]
    for code, lv in enumerate(case["table"].tolist()):
        rows.append("%s\t9\t9.000\t%.5f\t0.10000\n" % ("".join("ACGT"[(code >> (2 * (4 - j))) & 3] for j in range(5)), lv / squiggle.SCALE))
    (tmp_path / "kmer_levels.tsv").write_text("".join(rows))
    assert np.array_equal(squiggle.load_level_table(str(tmp_path / "kmer_levels.tsv"))[1], case["table"])
    (tmp_path / "sig").mkdir()
    for name, raw in case["reads"]:
        (tmp_path / "sig" / (name + ".signal")).write_text(" ".join(str(int(v)) for v in np.rint(raw)))
    argv = ["locate", "-s", str(tmp_path / "sig"), "-g", str(tmp_path / "genome.fa"), "--table", str(tmp_path / "kmer_levels.tsv"), "--prefix",
            str(cases.PREFIX), "--skip", str(cases.SKIP), "--targets", "ctg:1-300"]
    got = entry.main(argv + ["-o", str(tmp_path / "gpu")])
    args = entry.build_parser().parse_args(argv + ["-o", str(tmp_path / "ref")])
    want = locate.locate_command(args, locator=ref.locate)
    assert (tmp_path / "gpu" / "located.tsv").read_bytes() == (tmp_path / "ref" / "located.tsv").read_bytes()
    on_disk = json.loads((tmp_path / "gpu" / "locate_report.json").read_text())
    assert got == want == on_disk == json.loads((tmp_path / "ref" / "locate_report.json").read_text())
    assert got["reads"] == {"total": 30, "used": 30, "dropped": {"too_short": 0, "flat_signal": 0}} and got["status"]["placed"] == 30
    assert got["columns"] == 1201 and got["break_columns"] == 9 and got["batches"] == 1 and 0 < got["on_target"] < 30
    lines = [ln.split("\t") for ln in (tmp_path / "gpu" / "located.tsv").read_text().splitlines()]
    assert tuple(lines[0]) == locate.LOCATED_COLUMNS + ("target",) and len(lines) == 31
    assert sorted(f[0] for f in lines[1:]) == sorted(name for name, _ in case["reads"]) and all(f[2] == "ctg" and f[5] in "+-" for f in lines[1:])
