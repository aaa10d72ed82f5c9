"""chiron_align_overlap on the GPU against tests/overlap_ref.py, exact integer equality everywhere: every form at small shapes, the
four overlap types on both strands, more pairs than workgroups, the LDS boundary of the band, reads shared by many pairs, the
"Caller's memory" contract, and the planted case through the command."""
import json
import os

import numpy as np
import pytest

import assess_ref
import map_ref
import overlap_cases as cases
import overlap_ref as ref
from chiron_amd import _lib, overlap
from ws_guard import FILLS, Recorder

pytestmark = pytest.mark.gpu


def _rows(got):
    return [tuple(int(v) for v in r) for r in got]


def test_every_form_at_small_shapes(built):
    """tests/overlap_cases.small_forms in one call, against the plain recurrence; and each pair of a sample in a call of its own: a
    result does not depend on what else the call holds."""
    reads, pairs = cases.small_forms()
    got = _rows(overlap.align_overlap(reads, pairs))
    want = [ref.recurrence(reads[a], reads[b], dlo, dhi) for a, b, dlo, dhi in pairs.tolist()]
    bad = [(pairs[k].tolist(), got[k], want[k]) for k in range(len(pairs)) if got[k] != want[k]]
    assert len(pairs) > 400 and not bad, (len(bad), bad[:5])
    for k in range(0, len(pairs), 37):
        assert _rows(overlap.align_overlap(reads, pairs[k:k + 1])) == [want[k]]


@pytest.mark.parametrize("kind,strand", cases.TYPED)
def test_the_four_types_on_both_strands(built, kind, strand):
    """tests/overlap_cases.typed_case through find_overlaps on the GPU: the records equal the reference's, and the PAF line is
    what a plain walk over the strings gives."""
    reads, want = cases.typed_case(kind, strand, 900 + cases.TYPED.index((kind, strand)))
    names, result = overlap.find_overlaps(reads, min_overlap=100)
    _, expect = overlap.find_overlaps(reads, min_overlap=100, aligner=cases.reference_aligner)
    assert result == expect and len(result["overlaps"]) == 1
    o = result["overlaps"][0]
    assert (o["type"], o["strand"], o["match"], o["edit"]) == (kind, strand, 300, 0)
    assert tuple(overlap.paf_lines(names, result)[0].split("\t")[:12]) == tuple(str(v) for v in want["paf"])


def test_more_pairs_than_workgroups(built):
    """2048 + 100 tiny pairs, every third a repeat of its predecessor: a workgroup's second pair runs on whatever its first left in
    LDS, and the repeat lands on another workgroup than the pair it repeats."""
    rng = np.random.default_rng(808)
    reads, pairs = [], []
    for k in range(overlap.MAX_GROUPS + 100):
        if k % 3 == 2:
            pairs.append(pairs[-1])
            continue
        n, m = int(rng.integers(0, 13)), int(rng.integers(0, 13))
        reads += [rng.integers(0, 2, n).astype(np.uint8), rng.integers(0, 2, m).astype(np.uint8)]
        dlo = int(rng.integers(-n, m + 1))
        pairs.append((len(reads) - 2, len(reads) - 1, dlo, int(rng.integers(dlo, m + 1))))
    pairs = np.array(pairs, dtype=np.int64)
    got = _rows(overlap.align_overlap(reads, pairs))
    want = [ref.recurrence(reads[a], reads[b], dlo, dhi) for a, b, dlo, dhi in pairs.tolist()]
    bad = [(k, pairs[k].tolist(), got[k], want[k]) for k in range(len(pairs)) if got[k] != want[k]]
    assert not bad, (len(bad), bad[:5])
    assert all(got[k] == got[k - 1] for k in range(2, len(pairs), 3))


def test_band_at_the_lds_boundary(built):
    """Reads of about 2.2 k bases: a band of exactly CHIRON_ALIGN_LDS_SLOTS diagonals stays in LDS, one diagonal more takes the
    workspace row (the size function says so); both in calls of their own and together."""
    rng = np.random.default_rng(4096)
    b = assess_ref.random_seq(2230, rng)
    a = map_ref.mutate_counted(b[700:] + assess_ref.random_seq(700, rng), 0.12, rng)[0]
    reads = [np.array(ref.codes_of(x), dtype=np.uint8) for x in (a, b)]
    n, m, S = len(a), len(b), overlap.LDS_SLOTS
    assert n + m + 1 > S + 1 and -n < -2100 and -2100 + S < m
    pairs = np.array([(0, 1, -2100, -2100 + S - 1), (0, 1, -2100, -2100 + S)], dtype=np.int64)
    assert overlap.workspace_size(2, n + m, 1, S) + ((S + 1) * 8 + 255) // 256 * 256 == overlap.workspace_size(2, n + m, 1, S + 1)
    want = _rows(ref.rows(reads, pairs))
    assert want[0][0] < -700 and want[0][1] > 1100 and want[0][2] >= n and want[0][3] > m      # the planted dovetail, about 1.5 k bases, b then a
    assert _rows(overlap.align_overlap(reads, pairs)) == want
    assert _rows(overlap.align_overlap(reads, pairs[:1])) == want[:1]
    assert _rows(overlap.align_overlap(reads, pairs[1:])) == want[1:]


def test_one_read_shared_by_many_pairs(built):
    """Read 0 against 30 others, as a and as b and against itself, in one call: the read is copied once (the workspace holds the
    31 reads' bases, not the pairs')."""
    rng = np.random.default_rng(31)
    core = assess_ref.random_seq(260, rng)
    reads = [np.array(ref.codes_of(core), dtype=np.uint8)]
    for k in range(30):
        lo = int(rng.integers(0, 150))
        piece = map_ref.mutate_counted(core[lo:lo + 110] + assess_ref.random_seq(int(rng.integers(0, 90)), rng), 0.1, rng)[0]
        reads.append(np.array(ref.codes_of(piece), dtype=np.uint8))
    pairs = [(0, k, -260, 300) for k in range(1, 31)] + [(k, 0, -20 - k, 200) for k in range(1, 31)] + [(0, 0, -5, 5)]
    pairs = np.array(pairs, dtype=np.int64)
    total = sum(len(r) for r in reads)
    assert overlap.workspace_size(31, total, len(pairs), 561) < 61 * 32 + 61 * 20 + total + 4 * 256
    got = _rows(overlap.align_overlap(reads, pairs))
    assert got == _rows(ref.rows(reads, pairs))
    assert got[-1] == (-260, 260, 260, 260)


def test_workspace_contract(built, monkeypatch):
    """"Caller's memory" of include/chiron_amd.h for chiron_align_overlap: under each fill of tests/ws_guard.py the workspace is
    exactly the size function's bytes between two guards and holds the fill on entry, and so does the host output.  The call has
    bands on both sides of the LDS boundary, so the workspace rows are in use.  The guards are intact afterwards, the result equals
    the reference under all three (which an element left unwritten cannot), and the three results are the same bytes.  A workspace
    said to be one byte short is refused before anything is written."""
    import torch
    rng = np.random.default_rng(6500)
    b = assess_ref.random_seq(2300, rng)
    texts = [map_ref.mutate_counted(b[900:], 0.12, rng)[0] + assess_ref.random_seq(900, rng), b,
             map_ref.mutate_counted(b[300:700], 0.1, rng)[0], "", "ACGTNACGT"]
    reads = [np.array(ref.codes_of(x), dtype=np.uint8) for x in texts]
    pairs = np.array([(0, 1, -2200, 2100), (2, 1, 40, 560), (0, 1, -1000, -800), (3, 1, 0, 2300), (4, 3, -9, 0), (4, 4, -1, 1), (2, 0, -400, 2000),
                      (1, 0, 0, 4200)], dtype=np.int64)
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    read_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64) + 3
    codes = np.ascontiguousarray(np.concatenate([np.full(3, 9, np.uint8)] + reads + [np.full(4, 9, np.uint8)]))
    cols = [np.ascontiguousarray(pairs[:, k], dtype=np.int32) for k in range(4)]
    widest = int((np.minimum(pairs[:, 3], lens[pairs[:, 1]]) - np.maximum(pairs[:, 2], -lens[pairs[:, 0]]) + 1).max())
    need = overlap.workspace_size(len(reads), int(lens.sum()), len(pairs), widest)
    want = np.array([list(r) + [0] for r in _rows(ref.rows(reads, pairs))], dtype=np.int32)
    assert widest > overlap.LDS_SLOTS and need > len(pairs) * widest * 8
    results = []
    for fill in FILLS:
        rec = Recorder(fill)
        monkeypatch.setattr(_lib, "alloc_hook", rec)
        try:
            lib, ws, stream = _lib.device_workspace(need, 0, "test", "overlap kernel")
            out = np.full((len(pairs), 5), fill * 0x01010101, dtype=np.uint32).view(np.int32)
            before = out.copy()
            args = (0, codes.ctypes.data, read_off.ctypes.data, len(reads), cols[0].ctypes.data, cols[1].ctypes.data, cols[2].ctypes.data,
                    cols[3].ctypes.data, len(pairs), out.ctypes.data, ws.data_ptr())
            st = lib.chiron_align_overlap(*args, need - 1, 0, stream)
            assert st == _lib.ERR_INVALID and ("a workspace of %d bytes, %d are needed" % (need - 1, need)) in lib.chiron_last_error().decode()
            assert np.array_equal(out, before)
            _lib.check(lib.chiron_align_overlap(*args, need, 0, stream))
        finally:
            monkeypatch.setattr(_lib, "alloc_hook", None)
        torch.cuda.synchronize()
        rec.check()
        assert rec.sizes == [need]
        assert np.array_equal(out, want), fill
        results.append(out.tobytes())
    assert len(results) == 3 and results[0] == results[1] == results[2]


def test_planted_case_through_the_command(built, tmp_path):
    """The planted case of one seed as a FASTQ folder through `chiron overlap`, once on the GPU and once with aligner= set to the
    reference: overlaps.paf and overlap_report.json are the same bytes.  What the overlaps are worth is the reference's business
    (tests/test_overlap_cpu.py); the GPU's bar is equality with it."""
    from chiron_amd import entry
    reads, _ = cases.planted(cases.SEEDS[0])
    src = tmp_path / "reads"
    src.mkdir()
    for name, seq in reads.items():
        (src / (name + ".fastq")).write_text("@%s\n%s\n+\n%s\n" % (name, seq, "I" * len(seq)))
    entry.main(["overlap", "-i", str(src), "-o", str(tmp_path / "gpu")])
    overlap.overlap_command(str(src), str(tmp_path / "ref"), aligner=cases.reference_aligner)
    paf = (tmp_path / "gpu" / "overlaps.paf").read_bytes()
    assert paf == (tmp_path / "ref" / "overlaps.paf").read_bytes() and paf.count(b"\n") > 500
    assert (tmp_path / "gpu" / "overlap_report.json").read_bytes() == (tmp_path / "ref" / "overlap_report.json").read_bytes()
    report = json.loads((tmp_path / "gpu" / "overlap_report.json").read_text())
    assert report["reads"] == 80 and report["kept"]["contained"] > 0 and report["kept"]["contains"] > 0 and os.path.isdir(str(tmp_path / "gpu"))
