"""GPU: what a workgroup of an alignment kernel leaves behind for its next item.  align_kernel (csrc/assess.hip), infix_kernel
(map.hip), trace_kernel (trace.hip), ctc_align_kernel (ctc_align.hip) and pileup_count_kernel (pileup.hip) run item q on
workgroup q mod G; the batches of tests/reuse_cases.py hold 2 G + 40 items, so every workgroup takes a second item and forty a
third, in the designed orders that file lists (workspace row -> LDS, empty -> ordinary -> empty, three doublings -> band0, the
statuses of `label`, the scan state of `pileup`, the longest walk of `trace`).  tests/test_reuse_cases_cpu.py checks that the
items are what they are named.

Per kernel, through the public entry point, all exact (bytes or ints, no tolerance):
    the whole batch equals the reference, item for item;
    a second call returns the same bytes;
    the batch reversed gives the reversed answer (every item changes its workgroup and every tenant order turns round);
    every designed item run alone equals its answer in the batch (for `label` the launch's LDS row is sized by the call's widest
    read, so an item's rows sit in LDS in one call and could sit elsewhere in another).
"""
import numpy as np
import pytest

from chiron_amd import assess, label, map as cmap, pileup

import assess_ref
import reuse_cases

pytestmark = pytest.mark.gpu


def _name_of(c, k):
    return [n for n, at in c["names"].items() if at == k] or "filler"


def test_align_pairs_with_three_tenants_a_workgroup(built):
    c = reuse_cases.case("assess")
    items, want = c["items"], c["want"]
    run = lambda its: assess.align_pairs([a for a, _ in its], [b for _, b in its])
    first = run(items)
    assert len(first) == len(items) > 2 * c["G"]
    for k, ((a, b), (E, M)) in enumerate(zip(items, want)):
        n, m = len(a), len(b)
        row = tuple(int(first[f][k]) for f in ("read_len", "ref_len", "edit", "match", "band"))
        assert row == (n, m, E, M, reuse_cases.assess_band(n, m, E)), (k, _name_of(c, k), row)
        assert tuple(int(first[f][k]) for f in ("mismatch", "insertion", "deletion")) == assess_ref.counts(n, m, E, M), k
        assert first["identity"][k] == (M / (n + m - M - (n + m - 2 * M - E)) if n + m else 0.0), k
    assert run(items).tobytes() == first.tobytes()
    assert run(items[::-1]).tobytes() == first[::-1].tobytes()
    for name, k in c["names"].items():
        assert run([items[k]]).tobytes() == first[k:k + 1].tobytes(), name


def test_align_infix_with_three_tenants_a_workgroup(built):
    c = reuse_cases.case("map")
    items, want, band0 = c["items"], c["want"], c["band0"]
    run = lambda its: cmap.align_infix([a for a, _ in its], [b for _, b in its], band0)
    first = run(items)
    assert first.dtype == want.dtype and len(first) == len(items) > 2 * c["G"]
    for k in range(len(items)):
        assert first[k].tobytes() == want[k].tobytes(), (k, _name_of(c, k), first[k], want[k])
    assert run(items).tobytes() == first.tobytes()
    assert run(items[::-1]).tobytes() == first[::-1].tobytes()
    for name, k in c["names"].items():
        assert run([items[k]]).tobytes() == first[k:k + 1].tobytes(), name


def test_align_ops_with_three_tenants_a_workgroup(built):
    c = reuse_cases.case("trace")
    items, want = c["items"], c["want"]
    run = lambda its: [o.tobytes() for o in assess.align_ops([a for a, _ in its], [b for _, b in its])]
    first = assess.align_ops([a for a, _ in items], [b for _, b in items])
    assert len(first) == len(items) > 2 * c["G"]
    for k, (ops, (E, M, ref_ops)) in enumerate(zip(first, want)):
        assert ops.dtype == np.uint8 and ops.tobytes() == ref_ops.tobytes(), (k, _name_of(c, k), assess.cigar(ops)[:80], assess.cigar(ref_ops)[:80])
    first = [o.tobytes() for o in first]
    assert run(items) == first
    assert run(items[::-1]) == first[::-1]
    for name, k in c["names"].items():
        assert run([items[k]]) == [first[k]], name


def _label_rows(got):
    """Per read, everything label.align returns for it, as bytes and ints."""
    return [(got["start"][k].tobytes(), got["score"][k].tobytes(), int(got["band"][k]), int(got["status"][k])) for k in range(len(got["start"]))]


def test_label_align_with_three_tenants_a_workgroup(built):
    c = reuse_cases.case("label")
    items, want, band0, max_band = c["items"], c["want"], c["band0"], c["max_band"]
    run = lambda its: label.align([x for x, _ in its], [lab for _, lab in its], band0=band0, max_band=max_band)
    got = run(items)
    assert len(got["start"]) == len(items) > 2 * c["G"]
    assert all(s.dtype == np.int32 for s in got["start"]) and got["score"].dtype == np.float64
    first, ref_rows = _label_rows(got), _label_rows(want)
    for k in range(len(items)):
        assert first[k] == ref_rows[k], (k, _name_of(c, k), first[k][1:], ref_rows[k][1:])
    assert got["score"].tobytes() == want["score"].tobytes()
    assert {0, 1, 2} == set(got["status"].tolist())
    again = run(items)
    assert _label_rows(again) == first and again["score"].tobytes() == got["score"].tobytes()
    assert _label_rows(run(items[::-1])) == first[::-1]
    for name, k in c["names"].items():
        assert _label_rows(run([items[k]])) == [first[k]], name


def test_pileup_tile_with_three_tenants_a_workgroup(built):
    c = reuse_cases.case("pileup")
    items, g0, g1, ref, min_depth = c["items"], c["g0"], c["g1"], c["ref"], c["min_depth"]
    planes, depth, call, clipped = c["want"]
    run = lambda its: pileup.pileup_tile(its, g0, g1, ref, min_depth)
    first = run(items)
    assert len(items) > 2 * c["G"] and first[0].dtype == np.int32 and first[0].shape == (pileup.PLANES, g1 - g0)
    assert np.array_equal(first[0], planes), np.argwhere(first[0] != planes)[:5]          # every count plane, not only the calls
    assert np.array_equal(first[1], depth) and np.array_equal(first[2], call) and first[3] == clipped
    for other in (run(items), run(items[::-1])):                                         # counts are sums: the order changes nothing
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first[:3], other[:3])) and other[3] == clipped
    for name, k in c["names"].items():                                                   # alone, an alignment gives its own share
        one = run([items[k]])
        share, clip = c["alone"][name]
        assert np.array_equal(one[0], share) and one[3] == clip, name
        assert np.array_equal(one[1], share[:6].sum(axis=0)), name
