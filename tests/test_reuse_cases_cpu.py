"""CPU: the batches of tests/reuse_cases.py are what tests/test_gpu_reuse.py needs them to be.  Every designed item has the
property its name claims, decided by the reference alone, so that a builder that drifts fails here and does not quietly take the
point out of the GPU test."""
import os
import re

import numpy as np
import pytest

from chiron_amd import _lib, assess

import map_ref
import reuse_cases
import trace_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kernel", sorted(reuse_cases.BUILDERS))
def test_every_workgroup_has_a_second_tenant_and_forty_a_third(kernel):
    c = reuse_cases.case(kernel)
    G, names = c["G"], c["names"]
    assert len(c["items"]) == 2 * G + reuse_cases.EXTRA > 2 * G
    assert G == {"assess": _lib.ALIGN_MAX_GROUPS, "map": _lib.INFIX_MAX_GROUPS, "trace": _lib.ALIGN_MAX_GROUPS,
                 "label": _lib.LABEL_MAX_GROUPS, "pileup": _lib.PILEUP_MAX_GROUPS}[kernel]
    assert all(k % G < reuse_cases.EXTRA for k in names.values())           # designed items sit on workgroups that take a third
    (i, j, k), = c["triplets"]
    assert (j, k) == (i + G, i + 2 * G)
    # the tenants of one sequence share a workgroup, in the order they were given
    by_seq = {}
    for name, at in names.items():
        by_seq.setdefault(name.split(".")[0], []).append(at)
    for seq, at in by_seq.items():
        assert len({a % G for a in at}) == 1 and sorted(at) == at and [a // G for a in at] == list(range(len(at))), seq


def test_the_group_count_of_the_pileup_kernel_is_the_source_s():
    with open(os.path.join(ROOT, "chiron_amd", "csrc", "pileup.hip")) as f:
        text = f.read()
    assert [int(v) for v in re.findall(r"constexpr int MAX_GROUPS = (\d+);", text)] == [_lib.PILEUP_MAX_GROUPS]
    assert "alignments < MAX_GROUPS ? alignments : MAX_GROUPS" in text


def _lens(c):
    return [(len(a), len(b)) for a, b in c["items"]]


def test_assess_items_are_what_their_names_say():
    c = reuse_cases.case("assess")
    names, want, lens = c["names"], c["want"], _lens(c)
    L, band0 = _lib.ALIGN_LDS_SLOTS, _lib.ALIGN_BAND0
    band = [reuse_cases.assess_band(n, m, E) for (n, m), (E, _) in zip(lens, want)]
    slots = [reuse_cases.band_slots(n, m, w) for (n, m), w in zip(lens, band)]
    wide = {names["a.wide"], names["bd.wide_doubling"]}
    assert {k for k, s in enumerate(slots) if s > L} == wide                  # two wide items, no more
    assert slots[names["a.wide"]] == L + 1 and band[names["a.wide"]] == 1024
    assert slots[names["bd.wide_doubling"]] == L + 1
    assert reuse_cases.doublings(band[names["bd.wide_doubling"]], band0) >= 3 and band[names["bd.band0"]] == band0
    for k in (names["a.tiny1"], names["a.tiny2"], names["bd.tiny"]):
        assert slots[k] < 128 and band[k] == band0
    assert c["items"][names["a.tiny1"]] == c["items"][names["a.tiny2"]]
    for tag, empty in (("n0", lambda n, m: n == 0 and m > 0), ("m0", lambda n, m: n > 0 and m == 0), ("both", lambda n, m: n == m == 0)):
        assert empty(*lens[names["c_%s.empty1" % tag]]) and empty(*lens[names["c_%s.empty2" % tag]])
        assert min(lens[names["c_%s.ordinary" % tag]]) >= 8
    i, j, k = c["triplets"][0]
    assert c["items"][i] == c["items"][j] == c["items"][k] and want[i] == want[j] == want[k] and min(lens[i]) >= 8
    filler = [k for k in range(len(lens)) if k not in names.values()]
    assert all(8 <= n <= 48 and 8 <= m <= 48 for n, m in (lens[k] for k in filler))
    related = sum(want[k][0] < min(lens[k]) // 2 for k in filler)
    assert related > len(filler) // 3 and len(filler) - related > len(filler) // 8


def test_map_items_are_what_their_names_say():
    c = reuse_cases.case("map")
    names, want, lens, band0 = c["names"], c["want"], _lens(c), c["band0"]
    L = _lib.INFIX_LDS_SLOTS
    assert band0 == _lib.INFIX_BAND0
    band = [map_ref.expected_band(n, m, int(E), band0) for (n, m), E in zip(lens, want["edit"])]
    assert band == want["band"].tolist()
    slots = [reuse_cases.band_slots(n, m, w) for (n, m), w in zip(lens, band)]
    assert {k for k, s in enumerate(slots) if s > L} == {names["a.wide"], names["b.wide"]}
    assert slots[names["a.wide"]] == slots[names["b.wide"]] == L + 1
    assert reuse_cases.doublings(band[names["d.doubling"]], band0) >= 3 and slots[names["d.doubling"]] <= L
    assert band[names["d.band0"]] == band0
    for k in (names["a.tiny1"], names["a.tiny2"], names["b.tiny"]):
        assert slots[k] < 128 and band[k] == band0
    assert c["items"][names["a.tiny1"]] == c["items"][names["a.tiny2"]]
    for tag, empty in (("n0", lambda n, m: n == 0 and m > 0), ("m0", lambda n, m: n > 0 and m == 0), ("both", lambda n, m: n == m == 0)):
        assert empty(*lens[names["c_%s.empty1" % tag]]) and empty(*lens[names["c_%s.empty2" % tag]])
        assert min(lens[names["c_%s.ordinary" % tag]]) >= 8
    i, j, k = c["triplets"][0]
    assert c["items"][i] == c["items"][j] == c["items"][k] and want[i] == want[j] == want[k] and min(lens[i]) >= 8
    filler = [k for k in range(len(lens)) if k not in names.values()]
    assert all(8 <= n <= 48 and 8 <= m <= 48 for n, m in (lens[k] for k in filler))
    assert 0 < sum(int(want["edit"][k]) == 0 for k in filler) < len(filler) // 2


def test_trace_items_are_what_their_names_say(built):
    c = reuse_cases.case("trace")
    names, want, lens = c["names"], c["want"], _lens(c)
    L = _lib.ALIGN_LDS_SLOTS
    slots = [reuse_cases.band_slots(n, m, trace_ref.tight_band(n, m, E)) for (n, m), (E, _, _) in zip(lens, want)]
    assert {k for k, s in enumerate(slots) if s > L} == {names["a.wide"], names["b.wide"]}
    assert slots[names["a.wide"]] == slots[names["b.wide"]] == L + 1
    assert lens[names["a.wide"]][0] > lens[names["a.wide"]][1] and lens[names["b.wide"]][0] < lens[names["b.wide"]][1]
    for k in (names["a.tiny1"], names["a.tiny2"], names["b.tiny"]):
        assert slots[k] < 128
    assert c["items"][names["a.tiny1"]] == c["items"][names["a.tiny2"]]
    columns = [len(ops) for _, _, ops in want]
    assert columns[names["g.longest"]] == max(columns) > 4200 and columns.count(max(columns)) == 1
    assert slots[names["g.odd"]] % 2 == 1 and slots[names["g.odd"]] > 1 and slots[names["g.longest"]] <= L
    for tag, empty in (("n0", lambda n, m: n == 0 and m > 0), ("m0", lambda n, m: n > 0 and m == 0), ("both", lambda n, m: n == m == 0)):
        assert empty(*lens[names["c_%s.empty1" % tag]]) and empty(*lens[names["c_%s.empty2" % tag]])
        assert min(lens[names["c_%s.ordinary" % tag]]) >= 8
    i, j, k = c["triplets"][0]
    assert c["items"][i] == c["items"][j] == c["items"][k] and min(lens[i]) >= 8
    assert want[i][:2] == want[j][:2] == want[k][:2] and want[i][2].tobytes() == want[j][2].tobytes() == want[k][2].tobytes()
    filler = [k for k in range(len(lens)) if k not in names.values()]
    assert all(8 <= n <= 48 and 8 <= m <= 48 for n, m in (lens[k] for k in filler))
    # align_ops traces the batch in one launch: the plan (host-only) does not split it at the default budget
    plan = assess.plan_trace_batches([n for n, _ in lens], [m for _, m in lens], [E for E, _, _ in want], 4096 << 20)
    assert len(plan) == 1 and plan[0][0] == list(range(len(lens)))


def test_label_items_are_what_their_names_say():
    c = reuse_cases.case("label")
    names, want, band0, max_band = c["names"], c["want"], c["band0"], c["max_band"]
    L = _lib.LABEL_LDS_SLOTS
    shape = [(x.shape[0], len(lab)) for x, lab in c["items"]]
    status, band = want["status"].tolist(), want["band"].tolist()
    width = [reuse_cases.label_width(nb, w) for (_, nb), w in zip(shape, band)]
    ran = [k for k in range(len(shape)) if status[k] != 1 and shape[k][0] > 0]          # the reads that ran a pass
    assert {k for k in ran if width[k] > L} == {names["a.wide"], names["b.wide_status2"]}
    assert width[names["a.wide"]] == width[names["b.wide_status2"]] == L + 1
    assert status[names["a.wide"]] == 0 and band[names["a.wide"]] == 2048 and names["a.wide"] < c["G"]     # a first tenant
    assert status[names["b.wide_status2"]] == 2 and band[names["b.wide_status2"]] == max_band == 2048
    assert status[names["e.status1"]] == 1 and status[names["e.ordinary"]] == 0
    rep = lambda lab: int(np.count_nonzero(lab[1:] == lab[:-1]))
    x, lab = c["items"][names["e.status1"]]
    assert x.shape[0] < len(lab) + rep(lab)
    assert reuse_cases.doublings(band[names["d.doubling"]], band0) >= 3 and status[names["d.doubling"]] == 0
    assert band[names["d.band0"]] == band0 and status[names["d.band0"]] == 0
    assert reuse_cases.label_width(shape[names["d.band0"]][1], band0) < 2 * shape[names["d.band0"]][1] + 1     # a clipped band, not the table
    for k in (names["a.tiny1"], names["a.tiny2"], names["b.tiny"]):
        assert width[k] <= 25
    a, b = c["items"][names["a.tiny1"]], c["items"][names["a.tiny2"]]
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and status[names["a.tiny1"]] == 0
    assert shape[names["c_f0.empty1"]] == shape[names["c_f0.empty2"]] == (0, 0)
    assert shape[names["c_f1.empty1"]] == shape[names["c_f1.empty2"]] == (1, 0)
    ordinary = [names[n] for n in ("b.ordinary", "c_f0.ordinary", "c_f1.ordinary", "e.ordinary", "h.first")]
    assert all(36 <= shape[k][1] <= 44 and status[k] == 0 for k in ordinary)
    i, j, k = c["triplets"][0]
    assert all(c["items"][i][t].tobytes() == c["items"][j][t].tobytes() == c["items"][k][t].tobytes() for t in (0, 1))
    assert want["score"][i].tobytes() == want["score"][j].tobytes() == want["score"][k].tobytes() and band[i] == band[j] == band[k]
    assert np.array_equal(want["start"][i], want["start"][j]) and np.array_equal(want["start"][i], want["start"][k])
    filler = [k for k in range(len(shape)) if k not in names.values()]
    assert all(nb <= 12 and F <= 6 * nb for F, nb in (shape[k] for k in filler))
    assert {status[k] for k in filler} == {0, 1} and len({band[k] for k in filler}) >= 3


def test_pileup_items_are_what_their_names_say():
    c = reuse_cases.case("pileup")
    names, items, g0, g1 = c["names"], c["items"], c["g0"], c["g1"]
    chunk = _lib.PILEUP_CHUNK
    planes, depth, call, clipped = c["want"]
    assert planes.shape == (_lib.PILEUP_PLANES, g1 - g0) and planes.any(axis=1).all()       # every plane is exercised
    m_of = lambda ops: int((np.asarray(ops) != 2).sum())
    touches = lambda pos, ops: m_of(ops) > 0 and pos < g1 and pos > g0 - m_of(ops)          # the host's rule for ncols != 0
    for tag in ("before", "after", "noref"):
        for role in ("ncols0_1", "ncols0_2"):
            pos, _, ops = items[names["c_%s.%s" % (tag, role)]]
            assert len(ops) > 0 and not touches(pos, ops)
            assert not c["alone"]["c_%s.%s" % (tag, role)][0].any()
        pos, _, ops = items[names["c_%s.ordinary" % tag]]
        assert touches(pos, ops) and c["alone"]["c_%s.ordinary" % tag][0].any()
    assert c["alone"]["c_noref.ncols0_1"][1] == 9 and m_of(items[names["c_noref.ncols0_1"]][2]) == 0
    pos, _, ops = items[names["f_long.columns3073"]]
    assert len(ops) == 3 * chunk + 1 == 3073 and g0 <= pos and pos + m_of(ops) <= g1        # wholly inside: no chunk is skipped
    pos, _, ops = items[names["f_long.leading_insertion"]]
    assert ops[0] == 2 and len(ops) < 60 and (ops[1:-1] == 2).any() and g0 <= pos and pos + m_of(ops) <= g1
    pos, _, ops = items[names["f_break.leaves_early"]]
    q_at_chunk2 = int((ops[:chunk] != 2).sum())
    assert touches(pos, ops) and len(ops) > 2 * chunk and pos - g0 + q_at_chunk2 - 1 >= g1 - g0    # the break's condition at base = chunk
    pos, _, ops = items[names["f_break.inside"]]
    assert g0 <= pos and pos + m_of(ops) <= g1 and 0 < len(ops) <= 60
    i, j, k = c["triplets"][0]
    assert all(np.array_equal(items[i][t], items[j][t]) and np.array_equal(items[i][t], items[k][t]) for t in (0, 1, 2))
    assert all(np.array_equal(c["alone"]["h.first"][0], c["alone"][n][0]) for n in ("h.second", "h.third")) and c["alone"]["h.first"][0].any()
    filler = [k for k in range(len(items)) if k not in names.values()]
    assert all(len(items[k][2]) <= 60 for k in filler)
    assert sum(not touches(items[k][0], items[k][2]) for k in filler) >= 5 and clipped > 100
