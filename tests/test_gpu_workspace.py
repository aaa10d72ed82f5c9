"""GPU: the memory contract of the twelve calls that compute in memory their caller hands them (include/chiron_amd.h, "Caller's
memory"): workspace, tape and output buffers may hold anything on entry, every output element is written, and nothing outside
the bytes the call's size function names is touched.

Each call runs its case once per fill byte of tests/ws_guard.py (0x00, 0xFF, 0x7F) with a Recorder on chiron_amd._lib.alloc_hook:
every tape, workspace and device output of the call is then exactly sized, poisoned, and (the byte buffers) fenced by 1 MiB
guards.  Asserted per call:
    reference     the result under the existing reference and rule of the call's own GPU test (no tolerance is new here);
    invariance    the three fills give the same bytes in every output;
    completeness  no element of a device output still holds the fill pattern (under 0xFF: no NaN anywhere);
    bounds        both guards of every buffer are intact after the stream is synchronised;
    sizes         every byte count the wrapper asked for is what the call's host-only size function gives for that run.
The cases are the smallest that reach every workspace region of their call, built from the case modules of the suite.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from chiron_amd import _lib, assess, ctc, demux, label, map as cmap, pileup, polish, train

import cnn_train_cases as cc
import ctc_align_ref
import ctc_ref
import demux_cases
import demux_ref
import pileup_cases
import pileup_ref
import polish_cases
import polish_ref
import reuse_cases
import seed_ref
import train_cases as tc
import trace_ref
import assess_ref
from ws_guard import FILLS, Recorder, still_filled

pytestmark = pytest.mark.gpu


def one_fill(monkeypatch, fill, run):
    """run() with a Recorder of that fill as the allocation hook; then the stream is synchronised, the guards are checked and no
    device output may keep the pattern.  -> (fill, byte counts asked for, what run returned); the blocks are dropped."""
    rec = Recorder(fill)
    monkeypatch.setattr(_lib, "alloc_hook", rec)
    try:
        res = run()
    finally:
        monkeypatch.setattr(_lib, "alloc_hook", None)
    torch.cuda.synchronize()
    rec.check()
    for k, t in enumerate(rec.outputs):
        if fill:                                  # a zero is a legitimate result; under the other two fills nothing may keep the pattern
            assert still_filled(t, fill) == 0, "output %d %s: %d elements still hold 0x%02X" % (k, tuple(t.shape), still_filled(t, fill), fill)
        if fill == 0xFF:
            assert not bool(torch.isnan(t).any()), "output %d %s holds a NaN" % (k, tuple(t.shape))
    return fill, rec.sizes, res


def per_fill(monkeypatch, run):
    """one_fill for each of the three fills, in turn."""
    return [one_fill(monkeypatch, fill, run) for fill in FILLS]


def same_bytes(runs, as_bytes):
    first = as_bytes(runs[0][2])
    for fill, _, res in runs[1:]:
        assert as_bytes(res) == first, "the result under 0x%02X differs from the one under 0x%02X" % (fill, runs[0][0])


def selection(c):
    """The designed items of a reuse_cases batch, in batch order, then G + 1 of its fillers: more items than workgroups, so the
    workgroups of the designed items take a filler after them.  -> (items, their indices in c["items"])"""
    named = sorted(set(c["names"].values()))
    idx = named + [i for i in range(len(c["items"])) if i not in set(named)][:c["G"] + 1]
    assert len(idx) == len(named) + c["G"] + 1
    return [c["items"][i] for i in idx], idx


# ------------------------------------------------------------------------------------------------------------------------------
# the alignment kernels
# ------------------------------------------------------------------------------------------------------------------------------
def test_align_pairs(built, monkeypatch):
    c = reuse_cases.case("assess")
    items, idx = selection(c)
    for name in ("a.wide", "a.tiny1", "c_both.empty1", "bd.wide_doubling"):         # a workspace row, LDS, empty, three doublings
        assert c["names"][name] in idx
    runs = per_fill(monkeypatch, lambda: assess.align_pairs([a for a, _ in items], [b for _, b in items]))
    max_len = max(max(len(a), len(b)) for a, b in items)
    assert max_len > _lib.ALIGN_LDS_SLOTS // 2
    for _, sizes, _ in runs:
        assert sizes == [assess.workspace_size(len(items), max_len)]
    got = runs[0][2]
    for k, i in enumerate(idx):
        (a, b), (E, M) = c["items"][i], c["want"][i]
        n, m = len(a), len(b)
        row = tuple(int(got[f][k]) for f in ("read_len", "ref_len", "edit", "match", "band"))
        assert row == (n, m, E, M, reuse_cases.assess_band(n, m, E)), (k, i, row)
    assert reuse_cases.doublings(int(got["band"][idx.index(c["names"]["bd.wide_doubling"])]), _lib.ALIGN_BAND0) >= 3
    same_bytes(runs, lambda r: r.tobytes())


def test_align_infix(built, monkeypatch):
    c = reuse_cases.case("map")
    items, idx = selection(c)
    runs = per_fill(monkeypatch, lambda: cmap.align_infix([a for a, _ in items], [b for _, b in items], c["band0"]))
    for _, sizes, _ in runs:
        assert sizes == [cmap.workspace_size(len(items), max(len(a) for a, _ in items), max(len(b) for _, b in items))]
    got = runs[0][2]
    assert got.dtype == c["want"].dtype
    for k, i in enumerate(idx):
        assert got[k].tobytes() == c["want"][i].tobytes(), (k, i, got[k], c["want"][i])
    same_bytes(runs, lambda r: r.tobytes())


def _trace_sizes(items, want, budget):
    """What align_ops asks for: the workspace of align_pairs, then one per planned run, each recomputed from the run's own pairs."""
    lens = [(len(a), len(b)) for a, b in items]
    sizes = [assess.workspace_size(len(items), max(max(n, m) for n, m in lens))]
    plan = assess.plan_trace_batches([n for n, _ in lens], [m for _, m in lens], [E for E, _, _ in want], budget)
    for batch, nbytes in plan:
        per = [assess.trace_pair_size(lens[i][0], lens[i][1], want[i][0]) for i in batch]
        own = assess.trace_workspace_size(len(batch), sum(p[0] for p in per), max(max(lens[i]) for i in batch), max(p[1] for p in per))
        assert own == nbytes
        sizes.append(own)
    return sizes, plan


@pytest.mark.parametrize("workspace_mb", [4096, 1])
def test_align_trace(built, monkeypatch, workspace_mb):
    """One run, and a budget of 1 MiB, which the back-pointers of either wide pair alone exceed: several runs."""
    c = reuse_cases.case("trace")
    items, idx = selection(c)
    want = [c["want"][i] for i in idx]
    odd = items[idx.index(c["names"]["g.odd"])]
    assert assess.trace_pair_size(len(odd[0]), len(odd[1]), 2)[1] == 3 and c["names"]["g.longest"] in idx      # an odd band: half a row of pad
    runs = per_fill(monkeypatch, lambda: assess.align_ops([a for a, _ in items], [b for _, b in items], workspace_mb=workspace_mb))
    sizes, plan = _trace_sizes(items, want, workspace_mb << 20)
    assert len(plan) == 1 if workspace_mb == 4096 else len(plan) >= 2
    for _, asked, _ in runs:
        assert asked == sizes
    for k, (ops, (E, M, ref_ops)) in enumerate(zip(runs[0][2], want)):
        assert ops.dtype == np.uint8 and ops.tobytes() == ref_ops.tobytes(), (k, idx[k])
    same_bytes(runs, lambda r: [o.tobytes() for o in r])


def test_align_trace_leaves_a_failed_pair_untouched(built, monkeypatch):
    """The raw call with E one too large and M one too small for pairs 1 and 3 (tests/test_gpu_trace.py): status 1, their slices of
    ops_out untouched under every fill, the other pairs traced."""
    rng = np.random.default_rng(6)
    reads = [assess_ref.random_seq(n, rng) for n in (200, 310, 150, 420, 90)]
    refs = [assess_ref.mutate(r, 0.15, rng) for r in reads]
    want = [trace_ref.full_trace(a, b) for a, b in zip(reads, refs)]
    edit = np.array([E for E, _, _ in want], dtype=np.int32)
    match = np.array([M for _, M, _ in want], dtype=np.int32)
    for bad in (1, 3):
        edit[bad] += 1
        match[bad] -= 1
    codes, la, lb, read_off, ref_off = _lib.pack_pairs([assess.encode(s) for s in reads], [assess.encode(s) for s in refs])
    ops_off = np.concatenate([[0], np.cumsum(edit.astype(np.int64) + match)]).astype(np.int64)
    per = [assess.trace_pair_size(int(n), int(m), int(e)) for n, m, e in zip(la, lb, edit)]
    nbytes = assess.trace_workspace_size(5, sum(p[0] for p in per), int(max(la.max(), lb.max())), max(p[1] for p in per))

    def run():
        ops = np.full(int(ops_off[-1]), 7, dtype=np.uint8)
        status = np.full(5, -1, dtype=np.int32)
        lib, ws, stream = _lib.device_workspace(nbytes, 0, "test", "traceback")
        _lib.check(lib.chiron_align_trace(0, codes.ctypes.data, read_off.ctypes.data, ref_off.ctypes.data, 5, edit.ctypes.data, match.ctypes.data,
                                          ops_off.ctypes.data, 0, ops.ctypes.data, status.ctypes.data, ws.data_ptr(), stream))
        return ops, status

    runs = per_fill(monkeypatch, run)
    for _, sizes, (ops, status) in runs:
        assert sizes == [nbytes] and status.tolist() == [0, 1, 0, 1, 0]
        for k in range(5):
            piece = ops[ops_off[k]:ops_off[k + 1]]
            assert np.all(piece == 7) if k in (1, 3) else piece.tobytes() == want[k][2].tobytes(), k


_LABEL_WANT = {}


def _label_rows(got):
    return [(got["start"][k].tobytes(), got["score"][k].tobytes(), int(got["band"][k]), int(got["status"][k])) for k in range(len(got["start"]))]


@pytest.mark.parametrize("band0", [0, 8])
def test_ctc_align(built, monkeypatch, band0):
    """band0 = 8 doubles to the 4097 states of the wide read (rows in the workspace) and exhausts max_band on the status-2 read;
    band0 = 0 runs every read's full table, the wide reads' in the workspace."""
    c = reuse_cases.case("label")
    items, idx = selection(c)
    xs, labs, max_band = [x for x, _ in items], [lab for _, lab in items], c["max_band"]
    if band0 not in _LABEL_WANT:
        _LABEL_WANT[band0] = ctc_align_ref.align(xs, labs, band0, max_band)
    want = _LABEL_WANT[band0]
    assert set(want["status"].tolist()) == ({0, 1, 2} if band0 else {0, 1})
    widths = [reuse_cases.label_width(len(lab), int(b)) for lab, b in zip(labs, want["band"])]
    assert max(widths) > _lib.LABEL_LDS_SLOTS and min(widths) < 8
    runs = per_fill(monkeypatch, lambda: label.align(xs, labs, band0=band0, max_band=max_band))
    for _, sizes, _ in runs:
        assert sizes == [label.workspace_size([len(x) for x in xs], [len(lab) for lab in labs], band0, max_band)]
    got, ref_rows = _label_rows(runs[0][2]), _label_rows(want)
    for k in range(len(items)):
        assert got[k] == ref_rows[k], (k, idx[k], got[k][1:], ref_rows[k][1:])
    same_bytes(runs, _label_rows)


# ------------------------------------------------------------------------------------------------------------------------------
# pileup
# ------------------------------------------------------------------------------------------------------------------------------
def test_pileup_tile(built, monkeypatch):
    c = reuse_cases.case("pileup")
    g0, g1, ref, min_depth = c["g0"], c["g1"], c["ref"], c["min_depth"]
    items = [c["items"][c["names"][n]] for n in ("f_long.columns3073", "f_long.leading_insertion", "f_break.leaves_early", "f_break.inside")]
    assert len(items[0][2]) == 3 * _lib.PILEUP_CHUNK + 1 and items[1][2][0] == 2
    planes, depth, call, clipped = pileup_ref.counter(items, g0, g1, ref, min_depth)
    runs = per_fill(monkeypatch, lambda: pileup.pileup_tile(items, g0, g1, ref, min_depth))
    for _, sizes, _ in runs:
        assert sizes == [pileup.workspace_size(len(items), sum(len(a[1]) for a in items), sum(len(a[2]) for a in items), g1 - g0)]
    got = runs[0][2]
    assert np.array_equal(got[0], planes), np.argwhere(got[0] != planes)[:5]
    assert np.array_equal(got[1], depth) and np.array_equal(got[2], call) and got[3] == clipped
    same_bytes(runs, lambda r: (r[0].tobytes(), r[1].tobytes(), r[2].tobytes(), r[3]))


def test_pileup_count_over_three_tiles(built, monkeypatch):
    rng = np.random.default_rng(2718)
    total = 700
    alns = pileup_cases.random_set(rng, 150, total)
    ref = rng.integers(0, 5, total).astype(np.uint8)
    genome = cmap.Genome([("c", "".join("ACGTN"[v] for v in ref))])
    planes, clipped = pileup_ref.count_columns(alns, 0, total)
    depth, call = pileup_ref.call_tile(planes, ref, 3)
    budget = pileup.plan_tiles(alns, total, 1 << 40)[0][3] * 2 // 5
    plan = pileup.plan_tiles(alns, total, budget)
    assert len(plan) >= 3
    runs = per_fill(monkeypatch, lambda: pileup.count(alns, genome, min_depth=3, workspace_mb=budget / (1 << 20), want_counts=True))
    for _, sizes, _ in runs:                      # one workspace a tile; the closing empty tile asks for none
        assert len(sizes) == len(plan)
        for nbytes, (g0, g1, sel, planned) in zip(sizes, plan):
            assert nbytes == planned == pileup.workspace_size(len(sel), sum(len(alns[i][1]) for i in sel), sum(len(alns[i][2]) for i in sel), g1 - g0)
    got = runs[0][2]
    assert np.array_equal(got["counts"], planes) and np.array_equal(got["depth"], depth) and np.array_equal(got["call"], call)
    assert got["clipped"] == clipped and got["over_total"] == int(planes[pileup_ref.OVER].sum())
    same_bytes(runs, lambda r: (r["counts"].tobytes(), r["depth"].tobytes(), r["call"].tobytes(), r["clipped"], r["over_total"]))


# ------------------------------------------------------------------------------------------------------------------------------
# seeding
# ------------------------------------------------------------------------------------------------------------------------------
def _seed_size(index, reads):
    lens = [len(r) for r in reads]
    return cmap.seed_workspace_size(len(index[0]), int(index[1].max()) + cmap.K, len(reads), max(lens), sum(lens))


@pytest.mark.parametrize("name", ["bin_boundaries", "repeats_occ64", "second_copy_far"])
def test_seed_votes_hand_cases(built, monkeypatch, name):
    index, reads = seed_ref.hand_cases()[0][name]
    want = [cmap.vote(index, r) for r in reads]
    runs = per_fill(monkeypatch, lambda: cmap.vote_reads(index, reads))
    for _, sizes, got in runs:
        assert sizes == [_seed_size(index, reads)]
        assert got == want
    if name == "second_copy_far":
        assert [v["votes_second"] for v in runs[0][2]] == [286, 286]


def test_seed_votes_a_second_read_after_a_long_one(built, monkeypatch):
    """The 131072-base read first, MAX_GROUPS - 1 short ones, then 400 bases out of the long read: read r runs on workgroup r mod
    MAX_GROUPS, so the last read is the second tenant of the long read's workgroup, with kc rows sized by the long read and its
    hits in bins the long read counted in: a counter left behind would be a vote too many."""
    G = _lib.SEED_MAX_GROUPS
    index, long, short = seed_ref.mixed_batch(G - 1)
    reads = [long] + short + [long[:400].copy()]
    assert len(reads) == G + 1 and len(long) == _lib.INFIX_MAX_READ
    want = [cmap.vote(index, r) for r in reads]
    assert want[0]["votes"] > 0 and want[-1]["votes"] > 0 and want[-1]["strand"] == want[0]["strand"]
    assert want[-1]["delta"] // cmap.BIN == want[0]["delta"] // cmap.BIN              # the same bin
    mb = _seed_size(index, reads) // (1 << 20) + 1
    runs = per_fill(monkeypatch, lambda: cmap.vote_reads(index, reads, workspace_mb=mb))
    for _, sizes, got in runs:
        assert sizes == [_seed_size(index, reads)]
        assert got == want


# ------------------------------------------------------------------------------------------------------------------------------
# polish: chiron_ctc_score
# ------------------------------------------------------------------------------------------------------------------------------
def _score_case():
    """The items of test_gpu_polish.py's test_lane_and_state_boundaries (without and with repeats) at L in 1, 2, 32, 63, 127, then
    an item of no frames and an item without a candidate, in frame order."""
    from test_gpu_polish import _codes, _no_repeats, _with_repeats
    parts, items, cands, at = [], [], [], 0
    for repeats in (False, True):
        rng = np.random.default_rng(311 + repeats)
        for L in (1, 2, 32, 63, 127):
            lab = _with_repeats(rng, L) if repeats else _no_repeats(rng, L)
            rep = int(np.count_nonzero(lab[1:] == lab[:-1]))
            other = lab.copy()
            other[L // 2] = (other[L // 2] + 1) % 4
            for T in (L + rep, 3 * L):
                x = polish_cases.planted(rng, lab, dwell_p=0.5)[:T] if T > L + rep else rng.normal(0, 2, (T, 5)).astype(np.float32)
                x = np.concatenate([x, rng.normal(0, 2, (T - len(x), 5)).astype(np.float32)])
                parts.append(x)
                items.append((at, at + T))
                cands.append([lab, other, lab[:-1], np.concatenate([lab, lab[:1]])[:polish.MAX_LABEL]])
                at += T
    items.append((at, at))
    cands.append([_codes(""), _codes("A")])                  # T = 0: 0.0, and infeasible
    items.append((at - 20, at))
    cands.append([])                                         # no candidate
    return np.concatenate(parts), items, cands


def _score_sizes(items, cands, budget):
    plan = polish.plan_batches(items, cands, budget)
    sizes = []
    for first, last, lo, hi in plan:
        labs = [l for ls in cands[first:last] for l in ls]
        if labs:                                             # a run without a candidate launches nothing and asks for nothing
            sizes.append(polish.workspace_size(hi - lo, last - first, len(labs), sum(len(l) for l in labs)))
    return sizes, plan


@pytest.mark.parametrize("runs_wanted", [1, 3])
def test_ctc_score(built, monkeypatch, runs_wanted):
    from test_gpu_polish import _close
    x, items, cands = _score_case()
    want = polish_ref.score(x, items, cands)
    labs = [l for ls in cands for l in ls]
    whole = polish.workspace_size(len(x), len(items), len(labs), sum(len(l) for l in labs))
    budget = (4096 << 20) if runs_wanted == 1 else whole * 10 // 32
    sizes, plan = _score_sizes(items, cands, budget)
    assert len(plan) == 1 if runs_wanted == 1 else len(plan) >= 3
    runs = per_fill(monkeypatch, lambda: polish.score(x, items, cands, workspace_mb=budget / (1 << 20)))
    for _, asked, _ in runs:
        assert asked == sizes and len(asked) >= runs_wanted
    got = runs[0][2]
    assert len(got["loglik"]) == len(got["status"]) == len(items)
    for i, (gl, gs, wl, ws) in enumerate(zip(got["loglik"], got["status"], want["loglik"], want["status"])):
        assert gl.dtype == np.float64 and gs.dtype == np.int32 and len(gl) == len(gs) == len(cands[i])
        assert np.array_equal(gs, ws), (i, gs, ws)
        for k in range(len(gl)):
            assert _close(gl[k], wl[k]), (i, k, items[i], gl[k], wl[k])
    assert got["loglik"][-2].tolist() == [0.0, -np.inf] and got["status"][-2].tolist() == [0, 1] and got["loglik"][-1].shape == (0,)
    same_bytes(runs, lambda r: ([a.tobytes() for a in r["loglik"]], [a.tobytes() for a in r["status"]]))


# ------------------------------------------------------------------------------------------------------------------------------
# demux
# ------------------------------------------------------------------------------------------------------------------------------
_DEMUX_KEYS = ("best", "dist", "end", "second")


def _demux(monkeypatch, windows, patterns, groups, want_matrix):
    want = demux_ref.match(windows, patterns, groups, want_matrix=want_matrix)
    runs = per_fill(monkeypatch, lambda: demux.match_call(windows, patterns, groups, want_matrix=want_matrix))
    keys = _DEMUX_KEYS + (("pair_dist", "pair_end") if want_matrix else ())
    for _, sizes, got in runs:
        assert sizes == [demux.workspace_size(len(windows), sum(len(w) for w in windows), len(patterns), want_matrix)]
        assert set(got) == set(keys)
    got = runs[0][2]
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, (k, len(patterns), bad[:5].tolist())
    same_bytes(runs, lambda r: [r[k].tobytes() for k in keys])


def test_demux_edge_case(built, monkeypatch):
    windows, patterns, groups = demux_cases.edge_case()
    _demux(monkeypatch, windows, patterns, groups, True)


@pytest.mark.parametrize("want_matrix", [True, False])
@pytest.mark.parametrize("patterns", [70, 3])
def test_demux_lane_maps(built, monkeypatch, patterns, want_matrix):
    """37 windows of 0 .. 40 bases, lengths 0, 7, 8 and 9 among them (the 8-byte pad of a packed window); 70 patterns are two rounds
    a lane with one window slot a wave, 3 patterns 16 slots a wave with the last wave half empty."""
    rng = np.random.default_rng(700 + patterns)
    pats = [demux_cases.random_codes(int(rng.integers(1, 25)), rng, with_n=q % 7 == 3) for q in range(patterns)]
    groups = rng.integers(0, max(patterns // 2, 1) + 1, patterns).astype(np.int32)
    lens = [0, 7, 8, 9] + [int(rng.integers(0, 41)) for _ in range(33)]
    windows = [demux_cases.random_codes(n, rng, with_n=w % 5 == 2) for w, n in enumerate(lens)]
    for w in range(0, 37, 3):
        p = pats[int(rng.integers(0, patterns))]
        if len(windows[w]) >= len(p):
            at = int(rng.integers(0, len(windows[w]) - len(p) + 1))
            windows[w][at:at + len(p)] = p
    assert len(windows) == 37 and {0, 7, 8, 9} <= {len(w) for w in windows}
    _demux(monkeypatch, windows, pats, groups, want_matrix)


# ------------------------------------------------------------------------------------------------------------------------------
# CTC loss and gradient
# ------------------------------------------------------------------------------------------------------------------------------
def _ctc(monkeypatch, logits, seq_len, labels, label_len):
    from test_gpu_ctc import _check_loss, _torch_grad
    B, T, _ = logits.shape
    runs = per_fill(monkeypatch, lambda: ctc.ctc_loss(logits, seq_len, labels, label_len, want_grad=True))
    for _, sizes, _ in runs:
        assert sizes == [_lib.sized("chiron_ctc_workspace_size", B, T, labels.shape[1], _lib.CTC_WANT_GRAD)]
    loss, grad = runs[0][2]
    status = ctc.row_status(seq_len, labels, label_len)
    ok = np.nonzero(status == ctc.STATUS_SCORED)[0]
    tl, tg = _torch_grad(logits[ok], seq_len[ok], labels[ok], label_len[ok])
    want = np.where(status == ctc.STATUS_INFEASIBLE, np.inf, 0.0)
    want[ok] = tl
    _check_loss(loss, want)
    assert np.abs(grad[ok] - tg).max() <= 1e-5, np.abs(grad[ok] - tg).max()
    for b in range(B):
        assert not grad[b, seq_len[b]:].any(), b                      # frames past seq_len: exactly 0
        if status[b] != ctc.STATUS_SCORED:
            assert not grad[b].any() and loss[b] == want[b], b        # skipped: 0, infeasible: +inf, a zero gradient for both
    same_bytes(runs, lambda r: (r[0].tobytes(), r[1].tobytes()))
    return loss, status


def test_ctc_loss_every_kind_of_row(built, monkeypatch):
    rng = np.random.default_rng(65)
    B, T, Lmax = 5, 65, 20
    logits = rng.normal(scale=2.5, size=(B, T, 5)).astype(np.float32)
    seq_len = np.array([65, 40, 65, 12, 6], dtype=np.int32)
    label_len = np.array([20, 13, 0, 20, 4], dtype=np.int32)
    labels = rng.integers(0, 4, size=(B, Lmax)).astype(np.int32)
    labels[4, :4] = 2                                                  # 4 <= 6, but 4 + 3 repeats > 6
    loss, status = _ctc(monkeypatch, logits, seq_len, labels, label_len)
    assert status.tolist() == [0, 0, 0, 1, 2] and np.isfinite(loss[:4]).all() and loss[3] == 0 and loss[4] == np.inf
    want = ctc_ref.ctc_batch(logits.astype(np.float64), seq_len, labels, label_len)[0]
    assert abs(loss[2] - want[2]) <= 1e-5 * abs(want[2]) + 1e-4       # L = 0: the blanks' sum, by the float64 restatement too


def test_ctc_loss_on_the_workspace_heavy_side_of_the_lds_opt_in(built, monkeypatch):
    T = 3648
    rng = np.random.default_rng(T)
    logits = rng.normal(scale=3.0, size=(2, T, 5)).astype(np.float32)
    seq_len = np.array([T, T - 100], dtype=np.int32)
    label_len = np.array([T, T // 2], dtype=np.int32)
    labels = np.zeros((2, T), dtype=np.int32)
    labels[0] = np.arange(T) % 4
    labels[1, :T // 2] = rng.integers(0, 4, T // 2)
    _, status = _ctc(monkeypatch, logits, seq_len, labels, label_len)
    assert status.tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------------------------------------
# the training seams
# ------------------------------------------------------------------------------------------------------------------------------
DEV = torch.device("cuda", 0)


def _rnn_run(spec, w, fea, sl, dl, fresh):
    """Forward and backward through the ABI; fresh: the backward gets a workspace of its own, as uninitialised as the forward's was."""
    p = torch.from_numpy(tc.flat_params(spec, w)).to(DEV)
    x = torch.from_numpy(np.ascontiguousarray(fea, dtype=np.float32)).to(DEV)
    s = torch.from_numpy(np.ascontiguousarray(sl, dtype=np.int32)).to(DEV)
    logits, tape, ws = train.rnn_forward(spec, p, x, s)
    if fresh:
        ws = _lib.device_bytes(train.train_sizes(spec, *fea.shape[:2])[1], DEV)
    dparams, dfeat = train.rnn_backward(spec, p, x, s, torch.from_numpy(dl).to(DEV), tape, ws, True)
    torch.cuda.synchronize()
    return logits.cpu().numpy(), dparams.cpu().numpy(), dfeat.cpu().numpy()


@pytest.mark.parametrize("B,T", [(33, 3), (7, 17)])
@pytest.mark.parametrize("kind", ["dna-stack", "rna-multi"])
def test_rnn_train_forward_and_backward(built, monkeypatch, kind, B, T):
    from oracle import nn_oracle
    from test_gpu_train import _assert_rows
    spec, w, fea, sl, dl = tc.geometry_case(kind, B, T)
    tape_b, ws_b = train.train_sizes(spec, B, T)
    hip = {}
    _, sizes, rows = one_fill(monkeypatch, 0xFF, lambda: tc.accuracy(spec, w, fea, sl, dl, hip_out=hip))     # the reference, once
    assert sizes == [tape_b, ws_b]
    _assert_rows(rows, "%s B=%d T=%d" % (kind, B, T))
    w64 = {k: np.asarray(v, dtype=np.float64) for k, v in w.items()}
    ref = nn_oracle.fc_head(nn_oracle.rnn_forward(fea.astype(np.float64), sl, spec.to_dict(), w64), w64)
    assert np.abs(hip["logits"].astype(np.float64) - ref).max() <= 1e-4
    want = (hip["logits"].tobytes(), hip["flat"].tobytes(), hip["dfeatures"].tobytes())
    for fresh in (False, True):
        runs = per_fill(monkeypatch, lambda: _rnn_run(spec, w, fea, sl, dl, fresh))
        for fill, sizes, (logits, flat, dfeat) in runs:
            assert sizes == [tape_b, ws_b] + [ws_b] * fresh
            assert (logits.tobytes(), flat.tobytes(), dfeat.tobytes()) == want, (fill, fresh)
            assert np.isfinite(logits).all() and np.isfinite(flat).all() and np.isfinite(dfeat).all()
            for b in range(B):
                assert not dfeat[b, sl[b]:].any(), b


def _cnn_run(spec, w, x, g, fresh):
    fea, mom, tape, ws, p, xd = cc.hip_forward(spec, w, x)
    B, L = x.shape
    if fresh:
        ws = _lib.device_bytes(train.cnn_train_sizes(spec, B, L)[1], DEV)
    dp = train.cnn_backward(spec, p, xd, torch.from_numpy(g).to(DEV), tape, ws)
    torch.cuda.synchronize()
    relu = train.cnn_tape_relu(spec, tape, B, L)
    return fea.cpu().numpy(), mom.cpu().numpy(), dp.cpu().numpy(), {k: v.cpu().numpy() for k, v in relu.items()}


@pytest.mark.parametrize("kind", cc.SPECS)
def test_cnn_train_forward_and_backward(built, monkeypatch, kind):
    from test_gpu_cnn_train import FWD_FACTOR, GRAD_FACTOR
    B, L = 7, 120
    spec, w, x, g = cc.grad_case(kind, B, L)
    tape_b, ws_b = train.cnn_train_sizes(spec, B, L)
    label = "%s B=%d L=%d" % (kind, B, L)
    held = per_fill(monkeypatch, lambda: cc.hip_run(spec, w, x, g))
    fea, mom, dp, g_used, masks = held[0][2]
    assert held[0][1] == [tape_b, ws_b] and g_used.tobytes() == g.tobytes()
    cc.assert_rows(cc.forward_rows(spec, w, x, fea, mom, FWD_FACTOR), label + " fwd", FWD_FACTOR)
    cc.assert_rows(cc.gradient_rows(spec, w, x, dp, g_used, masks, GRAD_FACTOR, label), label, GRAD_FACTOR)
    same_bytes(held, lambda r: (r[0].tobytes(), r[1].tobytes(), r[2].tobytes(), [r[4][k].tobytes() for k in sorted(r[4])]))
    stats = [(off, int(np.prod(shape))) for name, (off, shape) in train.cnn_param_layout(spec).items() if name.endswith(("_bn/pop_mean", "_bn/pop_var"))]
    assert stats
    for fresh in (False, True):
        runs = per_fill(monkeypatch, lambda: _cnn_run(spec, w, x, g, fresh))
        for fill, sizes, (fea2, mom2, dp2, relu) in runs:
            assert sizes == [tape_b, ws_b] + [ws_b] * fresh
            assert (fea2.tobytes(), mom2.tobytes(), dp2.tobytes()) == (fea.tobytes(), mom.tobytes(), dp.tobytes()), (fill, fresh)
            assert np.isfinite(fea2).all() and np.isfinite(dp2).all()
            for off, n in stats:
                assert not dp2[off:off + n].any()                      # the statistics' slots: exactly 0
            assert set(relu) == set(masks)
            for name, v in relu.items():                               # the tape's ReLU outputs: written everywhere, and what hip_run saw
                assert np.isfinite(v).all() and v.min() >= 0 and v.max() < 1e30, (name, fill)
                assert ((v > 0) == masks[name]).all(), name


def test_the_hook_is_unset_afterwards():
    assert _lib.alloc_hook is None
