"""CPU: the float64 CTC restatement (tests/ctc_ref.py) against torch's CPU ctc_loss and brute-force path enumeration, the
labelled-window reader (chiron_amd/labelled.py) against the reference's (tests/golden/labelled_windows.json), and the argument
checks of the CTC entry points of the C ABI, none of which needs a GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from chiron_amd import _lib, ctc, labelled

import ctc_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch_ctc(logits, seq_len, labels, label_len):
    torch = pytest.importorskip("torch")
    x = torch.tensor(np.asarray(logits, dtype=np.float64), requires_grad=True)
    lp = x.log_softmax(-1).transpose(0, 1)
    loss = torch.nn.functional.ctc_loss(lp, torch.tensor(np.asarray(labels, dtype=np.int64)), torch.tensor(np.asarray(seq_len, dtype=np.int64)),
                                        torch.tensor(np.asarray(label_len, dtype=np.int64)), blank=4, reduction="none", zero_infinity=False)
    loss.sum().backward()
    return loss.detach().numpy(), x.grad.numpy()


def test_restatement_matches_torch_ctc():
    rng = np.random.default_rng(1)
    B, T, Lmax = 12, 30, 14
    logits = rng.normal(scale=3.0, size=(B, T, 5))
    seq_len = np.array([30, 30, 17, 1, 9, 30, 25, 12, 30, 8, 30, 20])
    labels = rng.integers(0, 4, size=(B, Lmax))
    label_len = np.array([14, 0, 8, 0, 4, 10, 14, 6, 3, 5, 14, 7])
    labels[1] = 0
    labels[3] = 2
    labels[5, :10] = 1                                      # all repeats: needs 2L - 1 = 19 frames
    labels[9, :5] = [0, 1, 1, 2, 3]                         # L + repeats = 6 <= 8
    labels[4, :4] = [2, 2, 2, 2]                            # L + repeats = 7 <= 9
    labels[7, :6] = [0, 0, 1, 1, 2, 2]                      # L + repeats = 9 <= 12
    labels[11, :7] = [3, 3, 3, 0, 0, 1, 2]                  # 7 + 3 = 10 <= 20
    labels[2, :8] = [0, 1, 2, 3, 0, 1, 2, 2]                # 8 + 1 = 9 <= 17
    # feasibility edge: L + repeats == seq_len exactly
    labels[6, :14] = [0, 0, 1, 1, 2, 2, 3, 3, 0, 0, 1, 1, 2, 2]   # 14 + 7 = 21 <= 25
    seq_len[6] = 21
    loss, grad = ctc_ref.ctc_batch(logits, seq_len, labels, label_len)
    tl, tg = _torch_ctc(logits, seq_len, labels, label_len)
    assert np.all(np.isfinite(loss))
    assert np.abs(loss - tl).max() <= 1e-10 * max(1.0, np.abs(tl).max())
    assert np.abs(grad - tg).max() <= 1e-10
    assert np.all(grad[2, 17:] == 0) and np.all(grad[3, 1:] == 0)


def test_restatement_skipped_and_infeasible():
    rng = np.random.default_rng(2)
    x = rng.normal(size=(3, 6, 5))
    labels = np.array([[0, 1, 2, 3, 0, 1, 2], [1, 1, 1, 1, 0, 0, 0], [1, 1, 1, 0, 0, 0, 0]])
    loss, grad = ctc_ref.ctc_batch(x, [6, 6, 6], labels, [7, 4, 3])
    assert loss[0] == 0 and loss[1] == np.inf and np.isfinite(loss[2])      # 7 > 6 skipped; 4 + 3 > 6 infeasible; 3 + 2 <= 6
    assert not grad[0].any() and not grad[1].any()
    assert list(ctc.row_status([6, 6, 6], labels, [7, 4, 3])) == [1, 2, 0]


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6])
def test_restatement_matches_brute_force(T):
    rng = np.random.default_rng(10 + T)
    cases = [[], [0], [1, 1], [2, 3], [0, 1, 0], [3, 3, 3]]
    for lab in cases:
        if len(lab) > T:
            continue
        x = rng.normal(scale=2.0, size=(T, 5))
        ref, _ = ctc_ref.ctc_row(x, lab)
        bf = ctc_ref.brute_force_loss(x, lab)
        if np.isinf(bf):
            assert np.isinf(ref), (T, lab)
        else:
            assert abs(ref - bf) <= 1e-10 * max(1.0, abs(bf)), (T, lab, ref, bf)


def test_levenshtein_helpers():
    assert ctc.levenshtein([0, 1, 2], [0, 1, 2]) == 0
    assert ctc.levenshtein([0, 1, 2], [0, 2]) == 1
    assert ctc.levenshtein([], [1, 2, 3]) == 3
    assert ctc.levenshtein([3, 3, 0, 1], [0, 1, 2]) == 3
    assert ctc.normalized_edit_distance([], []) == 0
    assert ctc.normalized_edit_distance([1], []) == np.inf
    assert ctc.normalized_edit_distance([0, 1], [0, 1, 2, 3]) == np.float32(0.5)
    rows = ctc.sparse_rows(np.array([[0, 0], [0, 1], [2, 0]]), np.array([3, 1, 2]), 3)
    assert rows == [[3, 1], [], [2]]


def test_labelled_reader_matches_reference(tmp_path):
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "labelled_windows.json")))
    assert {c["name"] for c in cases} >= {"gaps", "rejections", "short_padding", "zero_fill"}
    zf = [c for c in cases if c["name"] == "zero_fill"][0]
    assert any(e[-1] == 0 for e in zf["event"])                         # the window's tail is zero-filled
    for c in cases:
        lf = tmp_path / (c["name"] + ".label")
        lf.write_text("\n".join(c["label_lines"]) + "\n")
        lab = labelled.read_label(str(lf))
        assert list(lab.start) == c["raw_label"]["start"] and list(lab.length) == c["raw_label"]["length"]
        assert list(lab.base) == c["raw_label"]["base"]
        ev, el, lb, ll = labelled.read_raw(np.asarray(c["signal"], dtype=np.float32), lab, c["seq_length"])
        assert ev.shape == (len(c["event"]), c["seq_length"])
        assert np.array_equal(ev, np.asarray(c["event"], dtype=np.float32).reshape(ev.shape))
        assert list(el) == c["event_length"] and lb == c["label"] and list(ll) == c["label_length"]


def test_labelled_folder_walk(tmp_path):
    cases = {c["name"]: c for c in json.load(open(os.path.join(ROOT, "tests", "golden", "labelled_windows.json")))}
    for name in ("contiguous", "gaps"):
        c = cases[name]
        (tmp_path / (name + ".signal")).write_text(" ".join(str(int(v)) for v in c["signal"]))
        (tmp_path / (name + ".label")).write_text("\n".join(c["label_lines"]) + "\n")
    (tmp_path / "badbase.signal").write_text(" ".join(["500"] * 400))
    (tmp_path / "badbase.label").write_text("\n".join("%d %d N" % (i, i + 3) for i in range(0, 90, 3)) + "\n")
    (tmp_path / "past_end.signal").write_text(" ".join(["500"] * 50))
    (tmp_path / "past_end.label").write_text("\n".join("%d %d A" % (i, i + 3) for i in range(0, 90, 3)) + "\n")
    ds = labelled.read_raw_data_sets(str(tmp_path), seq_length=60)
    ev, el, lb, ll = labelled.read_raw(np.asarray(cases["gaps"]["signal"], dtype=np.float32),
                                       labelled.read_label(str(tmp_path / "gaps.label")), 60)
    ev2, _, lb2, _ = labelled.read_raw(np.asarray(cases["contiguous"]["signal"], dtype=np.float32),
                                       labelled.read_label(str(tmp_path / "contiguous.label")), 60)
    assert ds.event.shape[0] == ev.shape[0] + ev2.shape[0]          # the two broken files are skipped, not fatal
    assert ds.label == lb2 + lb                                      # sorted within the folder: contiguous, gaps
    capped = labelled.read_raw_data_sets(str(tmp_path), seq_length=60, max_segments=5)
    assert capped.event.shape[0] == 5 and capped.label == ds.label[:5]
    dense = labelled.dense_labels(ds.label, ds.label_length)
    assert dense.shape == (len(ds.label), int(ds.label_length.max()))


def test_ctc_workspace_size_formula_and_bound(built):
    lib = _lib.load()
    out = C.c_size_t()
    for B, T, L in ((1100, 100, 45), (3, 8192, 8192), (7, 5, 9), (0, 10, 3)):
        assert lib.chiron_ctc_workspace_size(B, T, L, _lib.CTC_WANT_GRAD, C.byref(out)) == _lib.OK
        assert out.value == B * T * (2 * min(L, T) + 1) * 8
        assert lib.chiron_ctc_workspace_size(B, T, L, 0, C.byref(out)) == _lib.OK and out.value == 0
    assert lib.chiron_ctc_workspace_size(1, _lib.CTC_MAX_T + 1, 4, 0, C.byref(out)) == _lib.ERR_OVERFLOW
    assert lib.chiron_ctc_workspace_size(1, 100, _lib.CTC_MAX_LABEL + 1, 0, C.byref(out)) == _lib.ERR_OVERFLOW
    # at the bound the formula still holds: the largest workspace (2^31 - 1 rows) is about 2^61 bytes, 64-bit offsets throughout
    assert lib.chiron_ctc_workspace_size(2 ** 31 - 1, _lib.CTC_MAX_T, _lib.CTC_MAX_LABEL, _lib.CTC_WANT_GRAD, C.byref(out)) == _lib.OK
    assert out.value == (2 ** 31 - 1) * 8192 * 16385 * 8
    assert lib.chiron_ctc_workspace_size(-1, 10, 3, 0, C.byref(out)) == _lib.ERR_INVALID


def test_ctc_loss_rejects_bad_arguments(built):
    """Argument errors come back before anything is launched; host arrays are enough to see them."""
    lib = _lib.load()
    B, T, L = 3, 10, 4
    logits = np.zeros((B, T, 5), dtype=np.float32)
    loss = np.zeros(B, dtype=np.float32)

    def call(seq_len, labels, label_len, batch=B, t=T):
        s = np.ascontiguousarray(seq_len, dtype=np.int32)
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        ln = np.ascontiguousarray(label_len, dtype=np.int32)
        return lib.chiron_ctc_loss(0, logits.ctypes.data, s.ctypes.data, lab.ctypes.data, ln.ctypes.data, batch, t, L, 0,
                                   loss.ctypes.data, None, None, None)

    good = np.zeros((B, L), dtype=np.int32)
    assert call([10, 5, 0], np.array([[0, 1, 2, 4]] * 3), [4, 2, 0]) == _lib.ERR_INVALID          # label 4 = blank
    assert call([10, 5, 0], np.array([[0, -1, 2, 3]] * 3), [4, 2, 0]) == _lib.ERR_INVALID
    assert call([10, 5, 0], good, [4, 5, 0]) == _lib.ERR_INVALID                                    # > max_label_len
    assert call([10, 5, 0], good, [4, -1, 0]) == _lib.ERR_INVALID
    assert call([11, 5, 0], good, [4, 2, 0]) == _lib.ERR_INVALID                                    # seq_len > T
    assert call([10, -1, 0], good, [4, 2, 0]) == _lib.ERR_INVALID
    assert call([10, 5, 0], good, [4, 2, 0], batch=-1) == _lib.ERR_INVALID
    assert b"label" in lib.chiron_last_error() or b"batch" in lib.chiron_last_error()
    # labels past label_len are padding and are not checked: what stops these host arrays is the device-memory check (a GPU is
    # visible) or the missing device (none is), never the label check
    pad = np.array([[0, 1, 2, 3], [1, 9, 9, 9], [7, 7, 7, 7]], dtype=np.int32)
    st = call([10, 5, 0], pad, [4, 1, 0])
    assert st in (_lib.ERR_INVALID, _lib.ERR_DEVICE)
    assert b"label" not in lib.chiron_last_error()


def test_engine_score_null_engine(built):
    lib = _lib.load()
    labels = np.zeros((2, 3), dtype=np.int32)
    ln = np.zeros(2, dtype=np.int32)
    out = np.zeros(2, dtype=np.float32)
    st = np.zeros(2, dtype=np.int32)
    assert lib.chiron_engine_score(None, 0, labels.ctypes.data, ln.ctypes.data, 2, 3, 0, out.ctypes.data, out.ctypes.data,
                                   st.ctypes.data) == _lib.ERR_INVALID
    assert b"null engine" in lib.chiron_last_error()
