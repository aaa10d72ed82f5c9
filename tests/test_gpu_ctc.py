"""GPU: the CTC loss / gradient kernels (chiron_ctc_loss) against the float64 restatement (tests/ctc_ref.py) and torch's float64
autograd, the autograd Function, determinism, Engine.score (chiron_engine_score) after submit (greedy, beam), after
chiron_engine_decode and on an RNA engine, the edit distance on truths of one to five 64-position words (tests/score_cases.py), the
gradient on both sides of the 64 KB LDS opt-in, and `validate` end to end."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import chiron_amd as ca
from chiron_amd import ctc, labelled

import ctc_ref
import score_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tol(ref):
    return 1e-5 * np.abs(ref) + 1e-4


def _check_loss(got, ref):
    got = np.asarray(got, dtype=np.float64)
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(got), inf)
    assert np.all(np.abs(got[~inf] - ref[~inf]) <= _tol(ref[~inf])), np.abs(got[~inf] - ref[~inf]).max()


@pytest.mark.parametrize("T", [1, 2, 7, 63, 64, 65, 400, 8192])
def test_loss_matches_float64(built, T):
    rng = np.random.default_rng(T)
    lens = sorted({0, 1, T // 2, T})
    B = len(lens) + 2
    logits = rng.normal(scale=2.0, size=(B, T, 5)).astype(np.float32)
    seq_len = np.full(B, T, dtype=np.int32)
    Lmax = max(lens)
    labels = np.zeros((B, max(Lmax, 1)), dtype=np.int32)
    label_len = np.zeros(B, dtype=np.int32)
    for i, L in enumerate(lens):
        # the longest feasible labels have no repeats: 0,1,2,3,0,1,...
        labels[i, :L] = np.arange(L) % 4 if L == T else rng.integers(0, 4, L)
        label_len[i] = L
    # an all-repeat row (AAAA: 2L - 1 frames) and a ragged row
    L = (T + 1) // 2
    labels[-2, :L] = 0
    label_len[-2] = L
    seq_len[-1] = T // 3
    labels[-1, :min(2, T)] = [1, 2][:min(2, T)]
    label_len[-1] = min(2, T)
    loss = ctc.ctc_loss(logits, seq_len, labels, label_len)
    ref = ctc_ref.ctc_loss_batched(logits, seq_len, labels, label_len)
    assert np.isfinite(ref[:-1]).all()
    _check_loss(loss, ref)


def test_headline_batch_and_ragged(built):
    rng = np.random.default_rng(5)
    B, T = 1100, 400
    logits = rng.normal(scale=3.0, size=(B, T, 5)).astype(np.float32)
    label_len = rng.integers(35, 56, B).astype(np.int32)
    seq_len = np.full(B, T, dtype=np.int32)
    seq_len[::7] = rng.integers(0, T + 1, len(seq_len[::7]))
    seq_len[3] = 0
    label_len[3] = 0
    labels = rng.integers(0, 4, size=(B, 56)).astype(np.int32)
    loss = ctc.ctc_loss(logits, seq_len, labels, label_len)
    ref = ctc_ref.ctc_loss_batched(logits, seq_len, labels, label_len)
    _check_loss(loss, ref)
    assert loss[3] == 0


def test_skipped_infeasible_and_gradient(built):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(9)
    B, T = 8, 40
    logits = rng.normal(scale=2.5, size=(B, T, 5)).astype(np.float32)
    seq_len = np.array([40, 40, 31, 12, 40, 4, 0, 40], dtype=np.int32)
    labels = rng.integers(0, 4, size=(B, 20)).astype(np.int32)
    label_len = np.array([20, 13, 9, 13, 0, 3, 0, 4], dtype=np.int32)
    labels[5, :3] = [2, 2, 2]          # 3 <= 4, but 3 + 2 repeats > 4: infeasible
    labels[7, :4] = [1, 1, 0, 0]
    loss, grad = ctc.ctc_loss(logits, seq_len, labels, label_len, want_grad=True)
    ref, _ = ctc_ref.ctc_batch(logits.astype(np.float64), seq_len, labels, label_len)
    _check_loss(loss, ref)
    assert loss[3] == 0 and not grad[3].any()            # skipped (13 > 12)
    assert loss[5] == np.inf and not grad[5].any()       # infeasible
    assert loss[6] == 0 and not grad[6].any()            # seq_len 0, no labels
    for b in range(B):
        assert not grad[b, seq_len[b]:].any()            # frames past seq_len are exactly 0
    ok = np.array([0, 1, 2, 4, 7])
    x = torch.tensor(logits[ok].astype(np.float64), requires_grad=True)
    tl = torch.nn.functional.ctc_loss(x.log_softmax(-1).transpose(0, 1), torch.tensor(labels[ok].astype(np.int64)),
                                      torch.tensor(seq_len[ok].astype(np.int64)), torch.tensor(label_len[ok].astype(np.int64)),
                                      blank=4, reduction="none")
    tl.sum().backward()
    assert np.abs(grad[ok] - x.grad.numpy()).max() <= 1e-5
    assert np.all(np.abs(loss[ok] - tl.detach().numpy()) <= _tol(tl.detach().numpy()))


def _torch_grad(logits, seq_len, labels, label_len):
    torch = pytest.importorskip("torch")
    x = torch.tensor(logits.astype(np.float64), requires_grad=True)
    tl = torch.nn.functional.ctc_loss(x.log_softmax(-1).transpose(0, 1), torch.tensor(labels.astype(np.int64)),
                                      torch.tensor(seq_len.astype(np.int64)), torch.tensor(label_len.astype(np.int64)),
                                      blank=4, reduction="none")
    tl.sum().backward()
    return tl.detach().numpy(), x.grad.numpy()


@pytest.mark.parametrize("B,T,L", [(1100, 400, 45), (4, 2000, 220)])
def test_gradient_at_headline_and_long_geometry(built, B, T, L):
    """The 1e-5 gradient bound where the gradient is used: the headline batch (1100 x 400, about 45 labels, logit scale 3; torch's
    float64 reference on a subset of rows) and a long window."""
    rng = np.random.default_rng(T)
    logits = rng.normal(scale=3.0, size=(B, T, 5)).astype(np.float32)
    seq_len = np.full(B, T, dtype=np.int32)
    seq_len[::5] = rng.integers(T // 2, T + 1, len(seq_len[::5]))
    label_len = rng.integers(L - 8, L + 9, B).astype(np.int32)
    labels = rng.integers(0, 4, (B, L + 8)).astype(np.int32)
    loss, grad = ctc.ctc_loss(logits, seq_len, labels, label_len, want_grad=True)
    # trusted arguments: same kernels, same bits, no read-back
    loss2, grad2 = ctc.ctc_loss(logits, seq_len, labels, label_len, want_grad=True, check=False)
    assert np.array_equal(loss, loss2) and np.array_equal(grad, grad2)
    rows = np.arange(B) if B <= 8 else rng.choice(B, 48, replace=False)
    tl, tg = _torch_grad(logits[rows], seq_len[rows], labels[rows], label_len[rows])
    _check_loss(loss[rows], tl)
    assert np.abs(grad[rows] - tg).max() <= 1e-5, np.abs(grad[rows] - tg).max()


def test_autograd_function_and_determinism(built):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(11)
    B, T, L = 64, 200, 30
    dev = torch.device("cuda", 0)
    x = torch.tensor(rng.normal(scale=2.0, size=(B, T, 5)).astype(np.float32), device=dev, requires_grad=True)
    sl = torch.tensor(rng.integers(L + 20, T + 1, B).astype(np.int32), device=dev)
    lab = torch.tensor(rng.integers(0, 4, (B, L)).astype(np.int32), device=dev)
    ll = torch.tensor(rng.integers(0, L + 1, B).astype(np.int32), device=dev)
    out = ctc.CTCLoss.apply(x, sl, lab, ll)
    out.sum().backward()
    loss1, grad1 = ctc.ctc_loss(x.detach(), sl, lab, ll, want_grad=True)
    loss2, grad2 = ctc.ctc_loss(x.detach(), sl, lab, ll, want_grad=True)
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), loss1)
    assert torch.equal(x.grad, grad1)
    assert torch.equal(loss1, loss2) and torch.equal(grad1, grad2)          # bitwise, run to run
    w = torch.linspace(0.5, 2.0, B, device=dev)
    x.grad = None
    (ctc.CTCLoss.apply(x, sl, lab, ll) * w).sum().backward()
    assert torch.allclose(x.grad, grad1 * w.reshape(-1, 1, 1), rtol=0, atol=1e-6)


def _labels_for(rng, n, Lmax=60):
    ll = rng.integers(20, Lmax + 1, n).astype(np.int32)
    ll[0] = 0
    return rng.integers(0, 4, (n, Lmax)).astype(np.int32), ll


def _check_score(eng, res, x_rows, sl, labels, ll, logits=None, want=None):
    """want: the rows' normalized edit distances, for a caller that scores the same rows more than once (plain DP is slow)"""
    loss, edit, status = eng.score(0, labels, ll)
    ref_loss = ctc.ctc_loss(res.logits if logits is None else logits, sl, labels, ll)                       # the standalone kernel on the collected logits
    assert np.array_equal(loss.view(np.uint32), ref_loss.view(np.uint32))
    assert list(status) == list(ctc.row_status(sl, labels, ll))
    if res.decoded is not None:
        rows = ctc.sparse_rows(res.decoded.indices, res.decoded.values, x_rows)
    else:
        flat, counts = res.compact.flat, res.compact.counts
        off = np.concatenate([[0], np.cumsum(counts)])
        rows = [list(flat[off[i]:off[i + 1]]) for i in range(x_rows)]
    if want is None:
        want = ctc.edit_distance(rows, labels, ll)
    assert np.array_equal(edit, want), (edit[:8], want[:8])
    return loss, edit, status


def test_engine_score_greedy_beam_decode(built):
    spec = ca.dna_default_spec()
    w = ca.synthetic_weights(spec, seed=7)
    B, Lseg = 48, 400
    sig = ca.synthetic_signal(1, 390 * B + 400, seed=3)[0]
    x = np.stack([sig[i * 390:i * 390 + Lseg] for i in range(B)]).astype(np.float32)
    rng = np.random.default_rng(2)
    labels, ll = _labels_for(rng, B)
    ll[1] = 60
    labels[1, :] = 2                      # 60 repeats need 119 frames: infeasible at seq_len 100
    with ca.Engine(spec, w, max_batch=B, segment_len=Lseg, max_beam=30) as eng:
        sl = ca.seq_len_for_engine(np.full(B, Lseg), eng.ratio)
        sl[5] = 30                         # ragged: row 5 is skipped (ll > 30)
        sl[1] = 100
        with pytest.raises(ca.engine._lib.ChironError) as ei:
            eng.score(0, labels, ll)       # nothing collected yet
        assert ei.value.status == ca.engine._lib.ERR_STATE
        for beam in (0, 30):
            res = eng.infer(x, sl, beam_width=beam, want_logits=True)
            loss, edit, status = _check_score(eng, res, B, sl, labels, ll)
            assert status[1] == 2 and np.isinf(loss[1])
        # compact decode leaves the same SparseTensor on the device (its collect hands out no logits: the batch's are the ones above)
        eng.submit(0, x, sl, beam_width=30, compact=True)
        comp = eng.collect(0)
        assert comp.decoded is None
        _check_score(eng, comp, B, sl, labels, ll, logits=res.logits)
        with pytest.raises(ca.engine._lib.ChironError):
            eng.score(0, labels[:5], ll[:5])   # batch does not match
        # crafted logits: greedy strings known; insertion, deletion, substitution against the truths
        T = eng.T
        want_rows = [[0, 1, 2, 3], [0, 1, 1, 2], [3, 2], [], [1, 2, 3, 0, 1]]
        n = len(want_rows)
        lg = np.full((n, T, 5), -4.0, dtype=np.float32)
        lg[:, :, 4] = 4.0
        for r, seq in enumerate(want_rows):
            for i, c in enumerate(seq):
                lg[r, 10 + 3 * i, c] = 6.0
        truths = [[0, 1, 2, 3], [0, 1, 2], [1, 2], [0], [1, 2, 0, 1]]   # exact, insertion, substitution, deletion, insertion
        tl = np.array([len(t) for t in truths], dtype=np.int32)
        tlab = np.zeros((n, 5), dtype=np.int32)
        for r, t in enumerate(truths):
            tlab[r, :len(t)] = t
        dsl = np.full(n, T, dtype=np.int32)
        res = eng.decode(lg, dsl, beam_width=0)
        assert ctc.sparse_rows(res.decoded.indices, res.decoded.values, n) == want_rows
        loss, edit, status = eng.score(0, tlab, tl)
        assert list(edit) == [0.0, np.float32(1) / np.float32(3), 0.5, 1.0, 0.25]
        assert np.array_equal(loss, ctc.ctc_loss(lg, dsl, tlab, tl))


def test_engine_score_edit_distance_across_truth_words(built):
    """edit_kernel on the rows of tests/score_cases.py: truths of 1 .. 320 positions (one to five 64-position words, exactly 64, 128,
    192, 256 and 320 among them), hypotheses one or two edits away, empty hypotheses and truths, designed rows at the edges of the
    kernel's 64-row blocks.  Bit for bit float32(d) / float32(m) with d from plain dynamic programming
    (score_cases.normalized, held to ctc.levenshtein on these rows by tests/test_score_cases_cpu.py); then the same collected batch
    against truths cut to 64 positions with max_label_len 64 and again at 320, so that the workspace stride changes between calls."""
    rows = score_cases.edit_cases(400)
    B = len(rows)
    hyps = [hyp for _, hyp, _ in rows]
    labels, ll = score_cases.dense_truths(rows)
    assert labels.shape == (B, 320) and B > 128
    want = score_cases.normalized(hyps, labels, ll)
    claim = score_cases.claims(400)
    for b, (name, hyp, truth) in enumerate(rows):
        if truth:           # the designed distances, as far as the construction decides them
            lo, hi = (np.float32(d) / np.float32(len(truth)) for d in claim[name])
            assert lo <= want[b] <= hi, name
    by_name = {name: b for b, (name, _, _) in enumerate(rows)}
    assert np.isposinf(want[by_name["empty_truth"]]) and want[by_name["both_empty"]] == 0 and want[by_name["empty_hyp_m320"]] == 1
    assert want[by_name["norepeat_del_first_m320"]] == np.float32(1) / np.float32(320)
    labels64, ll64 = np.ascontiguousarray(labels[:, :64]), np.minimum(ll, 64)
    want64 = score_cases.normalized(hyps, labels64, ll64)
    spec = ca.dna_default_spec()
    with ca.Engine(spec, ca.synthetic_weights(spec, seed=7), max_batch=B, segment_len=400) as eng:
        assert eng.T == 400
        lg = score_cases.greedy_logits(hyps, eng.T)
        sl = np.full(B, eng.T, dtype=np.int32)
        res = eng.decode(lg, sl, beam_width=0)
        assert ctc.sparse_rows(res.decoded.indices, res.decoded.values, B) == hyps
        for lab, n, w in ((labels, ll, want), (labels64, ll64, want64), (labels, ll, want)):
            _, edit, _ = _check_score(eng, res, B, sl, lab, n, logits=lg, want=w)
            assert edit.tobytes() == w.tobytes()


def _lds_bytes(S):
    """ctc_lds_bytes of csrc/ctc_loss.hip: the state row (S doubles), the frame's log-softmax (8 doubles), the extended label
    (S bytes, rounded up to 8)"""
    return (S + 8) * 8 + (S + 7) // 8 * 8


@pytest.mark.parametrize("T", [3632, 3648])
def test_gradient_on_both_sides_of_the_64k_lds_opt_in(built, T):
    """ctc_beta_kernel with the last LDS size that needs no opt-in (T = Lmax = 3632: 65 456 bytes, the next multiple of 16 is past
    64 KB) and the first size tested that needs it (3648: 65 744 bytes).  launch_ctc raises the limit of BOTH kernels; the loss
    kernel alone runs above 64 KB elsewhere (test_loss_matches_float64 at T = 8192).  Rows: the longest feasible labels (no repeats,
    one path), random labels of T / 2, a ragged row.  The alpha workspace is 3 * T * (2T + 1) doubles, about 0.64 GB."""
    Lmax = T
    S = 2 * min(Lmax, T) + 1
    assert _lds_bytes(S) == {3632: 65456, 3648: 65744}[T]
    assert _lds_bytes(2 * 3632 + 1) <= 64 * 1024 < _lds_bytes(2 * 3648 + 1)
    with open(os.path.join(ROOT, "chiron_amd", "csrc", "ctc_loss.hip")) as f:
        text = f.read()
    assert re.search(r"size_t ctc_lds_bytes\(int S_lds\) \{ return \(\(size_t\)S_lds \+ 8\) \* sizeof\(double\) \+ "
                     r"\(\(\(size_t\)S_lds \+ 7\) & ~\(size_t\)7\); \}", text)
    assert re.search(r"if \(lds > 64 \* 1024\) \{\s*if \(hipFuncSetAttribute\([^;]*ctc_alpha_kernel[^;]*hipFuncSetAttribute\([^;]*ctc_beta_kernel", text)
    assert re.search(r"p\.S_lds = S_ws;", text) and re.search(r"const int64_t S = 2 \* \(Lmax < T \? Lmax : T\) \+ 1;", text)
    rng = np.random.default_rng(T)
    B = 3
    logits = rng.normal(scale=3.0, size=(B, T, 5)).astype(np.float32)
    seq_len = np.array([T, T, T - 100], dtype=np.int32)
    label_len = np.array([T, T // 2, 40], dtype=np.int32)
    labels = np.zeros((B, Lmax), dtype=np.int32)
    labels[0] = np.arange(T) % 4
    labels[1, :T // 2] = rng.integers(0, 4, T // 2)
    labels[2, :40] = rng.integers(0, 4, 40)
    assert list(ctc.row_status(seq_len, labels, label_len)) == [0, 0, 0]
    loss, grad = ctc.ctc_loss(logits, seq_len, labels, label_len, want_grad=True)
    tl, tg = _torch_grad(logits, seq_len, labels, label_len)
    assert np.isfinite(tl).all()
    _check_loss(loss, tl)
    assert np.abs(grad - tg).max() <= 1e-5, np.abs(grad - tg).max()
    assert not grad[2, T - 100:].any() and grad[2, :T - 100].any()          # frames past seq_len are exactly 0


def test_engine_score_rna(built):
    spec = ca.rna_default_spec()
    w = ca.synthetic_weights(spec, seed=5)
    B, Lseg = 12, 2000
    sig = ca.synthetic_signal(1, 1900 * B + 2000, seed=4)[0]
    x = np.stack([sig[i * 1900:i * 1900 + Lseg] for i in range(B)]).astype(np.float32)
    rng = np.random.default_rng(8)
    labels, ll = _labels_for(rng, B, Lmax=120)
    with ca.Engine(spec, w, max_batch=B, segment_len=Lseg) as eng:
        lens = np.full(B, Lseg)
        lens[-1] = 1234
        sl = ca.seq_len_for_engine(lens, eng.ratio)
        res = eng.infer(x, sl, beam_width=0, want_logits=True)
        _check_score(eng, res, B, sl, labels, ll)


def _write_pairs(folder, rng, n_files=3, n_sig=6000):
    os.makedirs(folder, exist_ok=True)
    for f in range(n_files):
        sig = ca.synthetic_signal(1, n_sig, seed=30 + f)[0]
        with open(os.path.join(folder, "read%d.signal" % f), "w") as fh:
            fh.write(" ".join(str(int(v)) for v in sig))
        pos, lines = 3, []
        while pos < n_sig - 40:
            n = int(rng.integers(4, 14))
            lines.append("%d %d %s" % (pos, pos + n, "ACGT"[int(rng.integers(0, 4))]))
            pos += n + int(rng.integers(0, 3))
        with open(os.path.join(folder, "read%d.label" % f), "w") as fh:
            fh.write("\n".join(lines) + "\n")


def test_validate_end_to_end(built, tmp_path):
    rng = np.random.default_rng(13)
    data = str(tmp_path / "data")
    _write_pairs(data, rng)
    model = os.path.join(ROOT, "chiron_amd", "model", "DNA_default")
    out = str(tmp_path / "report.json")
    cmd = [sys.executable, "-m", "chiron_amd.entry", "validate", "-i", data, "-m", model, "-l", "400", "-b", "16", "--beam", "0",
           "--fl_gamma", "2", "--synthetic-weights", "-o", out]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = json.load(open(out))
    ds = labelled.read_raw_data_sets(data, seq_length=400)
    spec, w, _ = ca.load_model(model, allow_synthetic=True)
    n = ds.event.shape[0]
    assert rep["summary"]["windows"] == n and n > 16
    losses, edits = [], []
    with ca.Engine(spec, w, max_batch=16, segment_len=400) as eng:
        for i in range(0, n, 16):
            sl = ca.seq_len_for_engine(ds.event_length[i:i + 16], eng.ratio)
            res = eng.infer(ds.event[i:i + 16], sl, beam_width=0, want_logits=True)
            ll = ds.label_length[i:i + 16]
            lab = labelled.dense_labels(ds.label[i:i + 16], ll)
            losses.append(ctc_ref.ctc_loss_batched(res.logits, sl, lab, ll))
            edits.append(ctc.edit_distance(ctc.sparse_rows(res.decoded.indices, res.decoded.values, len(sl)), lab, ll))
    loss = np.concatenate(losses)
    edit = np.concatenate(edits)
    kept = np.isfinite(loss)
    ref_mean = loss[kept].mean()
    assert abs(rep["summary"]["loss_mean_reference"] - ref_mean) <= 1e-5 * abs(ref_mean) + 1e-4
    assert rep["summary"]["infeasible"] == int((~kept).sum())
    assert abs(rep["summary"]["error_mean"] - edit.mean()) <= 1e-6
    foc = ctc.focal(loss[kept], 2.0).mean()
    assert abs(rep["summary"]["focal_loss_mean_reference"] - foc) <= 1e-5 * abs(foc) + 1e-4
    assert sum(b["n"] for b in rep["batches"]) == n and len(rep["batches"]) == -(-n // 16)
