"""GPU tests of the training seam: chiron_rnn_train_forward / _backward against the float64 reference (tests/rnn_ref.py), their
exact properties, the autograd module and `chiron finetune` end to end.  The gradient bar is explained in tests/train_cases.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import chiron_amd as ca
from chiron_amd import labelled, train

import regimes
import train_cases as tc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["dna-stack", "rna-multi"]


def _torch():
    import torch
    return torch


# ---------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_forward_against_the_oracle_and_the_engine(built, kind):
    """Logits of the tape-writing forward on the float64 oracle's own features: within 1e-4 of the oracle; on the fp32 engine's
    device features: within 2e-4 of the engine's logits (two fp32 pipelines, each within 1e-4 of the same oracle)."""
    from oracle import nn_oracle
    torch = _torch()
    spec = tc.specs()[kind]
    w = ca.synthetic_weights(spec, seed=7)
    rng = np.random.default_rng(21)
    B, L = 19, 400 if kind == "dna-stack" else 500
    x, fea64 = tc.oracle_features(spec, w, B, L, rng)
    T = fea64.shape[1]
    sl = tc.ragged_seq_len(B, T, rng)
    ref = nn_oracle.fc_head(nn_oracle.rnn_forward(fea64, sl, spec.to_dict(), w), {k: np.asarray(v, dtype=np.float64) for k, v in w.items()})
    dev = torch.device("cuda", 0)
    p = torch.from_numpy(tc.flat_params(spec, w)).to(dev)
    sl_d = torch.from_numpy(sl).to(dev)
    logits, _, _ = train.rnn_forward(spec, p, torch.from_numpy(fea64.astype(np.float32)).to(dev), sl_d)
    err = float(np.abs(logits.cpu().numpy().astype(np.float64) - ref).max())
    print("%s: max |train forward - oracle| = %.3g" % (kind, err))
    assert err <= 1e-4
    with ca.Engine(spec, w, max_batch=B, segment_len=L) as eng:
        res = eng.infer(x.astype(np.float32), sl, beam_width=0, want_logits=True)
        feats = train.device_features(eng, 0)
        assert np.array_equal(feats.cpu().numpy(), eng.features(0))
        logits2, _, _ = train.rnn_forward(spec, p, feats, sl_d)
    err2 = float(np.abs(logits2.cpu().numpy() - res.logits).max())
    print("%s: max |train forward - engine| = %.3g" % (kind, err2))
    assert err2 <= 2e-4


# ---------------------------------------------------------------------------------------------
# gradients against float64 autograd, bar = 4 x the float32 restatement's own error
# ---------------------------------------------------------------------------------------------
def _assert_rows(rows, label):
    worst = max(rows.items(), key=lambda kv: kv[1]["ratio"] if kv[1]["norm"] > 0 else 0.0)
    for name, r in rows.items():
        print("%s %-62s err %.3g  e32 %.3g  err/e32 %.3g" % (label, name, r["err_rel"], r["e32_rel"], r["ratio"]))
    bad = [n for n, r in rows.items() if not r["ok"]]
    assert not bad, "%s: beyond %g x e32 + %g ||g64||: %s (worst %s: %.3g)" % (label, tc.FACTOR, tc.FLOOR, bad, worst[0], worst[1]["ratio"])


@pytest.mark.parametrize("T", [60, 400])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("source", ["random", "ctc"])
def test_gradients_against_float64_autograd(built, kind, T, source):
    spec = tc.specs()[kind]
    w = ca.synthetic_weights(spec, seed=7)
    rng = np.random.default_rng(100 + T)
    B = 24
    fea = tc.random_features(B, T, 256, rng)
    sl = tc.ragged_seq_len(B, T, rng)
    dl = rng.normal(size=(B, T, 5)).astype(np.float32) if source == "random" else tc.ctc_dlogits(sl, rng, T)[0]
    _assert_rows(tc.accuracy(spec, w, fea, sl, dl), "%s T=%d %s" % (kind, T, source))


@pytest.mark.parametrize("case", tc.CAP_CASES, ids=lambda c: "%s-B%d-T%d-%s" % c)
def test_gradients_past_the_reduction_caps(built, case):
    """More rows than the caps of the reductions over T * BP rows provide for (tests/train_cases.py, CAP_CASES): the head backward's
    workgroups straddle frames and padding rows, the split-K GEMMs and the column sum run 64 capped slices with a ragged last one.
    Every tensor is held to the bar of the cases above."""
    kind, B, T, what = case
    spec, w, fea, sl, dl = tc.cap_case(kind, B, T)
    hip = {}
    _assert_rows(tc.accuracy(spec, w, fea, sl, dl, hip_out=hip), "%s B=%d T=%d %s" % case)
    if what == "split":     # the slices are summed in slice order: two identical calls, the same bits
        _, _, dfeat2, flat2, _ = tc.hip_forward_backward(spec, w, fea, sl, dl)
        assert flat2.tobytes() == hip["flat"].tobytes() and dfeat2.tobytes() == hip["dfeatures"].tobytes()


@pytest.mark.parametrize("case", tc.GEOMETRY_CASES, ids=lambda c: "%s-B%d-T%d" % c)
def test_forward_and_gradients_at_tiny_and_odd_frame_counts(built, case):
    """T = 1, 2, 3, 17 and 33 with lengths drawn from 0 .. T (tests/train_cases.py, GEOMETRY_CASES).  The logits are held as
    test_forward_against_the_oracle_and_the_engine holds them, every gradient and dfeatures to the bar of the cases above.  At
    T = 1 no step has a predecessor: chiron_rnn_train_backward zeroes dWh in a branch of its own, and the recurrent rows of every
    kernel gradient are exactly 0.  The reductions run in a fixed order: two identical calls, the same bits."""
    from oracle import nn_oracle
    kind, B, T = case
    spec, w, fea, sl, dl = tc.geometry_case(kind, B, T)
    assert tuple(sl[:3]) == (0, 1, T)
    hip = {}
    rows = tc.accuracy(spec, w, fea, sl, dl, hip_out=hip)
    label = "%s B=%d T=%d" % case
    w64 = {k: np.asarray(v, dtype=np.float64) for k, v in w.items()}
    ref = nn_oracle.fc_head(nn_oracle.rnn_forward(fea.astype(np.float64), sl, spec.to_dict(), w64), w64)
    assert hip["logits"].shape == ref.shape == (B, T, 5)
    err = float(np.abs(hip["logits"].astype(np.float64) - ref).max())
    print("%s: max |train forward - oracle| = %.3g" % (label, err))
    assert err <= 1e-4
    _assert_rows(rows, label)
    assert set(rows) == set(train.param_layout(spec)) | {"dfeatures"}
    for b in range(B):     # d features is exactly 0 past every row's end
        assert not hip["dfeatures"][b, sl[b]:].any(), b
    if T == 1:
        kernels = [name for name in hip["named"] if name.endswith("lstm_cell/kernel")]
        assert len(kernels) == 2 * spec.rnn_layers
        for name in kernels:
            grad = hip["named"][name]
            in_w = grad.shape[0] - spec.hidden
            assert grad[:in_w].any() and not grad[in_w:].any(), name
    _, _, dfeat2, flat2, _ = tc.hip_forward_backward(spec, w, fea, sl, dl)
    assert flat2.tobytes() == hip["flat"].tobytes() and dfeat2.tobytes() == hip["dfeatures"].tobytes()


@pytest.mark.parametrize("name", ["write-through", "closed", "integrate-no-output", "hold-and-output", "midpoint"])
def test_gradients_with_saturated_gates(built, name):
    spec = ca.dna_default_spec()
    w = regimes.saturated_gate_weights(spec, name)
    rng = np.random.default_rng(7)
    B, T = 24, 60
    fea = tc.random_features(B, T, 256, rng)
    sl = tc.ragged_seq_len(B, T, rng)
    _assert_rows(tc.accuracy(spec, w, fea, sl, rng.normal(size=(B, T, 5)).astype(np.float32)), "saturated %s" % name)


# ---------------------------------------------------------------------------------------------
# exact properties
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_exact_properties(built, kind):
    spec = tc.specs()[kind]
    w = ca.synthetic_weights(spec, seed=7)
    rng = np.random.default_rng(9)
    B, T = 16, 50
    fea = tc.random_features(B, T, 256, rng)
    sl = tc.ragged_seq_len(B, T, rng)
    sl[B - 1] = 0
    dl = rng.normal(size=(B, T, 5)).astype(np.float32)
    _, _, dfeat, flat, _ = tc.hip_forward_backward(spec, w, fea, sl, dl)
    # d features is exactly 0 past every row's end
    for b in range(B):
        assert not dfeat[b, sl[b]:].any(), b
    assert dfeat[2].any()
    # two identical calls: the same bits
    _, _, dfeat2, flat2, _ = tc.hip_forward_backward(spec, w, fea, sl, dl)
    assert flat.tobytes() == flat2.tobytes() and dfeat.tobytes() == dfeat2.tobytes()
    # a row of seq_len 0 changes no gradient bit, whatever its features
    fea3 = fea.copy()
    fea3[B - 1] = 1e3 * rng.normal(size=(T, 256))
    _, _, dfeat3, flat3, _ = tc.hip_forward_backward(spec, w, fea3, sl, dl)
    assert flat3.tobytes() == flat.tobytes() and dfeat3.tobytes() == dfeat.tobytes()
    # its logits are the head's constant, so its dlogits reach the head's own four tensors and nothing else ...
    head0 = train.param_layout(spec)["rnn_fnn_layer/weights"][0]
    dl4 = dl.copy()
    dl4[B - 1] = 0.0
    _, _, dfeat4, flat4, _ = tc.hip_forward_backward(spec, w, fea, sl, dl4)
    assert flat4[:head0].tobytes() == flat[:head0].tobytes() and dfeat4.tobytes() == dfeat.tobytes()
    # ... and with them zero the batch equals the one without that row: 15 rows are padded to the kernels' 16 by exactly such a row
    _, _, dfeat5, flat5, _ = tc.hip_forward_backward(spec, w, fea[:B - 1], sl[:B - 1], dl[:B - 1])
    assert flat5.tobytes() == flat4.tobytes() and dfeat5.tobytes() == dfeat[:B - 1].tobytes()


@pytest.mark.parametrize("B", [1, 15, 16, 17, 300])
def test_padded_rows_contribute_nothing(built, B):
    """Batches off and on the kernels' 16-row multiple: the gradients meet the same bar against the reference, which knows no padding."""
    spec = ca.dna_default_spec()
    w = ca.synthetic_weights(spec, seed=7)
    rng = np.random.default_rng(40 + B)
    T = 24
    fea = tc.random_features(B, T, 256, rng)
    sl = tc.ragged_seq_len(B, T, rng) if B >= 3 else np.full(B, T, dtype=np.int32)
    _assert_rows(tc.accuracy(spec, w, fea, sl, rng.normal(size=(B, T, 5)).astype(np.float32)), "B=%d" % B)


# ---------------------------------------------------------------------------------------------
# autograd module
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_recurrent_head_autograd_equals_the_abi(built, kind):
    torch = _torch()
    from chiron_amd import ctc
    spec = tc.specs()[kind]
    w = ca.synthetic_weights(spec, seed=7)
    rng = np.random.default_rng(17)
    B, T = 12, 40
    fea = tc.random_features(B, T, 256, rng)
    sl = tc.ragged_seq_len(B, T, rng)
    f, lab, ll = tc.ctc_dlogits(sl, rng, T)
    _, named, dfeat, flat, _ = tc.hip_forward_backward(spec, w, fea, sl, f)
    dev = torch.device("cuda", 0)
    head = train.RecurrentHead(spec, w)
    assert isinstance(head, torch.nn.Module) and [n for n, _ in head.named_parameters()] == ["flat"]
    assert list(head.named_views()) == [n for n, _ in spec._rnn_and_head()]
    for n, v in head.named_views().items():
        assert np.array_equal(v.detach().cpu().numpy(), np.asarray(w[n], dtype=np.float32))
    x = torch.from_numpy(fea).to(dev).requires_grad_(True)
    sl_d = torch.from_numpy(sl).to(dev)
    logits = head(x, sl_d)
    loss = ctc.CTCLoss.apply(logits, sl_d, torch.from_numpy(lab).to(dev), torch.from_numpy(ll).to(dev))
    loss.sum().backward()
    assert head.flat.grad.cpu().numpy().tobytes() == flat.tobytes()
    assert x.grad.cpu().numpy().tobytes() == dfeat.tobytes()
    sw = head.state_weights()
    assert list(sw) == list(spec.canonical_weights(w))
    for k, v in spec.canonical_weights(w).items():
        assert np.asarray(sw[k]).tobytes() == np.asarray(v, dtype=np.float32).tobytes()


# ---------------------------------------------------------------------------------------------
# finetune end to end
# ---------------------------------------------------------------------------------------------
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


FINETUNE_STEPS, FINETUNE_RATE, FINETUNE_BATCH, FINETUNE_REPORT = 40, "4e-3", 32, 2


def test_finetune_end_to_end(built, tmp_path):
    """40 Adam steps at the reference's default rate on a few hundred windows: the training loss falls (mean of the last five
    reports against the first five), the saved folder loads and reproduces the trainer's logits, `validate` runs on it, the CNN is
    untouched."""
    torch = _torch()
    rng = np.random.default_rng(13)
    data = str(tmp_path / "data")
    _write_pairs(data, rng, n_files=20)
    model = os.path.join(ROOT, "chiron_amd", "model", "DNA_default")
    out = str(tmp_path / "tuned")
    cmd = [sys.executable, "-m", "chiron_amd.entry", "finetune", "-i", data, "-o", out, "-m", model, "-s", "400", "-b", str(FINETUNE_BATCH),
           "-t", FINETUNE_RATE, "-x", str(FINETUNE_STEPS), "--report-every", str(FINETUNE_REPORT), "--seed", "5", "--synthetic-weights"]
    r = subprocess.run(["timeout", "-k", "10", "540"] + cmd, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rep = json.load(open(os.path.join(out, "finetune.json")))
    losses = [x["train_loss"] for x in rep["reports"]]
    print("train loss per report:", " ".join("%.4g" % v for v in losses))
    assert len(losses) >= 10 and rep["windows"] >= 200
    assert np.mean(losses[-5:]) < np.mean(losses[:5])
    # the folder loads; the CNN entries are the input's, bit for bit; the recurrent ones moved
    spec0, w0, _ = ca.load_model(model, allow_synthetic=True)
    spec, w, _ = ca.load_model(out)
    assert spec.to_dict() == spec0.to_dict()
    trainable = set(train.param_layout(spec))
    canon0 = spec0.canonical_weights(w0)
    for k in canon0:
        same = np.asarray(w[k]).tobytes() == np.asarray(canon0[k], dtype=np.float32).tobytes()
        assert same != (k in trainable), k
    # an Engine built from it reproduces the trainer's logits
    ds = labelled.read_raw_data_sets(data, seq_length=400)
    xb = np.ascontiguousarray(ds.event[:16], dtype=np.float32)
    with ca.Engine(spec, w, max_batch=16, segment_len=400) as eng:
        sl = ca.seq_len_for_engine(ds.event_length[:16], eng.ratio)
        res = eng.infer(xb, sl, beam_width=0, want_logits=True)
        head = train.RecurrentHead(spec, w)
        logits = head(train.device_features(eng, 0), torch.from_numpy(np.ascontiguousarray(sl, dtype=np.int32)).cuda())
    err = float(np.abs(logits.detach().cpu().numpy() - res.logits).max())
    print("max |trainer logits - engine logits| = %.3g" % err)
    assert err <= 2e-4
    report = str(tmp_path / "report.json")
    v = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "chiron_amd.entry", "validate", "-i", data, "-m", out, "-l", "400",
                        "-b", "16", "--beam", "0", "-o", report], cwd=ROOT, capture_output=True, text=True)
    assert v.returncode == 0, v.stderr[-2000:]
    assert json.load(open(report))["summary"]["windows"] == ds.event.shape[0]
