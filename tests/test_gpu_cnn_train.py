"""GPU tests of the CNN training seam: chiron_cnn_train_forward / _backward against the float64 references (oracle/nn_oracle.py in
batch mode, tests/cnn_ref.py under autograd), their exact properties, train.Network and `chiron train` end to end.

The bar.  Per tensor ||g - g64|| <= FACTOR * e32 + 1e-6 * ||g64|| (tests/train_cases.py's form; e32 = the error of cnn_ref itself run
in float32 on the CPU), FACTOR = max(4, 1.5 x the largest max / median error ratio of an ensemble of float32 realisations of cnn_ref):
the plain run plus 8 draws with every convolution's channels permuted and the batch in another order, on every gradient case below,
CPU only, before any HIP result existed (tools/cnn_grad_accuracy.py -> profiles/cnn_grad_accuracy.json; 1.5 because the HIP blocking
is one more order the ensemble did not draw).
- Forward (features, every site's moments): the ensemble's largest ratio is 1.53, so FWD_FACTOR = 4.
- Gradients.  With free ReLUs the ensemble's ratios reach 3e4: a ReLU whose pre-activation is within rounding of 0 flips between
  realisations and moves every upstream gradient by a discrete amount (one mask element of a site is 1e-3 of a tensor's norm, against
  the 1e-6 of rounding).  A bar that wide shows nothing, so the comparison is made smooth instead: the reference runs under FIXED masks,
  the implementation's own (the tape's ReLU outputs > 0, chiron_cnn_train_tape_relu), after a check that those masks are the float64
  signs everywhere except where the float64 pre-activation is within 1e-4 of the site's rms of 0, and there in at most 1e-3 of the
  elements (cnn_train_cases.assert_masks_legitimate).  Under fixed masks the ensemble's largest ratio is 2.852 (rna, batch 16, segment 500), so GRAD_FACTOR = 4.2778.
The HIP ratios measured afterwards (tools/cnn_grad_accuracy.py --hip) are recorded in the same JSON under "hip"; they did not enter
the choice."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import chiron_amd as ca
from chiron_amd import labelled, train

import cnn_ref
import cnn_train_cases as cc
import train_cases as tc
from train_cases import FLOOR, rel_l2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD_FACTOR = 4.0
GRAD_FACTOR = 4.2778


def _torch():
    import torch
    return torch


# ---------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 7, 16, 300])
@pytest.mark.parametrize("segment", ["short", "full"])
@pytest.mark.parametrize("kind", cc.SPECS)
def test_forward_against_the_float64_oracle_in_batch_mode(built, kind, segment, B):
    from oracle import nn_oracle
    spec = cc.spec_of(kind)
    w = ca.synthetic_weights(spec, seed=7)
    L = 120 if segment == "short" else cc.full_segment(kind)
    x = ca.synthetic_signal(B, L, seed=11)
    fea, mom, _, _, _, _ = cc.hip_forward(spec, w, x)
    fea, mom = fea.cpu().numpy(), mom.cpu().numpy()
    rows = cc.forward_rows(spec, w, x, fea, mom, FWD_FACTOR)
    batch_spec = dict(spec.to_dict(), bn_mode="batch")
    ref = nn_oracle.cnn_forward(x.astype(np.float64), batch_spec, {k: np.asarray(v, dtype=np.float64) for k, v in w.items()})
    assert fea.shape == ref.shape == (B, spec.output_len(L), 256)
    rows["features (oracle)"] = dict(rows["features"], err_rel=rel_l2(fea, ref),
                                     ok=bool(np.linalg.norm(fea - ref) <= FWD_FACTOR * rows["features"]["e32_rel"] * np.linalg.norm(ref)
                                             + FLOOR * np.linalg.norm(ref)))
    cc.assert_rows(rows, "%s L=%d B=%d" % (kind, L, B), FWD_FACTOR)
    # moments_out: only the statistics' slots are written
    named = cc.named(spec, mom)
    for name, v in named.items():
        assert name.endswith(("pop_mean", "pop_var")) or not v.any(), name


def test_network_forward_against_the_inference_engine_in_batch_mode(built):
    """A batch-BN Engine fed the same batch normalises by the same moments: logits within 2e-4 (the bound test_finetune_end_to_end
    uses between trainer and engine)."""
    torch = _torch()
    spec = ca.dna_default_spec("batch")
    w = ca.synthetic_weights(spec, seed=7)
    B, L = 19, 400
    x = ca.synthetic_signal(B, L, seed=3)
    rng = np.random.default_rng(2)
    sl = tc.ragged_seq_len(B, spec.output_len(L), rng)
    net = train.Network(spec, w)
    net.eval()
    logits = net(torch.from_numpy(x).cuda(), torch.from_numpy(sl).cuda()).detach().cpu().numpy()
    with ca.Engine(spec, w, max_batch=B, segment_len=L) as eng:
        res = eng.infer(x, sl, beam_width=0, want_logits=True)
    err = float(np.abs(logits - res.logits).max())
    print("max |Network logits - batch-BN engine logits| = %.3g" % err)
    assert err <= 2e-4


# ---------------------------------------------------------------------------------------------
# gradients against float64 autograd of cnn_ref
# ---------------------------------------------------------------------------------------------
def _ctc_chain(spec, w, B, T, rng):
    """callable(features on the GPU) -> dfeatures of the real chain: chiron_rnn_train_forward, chiron_ctc_loss, chiron_rnn_train_backward."""
    torch = _torch()
    sl = tc.ragged_seq_len(B, T, rng)
    f, _, _ = tc.ctc_dlogits(sl, rng, T)

    def chain(fea):
        dev = fea.device
        p = torch.from_numpy(tc.flat_params(spec, w)).to(dev)
        sl_d = torch.from_numpy(sl).to(dev)
        logits, tape, ws = train.rnn_forward(spec, p, fea, sl_d)
        _, dfeat = train.rnn_backward(spec, p, fea, sl_d, f(logits).contiguous(), tape, ws, True)
        return dfeat
    return chain


@pytest.mark.parametrize("source", ["random", "ctc"])
@pytest.mark.parametrize("case", cc.GRAD_CASES, ids=lambda c: "%s-B%d-L%d" % c)
def test_gradients_against_float64_autograd(built, case, source):
    kind, B, L = case
    spec, w, x, g = cc.grad_case(kind, B, L)
    if source == "ctc":
        g = _ctc_chain(spec, w, B, spec.output_len(L), np.random.default_rng(B + L))
    _, _, dp, g_used, masks = cc.hip_run(spec, w, x, g)
    assert np.abs(g_used).max() > 0
    label = "%s B=%d L=%d %s" % (kind, B, L, source)
    rows = cc.gradient_rows(spec, w, x, dp, g_used, masks, GRAD_FACTOR, label)
    assert set(rows) == set(cnn_ref.trainable_names(spec))
    cc.assert_rows(rows, label, GRAD_FACTOR)


@pytest.mark.parametrize("case", cc.CAP_GRAD_CASES, ids=lambda c: "%s-B%d-L%d" % c)
def test_gradients_past_the_reduction_caps(built, case):
    """Sites of more than 131 072 rows (cnn_train_cases.CAP_GRAD_CASES): the row reductions run 512 capped slices and cg_dw_kernel 64
    capped splits, each with a ragged last one.  The forward (features, every site's moments) and every gradient are held to the bar
    of the cases above, with the factors the same ensemble rule gave for these two cases on the CPU before any HIP result
    (profiles/cnn_grad_accuracy.json, "factor_cap": forward 4, gradients 4.4321 from a largest ratio of 2.955 at dna B 330)."""
    kind, B, L = case
    spec, w, x, g = cc.grad_case(kind, B, L)
    fea, mom, dp, g_used, masks = cc.hip_run(spec, w, x, g)
    label = "%s B=%d L=%d" % (kind, B, L)
    cc.assert_rows(cc.forward_rows(spec, w, x, fea, mom, cc.CAP_FWD_FACTOR), label + " fwd", cc.CAP_FWD_FACTOR)
    rows = cc.gradient_rows(spec, w, x, dp, g_used, masks, cc.CAP_GRAD_FACTOR, label)
    assert set(rows) == set(cnn_ref.trainable_names(spec))
    cc.assert_rows(rows, label, cc.CAP_GRAD_FACTOR)
    # the slices are summed in slice order: two identical calls, the same bits
    fea2, mom2, dp2, _ = cc.hip_forward_backward(spec, w, x, g)
    assert fea2.tobytes() == fea.tobytes() and mom2.tobytes() == mom.tobytes() and dp2.tobytes() == dp.tobytes()


# one row per topology also takes the real chain's dfeatures: T >= 18 there, so that labels fit (rna_model3 at 121 has 18 frames)
GEOMETRY_CTC = [("rna", 9, 123), ("rna_model2", 9, 122), ("rna_model3", 9, 121), ("dna", 5, 33)]
GEOMETRY_RUNS = [(case, "random") for case in cc.GEOMETRY_GRAD_CASES] + [(case, "ctc") for case in GEOMETRY_CTC]


@pytest.mark.parametrize("case,source", GEOMETRY_RUNS, ids=lambda v: v if isinstance(v, str) else "%s-B%d-L%d" % v)
def test_forward_and_gradients_across_window_geometry(built, case, source):
    """Every 'SAME' left pad of the strided sites and windows of 1 to 3 frames (cnn_train_cases.GEOMETRY_GRAD_CASES): the pad enters
    cg_conv_kernel (forward, and dX, where it decides which taps divide by the stride), cg_dw_kernel and the cg_rank1 kernels through
    CgRows; the short windows have most taps in the padding and walk cg_dw_kernel's (rb, rt) over several windows per k-tile.  The
    forward (features, every site's moments) and every gradient, under the implementation's own masks once they are shown
    legitimate, are held to the bar of the cases above with the factors the same ensemble rule gave for these cases on the CPU
    before any HIP result (profiles/cnn_grad_accuracy.json, "factor_geometry": forward 4, gradients 6.6315 from a largest ratio of
    4.421 at dna B 33 L 3).  tests/test_cnn_train_cpu.py shows that this bar rejects a padding moved by one frame at every case.
    What the sweep found: the window walk is right everywhere; rna B 9 L 124 had res_layer1/branch1/conv1/weights at 12.7 x e32 (err
    2.35e-5), because the BN backward took the recomputed xhat for centred while it is off by the rounding of the tape's float32
    mean, which that site (raw signal in, a filter weight of 8e-5) amplifies 150-fold.  cg_bn_bwd_* now measure and remove xhat's
    mean: 5.87 x e32 there (err 1.09e-5; e32 of that one-channel tensor happens to be low, 1.85e-6), at most 1.9 everywhere else."""
    kind, B, L = case
    assert case in cc.GEOMETRY_GRAD_CASES
    spec, w, x, g = cc.grad_case(kind, B, L)
    T = spec.output_len(L)
    if source == "ctc":
        assert T >= 18
        g = _ctc_chain(spec, w, B, T, np.random.default_rng(B + L))
    fea, mom, dp, g_used, masks = cc.hip_run(spec, w, x, g)
    assert fea.shape == (B, T, 256) and np.abs(g_used).max() > 0
    label = "%s B=%d L=%d %s" % (kind, B, L, source)
    cc.assert_rows(cc.forward_rows(spec, w, x, fea, mom, cc.GEOMETRY_FWD_FACTOR), label + " fwd", cc.GEOMETRY_FWD_FACTOR)
    rows = cc.gradient_rows(spec, w, x, dp, g_used, masks, cc.GEOMETRY_GRAD_FACTOR, label)
    assert set(rows) == set(cnn_ref.trainable_names(spec))
    cc.assert_rows(rows, label, cc.GEOMETRY_GRAD_FACTOR)


# ---------------------------------------------------------------------------------------------
# exact properties
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cc.SPECS)
def test_exact_properties(built, kind):
    spec = cc.spec_of(kind)
    w = ca.synthetic_weights(spec, seed=7)
    B, L = 9, 150
    x = ca.synthetic_signal(B, L, seed=21)
    rng = np.random.default_rng(4)
    g = rng.normal(size=(B, spec.output_len(L), 256)).astype(np.float32)
    fea, mom, dp, _ = cc.hip_forward_backward(spec, w, x, g)
    # two runs: the same bits
    fea2, mom2, dp2, _ = cc.hip_forward_backward(spec, w, x, g)
    assert fea.tobytes() == fea2.tobytes() and mom.tobytes() == mom2.tobytes() and dp.tobytes() == dp2.tobytes()
    # the statistics' slots get exactly 0, every trainable tensor something
    for name, v in cc.named(spec, dp).items():
        assert (not v.any()) == name.endswith(("pop_mean", "pop_var")), name
    assert np.isfinite(dp).all()
    # no gradient in, none out
    _, _, dp0, _ = cc.hip_forward_backward(spec, w, x, np.zeros_like(g))
    assert not dp0.any()
    # linear in dfeatures, bit for bit under a power of two (normal(0, 1) gradients: nothing near the subnormal range)
    _, _, dp_2, _ = cc.hip_forward_backward(spec, w, x, 2.0 * g)
    assert dp_2.tobytes() == (2.0 * dp).tobytes()
    # the pop_mean / pop_var slots of params are not read
    w_other = dict(w)
    for name in w:
        if name.endswith("pop_mean"):
            w_other[name] = np.asarray(w[name]) + 3.0
        if name.endswith("pop_var"):
            w_other[name] = np.asarray(w[name]) * 7.0
    fea3, _, dp3, _ = cc.hip_forward_backward(spec, w_other, x, g)
    assert fea3.tobytes() == fea.tobytes() and dp3.tobytes() == dp.tobytes()
    # window borders: the same windows in reversed batch order give the reversed features, and moments and gradients that are sums
    # over the same terms in another order: each run is held to the float64 reference of its own order under the bars above (a tap
    # that read its neighbouring window would read another neighbour now), and the two to each other within twice that
    xr, gr = x[::-1].copy(), g[::-1].copy()
    fea_r, mom_r, dp_r, _, masks_r = cc.hip_run(spec, w, xr, gr)
    cc.assert_rows(cc.forward_rows(spec, w, xr, fea_r, mom_r, FWD_FACTOR), "%s reversed fwd" % kind, FWD_FACTOR)
    cc.assert_rows(cc.gradient_rows(spec, w, xr, dp_r, gr, masks_r, GRAD_FACTOR, "%s reversed" % kind), "%s reversed grad" % kind, GRAD_FACTOR)
    rows = cc.forward_rows(spec, w, x, fea, mom, FWD_FACTOR)
    f64 = np.linalg.norm(fea.astype(np.float64))
    assert np.linalg.norm(fea_r[::-1].astype(np.float64) - fea) <= (2 * FWD_FACTOR * rows["features"]["e32_rel"] + FLOOR) * f64
    m, m_r = cc.named(spec, mom), cc.named(spec, mom_r)
    for name in m:
        if name.endswith(("pop_mean", "pop_var")):
            site = name[:-len("_bn/pop_mean")] if name.endswith("pop_mean") else name[:-len("_bn/pop_var")]
            r = rows[site + (" mean" if name.endswith("pop_mean") else " var")]
            assert np.linalg.norm(m_r[name].astype(np.float64) - m[name]) <= (2 * FWD_FACTOR * r["e32_rel"] + FLOOR) * r["norm"], name


# ---------------------------------------------------------------------------------------------
# autograd module
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dna", "rna_model3"])
def test_network_autograd_equals_the_two_seams_chained_by_hand(built, kind):
    torch = _torch()
    from chiron_amd import ctc
    spec = cc.spec_of(kind)
    w = ca.synthetic_weights(spec, seed=7)
    B, L = 12, 200
    T = spec.output_len(L)
    rng = np.random.default_rng(17)
    x = ca.synthetic_signal(B, L, seed=8)
    sl = tc.ragged_seq_len(B, T, rng)
    _, lab, ll = tc.ctc_dlogits(sl, rng, T)
    dev = torch.device("cuda", 0)
    net = train.Network(spec, w)
    assert isinstance(net, torch.nn.Module) and [n for n, _ in net.named_parameters()] == ["flat"]
    assert list(net.named_views()) == list(spec.blob_layout())
    blob = spec.pack(w)
    assert net.flat.detach().cpu().numpy().tobytes() == blob.tobytes()
    x_d, sl_d = torch.from_numpy(x).to(dev), torch.from_numpy(sl).to(dev)
    lab_d, ll_d = torch.from_numpy(lab).to(dev), torch.from_numpy(ll).to(dev)
    net.train()
    logits = net(x_d, sl_d)
    ctc.CTCLoss.apply(logits, sl_d, lab_d, ll_d).sum().backward()
    # by hand, from the same starting weights
    n_cnn = train.cnn_params_range(spec)[1]
    p = torch.from_numpy(blob).to(dev)
    fea, mom, ctape, cws = train.cnn_forward(spec, p[:n_cnn], x_d)
    logits2, rtape, rws = train.rnn_forward(spec, p[n_cnn:], fea, sl_d)
    _, dlogits = ctc.ctc_loss(logits2, sl_d, lab_d, ll_d, want_grad=True)
    d_rnn, dfeat = train.rnn_backward(spec, p[n_cnn:], fea, sl_d, dlogits.contiguous(), rtape, rws, True)
    d_cnn = train.cnn_backward(spec, p[:n_cnn], x_d, dfeat, ctape, cws)
    assert logits.detach().cpu().numpy().tobytes() == logits2.cpu().numpy().tobytes()
    grad = net.flat.grad.cpu().numpy()
    assert grad[:n_cnn].tobytes() == d_cnn.cpu().numpy().tobytes() and grad[n_cnn:].tobytes() == d_rnn.cpu().numpy().tobytes()
    # the moving averages moved by 0.99 / 0.01 (cnn.py:153-156), nothing else did
    idx = net.stat_index.cpu().numpy()
    now = net.flat.detach().cpu().numpy()
    want = (0.99 * torch.from_numpy(blob)[idx] + (1.0 - 0.99) * mom.cpu()[idx]).numpy()
    assert np.array_equal(now[idx], want)
    rest = np.ones(blob.size, dtype=bool)
    rest[idx] = False
    assert now[rest].tobytes() == blob[rest].tobytes() and not grad[idx].any()
    sw = net.state_weights()
    assert list(sw) == list(spec.blob_layout()) and spec.pack(sw).tobytes() == now.tobytes()
    # eval(): the same logits, no movement
    net.eval()
    net(x_d, sl_d)
    assert net.flat.detach().cpu().numpy().tobytes() == now.tobytes()


# ---------------------------------------------------------------------------------------------
# train end to end
# ---------------------------------------------------------------------------------------------
def _write_pairs(folder, rng, n_files, n_sig=6000):
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


STEPS, REPORT = 40, 2


def _run_train(tmp_path, extra):
    rng = np.random.default_rng(13)
    data = str(tmp_path / "data")
    _write_pairs(data, rng, n_files=20)
    out = str(tmp_path / "trained")
    cmd = [sys.executable, "-m", "chiron_amd.entry", "train", "-i", data, "-o", out, "-s", "400", "-b", "32", "-t", "4e-3", "-x", str(STEPS),
           "--report-every", str(REPORT), "--seed", "5"] + extra
    r = subprocess.run(["timeout", "-k", "10", "540"] + cmd, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rep = json.load(open(os.path.join(out, "train.json")))
    losses = [x["train_loss"] for x in rep["reports"]]
    print("train loss per report:", " ".join("%.4g" % v for v in losses))
    assert len(losses) >= 10 and rep["windows"] >= 200 and rep["global_step"] == STEPS
    assert np.isfinite(losses).all()
    assert np.mean(losses[-5:]) < np.mean(losses[:5])
    report = str(tmp_path / "report.json")
    v = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "chiron_amd.entry", "validate", "-i", data, "-m", out, "-l", "400",
                        "-b", "16", "--beam", "0", "-o", report], cwd=ROOT, capture_output=True, text=True)
    assert v.returncode == 0, v.stderr[-2000:]
    summary = json.load(open(report))["summary"]
    assert summary["windows"] == labelled.read_raw_data_sets(data, seq_length=400).event.shape[0]
    assert summary["loss_mean_reference"] is not None and np.isfinite(summary["loss_mean_reference"]), summary
    return out


def test_train_from_scratch_with_batch_bn_end_to_end(built, tmp_path):
    """A few tens of steps from init_weights prove plumbing, not learning: every CNN and RNN variable moves, the training loss
    falls, the folder loads as a batch-BN model and `validate` scores it."""
    out = _run_train(tmp_path, [])
    spec, w, config = ca.load_model(out)
    assert spec.bn_mode == "batch" and spec.to_dict() == ca.dna_default_spec("batch").to_dict() and config["opt_method"] == "Adam"
    w0 = train.init_weights(spec, 5)
    for name in spec.blob_layout():
        same = np.asarray(w[name]).tobytes() == np.asarray(w0[name]).tobytes()
        assert same == name.endswith(("pop_mean", "pop_var")), name     # not stored: load_model fills the statistics with 0 / 1


def test_train_from_a_population_bn_model_end_to_end(built, tmp_path):
    model = os.path.join(ROOT, "chiron_amd", "model", "DNA_default")
    out = _run_train(tmp_path, ["-m", model, "--synthetic-weights"])
    spec0, w0, _ = ca.load_model(model, allow_synthetic=True)
    spec, w, _ = ca.load_model(out)
    assert spec.bn_mode == "population" and spec.to_dict() == spec0.to_dict()
    canon0 = spec0.canonical_weights(w0)
    for name in spec.blob_layout():
        assert np.asarray(w[name]).tobytes() != np.asarray(canon0[name], dtype=np.float32).tobytes(), name   # pop_* moved too
