"""Shared set-up of the CNN training tests: the four topologies, the HIP calls through the ABI, and the accuracy rows.

The bar has the form of tests/train_cases.py: per tensor ||g - g64|| <= FACTOR * e32 + FLOOR * ||g64||, g64 from float64 autograd of
tests/cnn_ref.py and e32 the error of the same restatement run in float32 on the CPU.  FACTOR is derived in test_gpu_cnn_train.py.
Gradients are compared under FIXED ReLU masks, the implementation's own (tests/cnn_ref.py, `masks`), after `flipped_masks` has
checked that those masks are legitimate."""
import numpy as np
import torch

import chiron_amd as ca
from chiron_amd import train

import cnn_ref
from train_cases import FLOOR

SPECS = ["dna", "rna", "rna_model2", "rna_model3"]


def spec_of(kind, bn_mode="population"):
    if kind == "dna":
        return ca.dna_default_spec(bn_mode)
    if kind == "rna":
        return ca.rna_default_spec(bn_mode)
    return ca.rna_head_spec(kind, bn_mode)


def full_segment(kind):
    return 400 if kind == "dna" else 500


def cnn_params(spec, weights):
    first, n = train.cnn_params_range(spec)
    return spec.pack(weights)[first:first + n].copy()


def named(spec, flat):
    return {name: flat[off:off + int(np.prod(shape))].reshape(shape) for name, (off, shape) in train.cnn_param_layout(spec).items()}


def hip_forward(spec, weights, signal):
    """-> (features, moments flat, tape, ws, device params, device signal) through chiron_cnn_train_forward."""
    dev = torch.device("cuda", 0)
    p = torch.from_numpy(cnn_params(spec, weights)).to(dev)
    x = torch.from_numpy(np.ascontiguousarray(signal, dtype=np.float32)).to(dev)
    fea, mom, tape, ws = train.cnn_forward(spec, p, x)
    return fea, mom, tape, ws, p, x


def hip_run(spec, weights, signal, dfeatures):
    """-> (features, moments flat, dparams flat, dfeatures used, {relu name: bool mask}) as numpy arrays; dfeatures: array, or
    callable(features on the GPU) -> device tensor.  The masks are the tape's ReLU outputs > 0: what the backward multiplies by."""
    fea, mom, tape, ws, p, x = hip_forward(spec, weights, signal)
    g = dfeatures(fea) if callable(dfeatures) else torch.from_numpy(np.ascontiguousarray(dfeatures, dtype=np.float32)).to(fea.device)
    dp = train.cnn_backward(spec, p, x, g.contiguous(), tape, ws)
    torch.cuda.synchronize()
    masks = {k: (v > 0).cpu().numpy() for k, v in train.cnn_tape_relu(spec, tape, x.shape[0], x.shape[1]).items()}
    return fea.cpu().numpy(), mom.cpu().numpy(), dp.cpu().numpy(), g.cpu().numpy(), masks


def hip_forward_backward(spec, weights, signal, dfeatures):
    return hip_run(spec, weights, signal, dfeatures)[:4]


def row(got, ref, f32, factor):
    norm = float(np.linalg.norm(ref))
    err = float(np.linalg.norm(np.asarray(got, dtype=np.float64) - ref))
    e32 = float(np.linalg.norm(np.asarray(f32, dtype=np.float64) - ref))
    return {"err_rel": err / max(norm, 1e-300), "e32_rel": e32 / max(norm, 1e-300), "norm": norm,
            "ratio": err / e32 if e32 > 0 else (0.0 if err == 0 else float("inf")), "ok": bool(err <= factor * e32 + FLOOR * norm)}


def forward_rows(spec, weights, signal, fea, mom_flat, factor):
    """features and every site's moments against the float64 restatement, e32 from the float32 one."""
    f64, m64 = cnn_ref.forward(signal, spec, weights, torch.float64)
    f32, m32 = cnn_ref.forward(signal, spec, weights, torch.float32)
    got = named(spec, mom_flat)
    rows = {"features": row(fea, f64, f32, factor)}
    for site in m64:
        rows[site + " mean"] = row(got[site + "_bn/pop_mean"], m64[site][0], m32[site][0], factor)
        rows[site + " var"] = row(got[site + "_bn/pop_var"], m64[site][1], m32[site][1], factor)
    return rows


# A ReLU mask of the implementation may differ from the sign of the float64 pre-activation only where that pre-activation is within
# float32 rounding of 0.  The forward test holds every site to a few e32 ~ 1e-6 .. 1e-5 of its rms in L2; an element's own error can
# exceed the L2 average, so the tolerance is ten times the upper end of that, relative to the site's rms, and such elements must be
# rare (a float32 value lands within 1e-4 rms of 0 with probability of the order of 1e-4).
FLIP_TOL = 1e-4
FLIP_SHARE = 1e-3


def flipped_masks(masks, pre64):
    """{relu name: (elements whose mask is not the float64 sign, largest |float64 pre-activation| among them over the site's rms)}."""
    out = {}
    for name, m in masks.items():
        p = pre64[name]
        diff = m != (p > 0)
        rms = float(np.sqrt(np.mean(p * p)))
        out[name] = (int(diff.sum()), float(np.abs(p[diff]).max() / rms) if diff.any() else 0.0, diff.size)
    return out


def assert_masks_legitimate(masks, pre64, label):
    total = 0
    for name, (n, worst, size) in flipped_masks(masks, pre64).items():
        total += n
        if n:
            print("%s %-32s %d of %d mask elements differ from the float64 sign, largest |pre| / rms %.3g" % (label, name, n, size, worst))
        assert worst <= FLIP_TOL and n <= FLIP_SHARE * size, (label, name, n, worst)
    return total


def gradient_rows(spec, weights, signal, dparams_flat, g_used, masks, factor, label=""):
    """Per trainable tensor: the HIP gradient against float64 autograd of cnn_ref under the SAME masks, e32 from the float32 run under
    the same masks; asserts first that the masks are the float64 signs except within rounding of 0."""
    pre = {}
    _, g64 = cnn_ref.gradients(signal, spec, weights, g_used, torch.float64, masks=masks, pre=pre)
    assert_masks_legitimate(masks, pre, label)
    _, g32 = cnn_ref.gradients(signal, spec, weights, g_used, torch.float32, masks=masks)
    got = named(spec, dparams_flat)
    return {name: row(got[name], g64[name], g32[name], factor) for name in g64}


def print_rows(rows, label):
    for name, r in rows.items():
        print("%s %-44s err %.3g  e32 %.3g  err/e32 %.3g" % (label, name, r["err_rel"], r["e32_rel"], r["ratio"]))


def assert_rows(rows, label, factor):
    print_rows(rows, label)
    bad = [n for n, r in rows.items() if not r["ok"]]
    worst = max(rows.items(), key=lambda kv: kv[1]["ratio"] if kv[1]["norm"] > 0 else 0.0)
    assert not bad, "%s: beyond %g x e32 + %g ||g64||: %s (worst %s: %.3g)" % (label, factor, FLOOR, bad, worst[0], worst[1]["ratio"])


# the gradient cases: (topology, batch, segment length); test, ensemble tool and profiles/cnn_grad_accuracy.json share them
# the full-segment cases have more than 2048 rows at every site: several slices in every row reduction and in cg_dw_kernel's split;
# dna B64 has 25 600 rows (13 dW slices, 100 reduction slices)
GRAD_CASES = [(kind, B, L) for kind in SPECS for B, L in ((7, 120), (16, full_segment(kind)))] + [("dna", 64, 400)]


def grad_case(kind, B, L):
    """-> (spec, weights, signal, random dfeatures) of one gradient case, seeded by the case alone."""
    spec = spec_of(kind)
    w = ca.synthetic_weights(spec, seed=7)
    x = ca.synthetic_signal(B, L, seed=5)
    rng = np.random.default_rng(1000 * B + L)
    g = rng.normal(size=(B, spec.output_len(L), spec.blocks[-1]["out"])).astype(np.float32)
    return spec, w, x, g


# Past the caps of the row reductions of csrc/cnn_grad.hip (CG_MAX_SLICES slices of CG_SLICE_ROWS rows, CG_DW_MAX_SPLIT dW splits of
# CG_DW_SPLIT_ROWS rows: both 131 072 rows), seeded by grad_case like the cases above; tests/test_cnn_train_cpu.py pins them to the
# constants.  The smallest shapes that cross each cap with a ragged last slice:
#   rna B 300 L 500  the trainer's default batch: conv2a of block 1 reads the signal (ci == 1) at 150 000 rows, 512 slices of 293 rows
#                    (the last 277) in cg_sum_kernel, cg_bn_bwd_sum_kernel and cg_rank1_dw_kernel; the stride-5 sites have 30 000 rows
#   dna B 330 L 400  every site has 132 000 rows: 512 slices of 258 rows (the last 162), 64 dW splits of 2064 rows (the last 1968)
CAP_GRAD_CASES = [("rna", 300, 500), ("dna", 330, 400)]
# the factors of the bar for these cases: max(4, 1.5 x the largest max / median) of the float32 ensemble over them, run on the CPU before
# any HIP result (tools/cnn_grad_accuracy.py -> "factor_cap" of profiles/cnn_grad_accuracy.json; tests/test_cnn_train_cpu.py compares)
CAP_FWD_FACTOR = 4.0
CAP_GRAD_FACTOR = 4.4321


# Window geometry: every left pad of TF 'SAME' at every strided site, and windows of 1 to 3 frames.  left = pad_total // 2 depends on
# L mod stride, and GRAD_CASES above reach one residue per topology (120 and 500 are multiples of 5; 120 and 150 are 1 and 3 mod 7).
# B keeps about a hundred rows or more at every site: with a handful of rows one rounding flip is the whole of e32 (tests/f16_cases.py
# records the same lesson).  tests/test_cnn_train_cpu.py pins what these rows reach.
#   rna         conv2b of block 1 (k 13, stride 5): L = 121 .. 124 are residues 1 .. 4, left pads 6, 5, 5, 4; T = 25, so 225 rows at the
#               strided sites: one whole and one partial 128-row tile, window borders inside both
#   rna_model2  stem (k 9, stride 5): left pads 4, 3, 3, 2
#   rna_model3  stem (k 14, stride 7): residues 2, 4, 5, 6, 0; with 120 and 150 above, every residue
#   short       windows shorter than the strided kernel (L < k, most taps in the padding), T = 1 and 2
#   dna         T = 1, 2, 3 and 33 at stride 1: at T = 1 both outer taps of every k = 3 convolution lie in the padding
GEOMETRY_GRAD_CASES = ([("rna", 9, L) for L in (121, 122, 123, 124)] + [("rna_model2", 9, L) for L in (121, 122, 123, 124)] +
                       [("rna_model3", 9, L) for L in (121, 123, 124, 125, 126)] +
                       [("rna", 101, 3), ("rna", 40, 7), ("rna_model2", 101, 4), ("rna_model3", 60, 8)] +
                       [("dna", 101, 1), ("dna", 48, 2), ("dna", 33, 3), ("dna", 5, 33)])
# the factors of the bar for these cases, by the rule of the cap cases: the float32 ensemble over exactly these cases, run on the CPU
# before any HIP result (tools/cnn_grad_accuracy.py --cases geometry -> "factor_geometry" of profiles/cnn_grad_accuracy.json): the
# forward's largest max / median is 1.548 (dna B 101 L 1), the gradients' 4.421 (dna B 33 L 3)
GEOMETRY_FWD_FACTOR = 4.0
GEOMETRY_GRAD_FACTOR = 6.6315


def site_strides(spec):
    """[(site, k, stride)] of every convolution site, in the order of spec._sites(): the stem and a block's branch1 and conv2b carry
    a stride, conv2a and conv2c run at stride 1."""
    out = []
    for site, (_, k, _, _), _ in spec._sites():
        leaf = site.split("/")[-1]
        if leaf in ("conv2a", "conv2c"):
            out.append((site, k, 1))
        else:
            out.append((site, k, spec.stem["stride"] if site == spec.STEM_SITE
                        else next(b["stride"] for b in spec.blocks if site.startswith(b["name"] + "/"))))
    return out


def site_windows(spec, L):
    """[(site, k, stride, frames the site reads per window)], the same walk as site_rows."""
    out, t = [], L
    for site, k, stride in site_strides(spec):
        out.append((site, k, stride, t))
        leaf = site.split("/")[-1]
        if leaf == "conv2b" or site == spec.STEM_SITE:
            t = -(-t // stride)
    return out


def site_rows(spec, B, L):
    """[(site, ci, k, rows)]: the rows = B * output frames of every convolution site, the 'SAME' walk of csrc/model_layout.h restated:
    both branches of a block read the block's input, branch1 and conv2b carry its stride, conv2c runs at its output length."""
    out, t = [], L
    for site, (_, k, ci, _), _ in spec._sites():
        leaf = site.split("/")[-1]
        if leaf == "conv2a":
            out.append((site, ci, k, B * t))
            continue
        if leaf == "conv2c":
            out.append((site, ci, k, B * t))
            continue
        stride = spec.stem["stride"] if site == spec.STEM_SITE else next(b["stride"] for b in spec.blocks if site.startswith(b["name"] + "/"))
        tout = -(-t // stride)
        out.append((site, ci, k, B * tout))
        if leaf != "conv1" or site == spec.STEM_SITE:      # the stem and conv2b hand their output length on; branch1 (conv1) does not
            t = tout
    return out
