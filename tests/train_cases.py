"""Shared set-up of the training tests: cases, the HIP calls, and the accuracy yardstick.

The bar of the gradient tests is not derived from the code under test: the float64 restatement (tests/rnn_ref.py) gives the exact
gradients g64; the SAME restatement run in float32 on the CPU gives, per tensor, the relative L2 error e32 of one float32
realisation; the HIP gradient must satisfy  ||g - g64|| <= FACTOR * e32 * ||g64|| + 1e-6 * ||g64||,  FACTOR = 4 for the different
accumulation orders (blocked split-K over T * B rows against torch's order; the repository's ensemble study found float32
realisations of one formula 2 .. 3 x apart between orders, profiles/r06_parity_dist_*)."""
import os
import re

import numpy as np
import torch

import chiron_amd as ca
from chiron_amd import train

import rnn_ref

FACTOR = 4.0
FLOOR = 1e-6


def specs():
    return {"dna-stack": ca.dna_default_spec(), "rna-multi": ca.rna_default_spec()}


def ragged_seq_len(B, T, rng):
    sl = rng.integers(2, T + 1, size=B)
    sl[:3] = (0, 1, T)
    return sl.astype(np.int32)[:B]


def geometry_seq_len(B, T, rng):
    """Lengths uniform in 0 .. T with rows 0 to 2 set to (0, 1, T): what ragged_seq_len cannot draw at T = 1."""
    sl = rng.integers(0, T + 1, size=B)
    sl[:3] = (0, 1, T)
    return sl.astype(np.int32)[:B]


def oracle_features(spec, weights, B, segment_len, rng):
    """The float64 oracle's own CNN features [B, T, C] of seeded synthetic signal."""
    from oracle import nn_oracle
    x = ca.synthetic_signal(B, segment_len, seed=int(rng.integers(1, 1 << 30))).astype(np.float64)
    return x, nn_oracle.cnn_forward(x, spec.to_dict(), {k: np.asarray(v, dtype=np.float64) for k, v in weights.items()})


def random_features(B, T, C, rng):
    """Post-ReLU-like features: non-negative, about half of them zero, as the CNN's last block leaves them."""
    return np.maximum(rng.normal(0.0, 1.0, size=(B, T, C)), 0.0).astype(np.float32)


def flat_params(spec, weights):
    first, n = train.params_range(spec)
    return spec.pack(weights)[first:first + n].copy()


def hip_forward_backward(spec, weights, fea, seq_len, dlogits, want_dfeatures=True):
    """-> (logits, {name: grad}, dfeatures, flat dparams) as numpy arrays, through the two ABI entry points."""
    dev = torch.device("cuda", 0)
    p = torch.from_numpy(flat_params(spec, weights)).to(dev)
    x = torch.from_numpy(np.ascontiguousarray(fea, dtype=np.float32)).to(dev)
    sl = torch.from_numpy(np.ascontiguousarray(seq_len, dtype=np.int32)).to(dev)
    logits, tape, ws = train.rnn_forward(spec, p, x, sl)
    g = dlogits(logits) if callable(dlogits) else dlogits
    g_d = torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32)).to(dev) if not torch.is_tensor(g) else g
    dparams, dfeat = train.rnn_backward(spec, p, x, sl, g_d.contiguous(), tape, ws, want_dfeatures)
    torch.cuda.synchronize()
    flat = dparams.cpu().numpy()
    named = {name: flat[off:off + int(np.prod(shape))].reshape(shape) for name, (off, shape) in train.param_layout(spec).items()}
    return logits.cpu().numpy(), named, (dfeat.cpu().numpy() if want_dfeatures else None), flat, g_d.cpu().numpy()


def rel_l2(a, ref):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - ref) / max(np.linalg.norm(ref), 1e-300))


def accuracy(spec, weights, fea, seq_len, dlogits, hip_out=None):
    """Per tensor (every named parameter + 'dfeatures'): err (HIP against float64), e32 (float32 restatement against float64),
    norm of the float64 gradient, and whether the bar holds.  dlogits: array, or callable(logits tensor on the GPU) -> array / tensor.
    hip_out: a dict that receives the HIP run's flat dparams, dfeatures, logits and named gradients."""
    logits, named, dfeat, flat, g_used = hip_forward_backward(spec, weights, fea, seq_len, dlogits)
    if hip_out is not None:
        hip_out.update(flat=flat, dfeatures=dfeat, logits=logits, named=named)
    _, g64, dx64 = rnn_ref.gradients(fea, seq_len, spec, weights, g_used, torch.float64)
    _, g32, dx32 = rnn_ref.gradients(fea, seq_len, spec, weights, g_used, torch.float32)
    rows = {}
    for name in list(g64) + ["dfeatures"]:
        ref = dx64 if name == "dfeatures" else g64[name]
        f32 = dx32 if name == "dfeatures" else g32[name]
        hip = dfeat if name == "dfeatures" else named[name]
        norm = float(np.linalg.norm(ref))
        err = float(np.linalg.norm(hip.astype(np.float64) - ref))
        e32 = float(np.linalg.norm(f32 - ref))
        rows[name] = {"err_rel": err / max(norm, 1e-300), "e32_rel": e32 / max(norm, 1e-300), "norm": norm,
                      "ratio": err / e32 if e32 > 0 else (0.0 if err == 0 else float("inf")),
                      "ok": bool(err <= FACTOR * e32 + FLOOR * norm)}
    return rows


# Past the caps of the reductions over the M = T * BP rows (BP: the batch padded to 16), csrc/rnn_grad.hip; (kind, B, T, what).
# The smallest shapes that cross each constant with a ragged last slice; tests/test_train_cpu.py pins them to the constants.
#   "head"   M = 48 * 688 = 33 024 > RG_HEAD_WG * RG_HEAD_ROWS: 256 head workgroups of 129 rows, no multiple of 16, so every
#            workgroup's range straddles frames and takes in the padding rows 683 .. 687
#   "split"  M = 97 * 1376 = 133 472 > RG_MAX_SPLIT * RG_SPLIT_ROWS: 64 capped slices; the GEMM's chunk is 2096 (last slice 1424),
#            the column sum's 2086, dWh's (R = M - BP = 132 096) 2064 exactly; 522 rows per head workgroup
CAP_CASES = [("dna-stack", 683, 48, "head"), ("rna-multi", 683, 48, "head"), ("dna-stack", 1370, 97, "split")]


def cap_case(kind, B, T):
    """-> (spec, weights, features, seq_len, random dlogits) of one CAP_CASES entry, seeded as test_gradients_against_float64_autograd."""
    spec = specs()[kind]
    rng = np.random.default_rng(100 + T)
    fea = random_features(B, T, 256, rng)
    sl = ragged_seq_len(B, T, rng)
    return spec, ca.synthetic_weights(spec, seed=7), fea, sl, rng.normal(size=(B, T, 5)).astype(np.float32)


# Tiny and odd frame counts, (kind, B, T): T = 1 (no recurrent step at all: chiron_rnn_train_backward zeroes dWh instead of running a
# GEMM over M - BP = 0 rows), 2 and 3 frames, and T = 17 and 33, multiples of nothing in rg_lstm_fwd / rg_lstm_bwd or the 16-row k-tile.
# B keeps about a hundred rows or more (T * B) and is off the kernels' 16-row multiple except at 48.
GEOMETRY_CASES = [(kind, B, T) for kind in ("dna-stack", "rna-multi") for B, T in ((101, 1), (48, 2), (33, 3), (7, 17), (5, 33))]


def geometry_case(kind, B, T):
    """-> (spec, weights, post-ReLU-like features, seq_len, random dlogits) of one GEOMETRY_CASES entry, seeded by the case alone."""
    spec = specs()[kind]
    rng = np.random.default_rng(1000 * B + T)
    fea = random_features(B, T, 256, rng)
    sl = geometry_seq_len(B, T, rng)
    return spec, ca.synthetic_weights(spec, seed=7), fea, sl, rng.normal(size=(B, T, 5)).astype(np.float32)


def kernel_constants(hip_file, names):
    """{name: value} of `constexpr int` constants, read out of chiron_amd/csrc/<hip_file>."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "chiron_amd", "csrc", hip_file)).read()
    decl = "\n".join(re.findall(r"^constexpr int [^;]*;", src, flags=re.M))
    out = {}
    for name in names:
        found = re.findall(r"\b%s = (\d+)\b" % name, decl)
        assert len(found) == 1, (hip_file, name, found)
        out[name] = int(found[0])
    return out


def slices(rows, n, chunk):
    """[(begin, end)] of the n slices of a row reduction as every kernel forms them: begin = z * chunk, end = min(rows, begin + chunk)."""
    return [(z * chunk, min(rows, (z + 1) * chunk)) for z in range(n)]


def assert_slices_tile(rows, n, chunk):
    """No slice is empty, and the slices tile [0, rows) (they are contiguous by construction)."""
    assert n >= 1 and (n - 1) * chunk < rows <= n * chunk, (rows, n, chunk)


def ctc_dlogits(seq_len, rng, T):
    """callable(logits) -> the real chiron_ctc_loss gradient for random labels that fit every row."""
    from chiron_amd import ctc
    B = len(seq_len)
    ll = np.array([min(int(n) // 3, 40) for n in seq_len], dtype=np.int32)
    lab = rng.integers(0, 4, size=(B, max(int(ll.max()), 1))).astype(np.int32)

    def f(logits):
        dev = logits.device
        _, grad = ctc.ctc_loss(logits, torch.from_numpy(np.ascontiguousarray(seq_len, dtype=np.int32)).to(dev),
                               torch.from_numpy(lab).to(dev), torch.from_numpy(ll).to(dev), want_grad=True)
        return grad
    return f, lab, ll
