"""The network of the fp32 engine restated in numpy, stage by stage, in the kernel form each stage runs.

The stages tests/test_gpu_fp32_ref.py judges: "cnn" (signal -> features), one stage per LSTM layer ("rnn1" .. "rnn<n>": ANY input
of the layer -> its output, so that the float64 layer can be applied to the engine's own previous output, as
tools/parity_budget.py local_reference does) and "head" (lasth -> logits).  `acc` is the dtype every product is accumulated in and
every value is held in: float64 is the reference, float32 the yardstick e32 -- one float32 realisation of the same formula.  `draw`
(a numpy Generator) permutes the channels of every K dimension: another float32 realisation of the same sums
(tools/fp32_stage_accuracy.py).  Built on the pieces of tests/f16_ref.py (fold_bn / folded / _conv / _mm / head, the `mutate`
hooks) and oracle/nn_oracle.py; nothing is rounded to halves here.

What the restatement takes from the engine, read from chiron_amd/csrc (weight_pack.h WeightPacker::stem_and_blocks / lstm_layer,
engine.hip run_cnn / run_rnn, wino.hip, lstm.hip), because it is the engine's documented arithmetic and not a defect:

  folding     BN folds in fp32 (fold_bn / fold_filter): W' = W * inv, sh = offset - mean * inv; conv2c's and branch1's shifts are added
              in fp32 where both run as one GEMM along K; the lifted first block keeps branch1 apart: sig * res_a + res_b, added to the
              finished sum.  forget_bias is added to the LSTM bias in fp32.
  conv2b      the form is an argument: "direct" (three taps, one K = 3 C sum), "f2" (Winograd F(2,3)) or "f4" (F(4,3)), on the blocks
              weight_pack.h gives a wino_u (1 x 3, stride 1, C -> C channels, not the one-channel first block).  The Winograd forms
              apply the input transform, the per-channel K sums of the transformed operands against the transformed filters U and the
              output transform in `acc`; U = G g in float64 from the taps g = (double) W * inv, rounded to float32 ONCE, exactly as
              weight_pack.h builds wino_u -- also in the float64 reference: U is the operand the engine multiplies by.  The
              transforms' amplification of rounding (F(4,3)'s most) therefore sits in e32: it belongs to the algorithm.
              exact_u = True keeps U in float64: then both forms ARE the direct form (tests/test_fp32_ref_cpu.py, 1e-12).
  block 1     the table form (pwl.hip) and the lifted form (CHIRON_NO_PWL=1) are one formula without roundings; the table's entries
              are float64 sums, so the table form has fewer float32 roundings than this restatement counts.
  gates       the formula is an argument.  "libm" (the default, and the yardstick of tests/fp32_cases.py): sigmoid and tanh as numpy
              computes them, what CHIRON_GATE_MATH 2 builds and what nn_oracle computes.  "engine": lstm.hip's gate math of the shipped
              build (form 0): sigmoid(x) = 1 / (1 + 2^(-x log2 e)), tanh(x) = 1 - 2 / (2^(2 x log2 e) + 1), each operation rounded to
              `acc`.  In float64 both are sigmoid and tanh to 1e-16; in float32 form 0's tanh carries an ABSOLUTE error of an ulp of 1
              (lstm.hip's own comment) where libm's is relative, which shows where the cell state is small (T = 1, T = 2).  The engine
              meets the bar under the stricter libm yardstick, so "engine" is kept only to explain those rows.
  head        fp32 throughout: f16_ref.head.

`mutate`: deliberate defects for the sensitivity tests (tests/fp32_cases.py DEFECTS), never set otherwise.  The structural ones are
f16_ref's (no_shift, tap_leak, whh_column, bw_from_end); the operand ones round a weight to 16 significant bits -- what a six-term
bf16 product with one term lost, or a tile that fell back to a two-plane path, multiplies by:
  conv16 = (site, out-channel slice, in-channel slice)    the folded filter of one conv site
  wx16 = (layer, direction, row slice)                     rows of W_x
  whh16 = (layer, direction)                               W_hh"""
import numpy as np

from oracle import nn_oracle

import f16_ref
from f16_ref import fold_bn, folded, head, head_constant      # noqa: F401  (the head and the folding are f16_ref's)

CONV2B_FORMS = ("direct", "f2", "f4")
LOG2E = 1.4426950408889634

# weight_pack.h: F(2,3): g0, (g0 + g1 + g2) / 2, (g0 - g1 + g2) / 2, g2;  F(4,3): U = G g
G2 = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=np.float64)
G4 = np.array([[0.25, 0, 0], [-1.0 / 6, -1.0 / 6, -1.0 / 6], [-1.0 / 6, 1.0 / 6, -1.0 / 6],
               [1.0 / 24, 1.0 / 12, 1.0 / 6], [1.0 / 24, -1.0 / 12, 1.0 / 6], [0, 0, 1]], dtype=np.float64)
# wino.hip: v = B^T d over d = x[2p - 1 .. 2p + 2] / x[4q - 1 .. 4q + 4], y = A^T m
BT2 = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
AT2 = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64)
BT4 = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0],
                [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], dtype=np.float64)
AT4 = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=np.float64)


def round_bits(a, bits=16):
    """every element at `bits` significant bits (round to nearest), the dtype kept"""
    a = np.asarray(a)
    m, e = np.frexp(a.astype(np.float64))
    return np.ldexp(np.round(m * 2.0 ** bits) / 2.0 ** bits, e).astype(a.dtype)


def wino_eligible(blk, c_in):
    """the blocks weight_pack.h gives a wino_u at an even length (population BN, fp32): 1 x 3, stride 1, C -> C, C % 64 == 0"""
    return c_in > 1 and blk["k"] == 3 and blk.get("stride", 1) == 1 and blk["in"] == blk["out"] and blk["out"] % 64 == 0


def _taps16(w, site, mutate):
    """mutation conv16 on a folded filter [k, Cin, Cout] (any float dtype)"""
    m = mutate.get("conv16")
    if m is None or m[0] != site:
        return w
    w = np.array(w, copy=True)
    w[:, m[2], m[1]] = round_bits(w[:, m[2], m[1]])
    return w


def wino_conv(a, g, form, acc, draw=None, exact_u=False):
    """a [B, T, C] in `acc`, g [3, C, N] float64 folded taps -> the 1 x 3 SAME convolution [B, T, N] in Winograd form, every sum in `acc`"""
    B, T, C = a.shape
    G, BT, AT, m = (G2, BT2, AT2, 2) if form == "f2" else (G4, BT4, AT4, 4)
    assert T % m == 0, (form, T)
    U = np.einsum("jt,tcn->jcn", G, np.asarray(g, dtype=np.float64))
    if not exact_u:
        U = U.astype(np.float32)                               # rounded to float32 once (weight_pack.h)
    U = U.astype(acc)
    xp = np.zeros((B, T + 2, C), dtype=acc)                    # SAME: one zero frame before and after every window
    xp[:, 1:T + 1] = a
    n_in = m + 2
    d = [xp[:, i:i + T:m] for i in range(n_in)]                # d[i][:, q] = x[m q - 1 + i]
    if draw is not None:
        p = draw.permutation(C)
        d, U = [np.ascontiguousarray(v[:, :, p]) for v in d], np.ascontiguousarray(U[:, p, :])
    BTa, ATa = BT.astype(acc), AT.astype(acc)
    ms = []
    for j in range(n_in):
        v = np.zeros_like(d[0])
        for i in range(n_in):
            if BT[j, i]:
                v = v + BTa[j, i] * d[i]
        ms.append(v @ U[j])
    y = np.zeros((B, T, U.shape[2]), dtype=acc)
    for r in range(m):
        s = np.zeros_like(ms[0])
        for j in range(n_in):
            if AT[r, j]:
                s = s + ATa[r, j] * ms[j]
        y[:, r::m] = s
    return y


def cnn(signal, spec, weights, acc=np.float64, draw=None, conv2b="direct", mutate=None, fold=np.float32, exact_u=False):
    """signal [B, L] -> features [B, T, C].  conv2b: the form of the eligible blocks' 1 x 3 convolution.  conv2b "direct" with fold
    float64 is nn_oracle.cnn_forward."""
    assert spec["bn_mode"] == "population" and conv2b in CONV2B_FORMS
    mutate = mutate or {}
    dt = np.dtype(acc).type
    wide = lambda a: np.asarray(a, dtype=acc)
    relu = lambda a: np.maximum(a, dt(0))

    def shift(sh, site):
        sh = wide(sh).copy()
        if mutate.get("no_shift") and mutate["no_shift"][0] == site:
            sh[mutate["no_shift"][1]] = 0
        return sh

    def filt(site, bn):
        w, sh = folded(weights, site, bn, fold)
        return _taps16(w, site, mutate), sh

    def conv3(a, site, blk, eligible):
        wb, shb = filt(site, True)
        s = blk.get("stride", 1)
        if eligible and conv2b != "direct":
            w = np.asarray(weights[site + "/weights"], dtype=fold)
            w = w.reshape(w.shape[-3], w.shape[-2], w.shape[-1])
            g = w.astype(np.float64) * fold_bn(weights, site, True, fold)[0].astype(np.float64)      # (double) W * inv
            y = wino_conv(a, _taps16(g, site, mutate), conv2b, acc, draw, exact_u)
        else:
            y = f16_ref._conv(a, wide(wb), s, draw)
        if mutate.get("tap_leak"):                             # f16_ref._conv2b's defect, in whichever form
            _, left, _ = nn_oracle.same_padding(a.shape[1], wb.shape[0], s)
            assert left >= 1
            y[1:, 0] += a[:-1, -1] @ wide(wb[left - 1])
        return relu(y + shift(shb, site))

    x = np.asarray(signal, dtype=acc)[:, :, None]
    if spec.get("stem"):
        w, sh = filt("conv_layer/conv1", True)
        x = relu(f16_ref._conv(x, wide(w), spec["stem"]["stride"], draw) + shift(sh, "conv_layer/conv1"))
    for blk in spec["cnn"]:
        n, s = blk["name"], blk.get("stride", 1)
        w1, sh1 = filt(n + "/branch1/conv1", blk["i_bn"])
        wa, sha = filt(n + "/branch2/conv2a", True)
        wc, shc = filt(n + "/branch2/conv2c", True)
        if x.shape[2] == 1:
            a = relu(x * wide(wa[0, 0]) + shift(sha, n + "/branch2/conv2a"))
            b = conv3(a, n + "/branch2/conv2b", blk, False)
            res = x[:, 0:(b.shape[1] - 1) * s + 1:s] * wide(w1[0, 0]) + wide(sh1)        # sig[t * stride] * res_a + res_b
            # (mutation no_shift at this site removes conv2c's and branch1's shifts together: one accumulator's worth, as in f16_ref)
            gone = mutate.get("no_shift") and mutate["no_shift"][0] == n + "/branch2/conv2c"
            if gone:
                res = res.copy()
                res[:, :, mutate["no_shift"][1]] -= wide(sh1)[mutate["no_shift"][1]]
            c = f16_ref._conv(b, wide(wc), 1, draw) + shift(shc, n + "/branch2/conv2c") + res
        else:
            a = relu(f16_ref._conv(x, wide(wa), 1, draw) + shift(sha, n + "/branch2/conv2a"))
            b = conv3(a, n + "/branch2/conv2b", blk, wino_eligible(blk, x.shape[2]))
            shc1 = (shc + sh1).astype(fold)                    # one GEMM along K: the shifts are added in fp32 (fold_filter)
            c = f16_ref._conv(b, wide(wc), 1, draw) + f16_ref._conv(x, wide(w1), s, draw) + shift(shc1, n + "/branch2/conv2c")
        x = relu(c)
    return x


def _gates(kind, acc):
    """-> (sigmoid, tanh) in `acc`"""
    if kind == "libm":
        return nn_oracle._sigmoid, np.tanh
    assert kind == "engine", kind
    dt = np.dtype(acc).type
    one, two, k = dt(1), dt(2), dt(LOG2E)
    sig = lambda v: one / (one + np.exp2(v * -k))
    tanh = lambda v: one - two / (np.exp2(v * (two * k)) + one)
    return sig, tanh


def lstm_direction(x, seq_len, kernel, bias, reverse, acc, draw=None, gates="libm", mutate=None, fold=np.float32):
    """f16_ref.lstm_direction without roundings and with the gate formula as an argument: z_x = x W_x + (bias + forget_bias) for all
    frames at once (the projection GEMM), z = z_x + h W_hh, gates and c in `acc`"""
    mutate = mutate or {}
    B, T, nin = x.shape
    H = kernel.shape[1] // 4
    k32 = np.asarray(kernel, dtype=fold)
    wx, wh = k32[:nin].copy(), k32[nin:].copy()
    if mutate.get("wx16") is not None:
        wx[mutate["wx16"]] = round_bits(wx[mutate["wx16"]])
    if mutate.get("whh16"):
        wh = round_bits(wh)
    if mutate.get("whh_column") is not None:
        col = mutate["whh_column"]
        wh[:, col] = wh[:, col + 1]
    wx, wh = wx.astype(acc), wh.astype(acc)
    b32 = np.asarray(bias, dtype=fold).copy()
    b32[2 * H:3 * H] += fold(nn_oracle.FORGET_BIAS)
    zx = f16_ref._mm(np.asarray(x, dtype=acc), wx, draw) + b32.astype(acc)
    hp = draw.permutation(H) if draw is not None else None
    out = np.zeros((B, T, H), dtype=acc)
    h = np.zeros((B, H), dtype=acc)
    c = np.zeros((B, H), dtype=acc)
    seq_len = np.minimum(np.asarray(seq_len).astype(np.int64), T)
    rows = np.arange(B)
    start = np.full(B, T, np.int64) if mutate.get("bw_from_end") else seq_len
    sig, tanh = _gates(gates, acc)
    for step in range(int(seq_len.max()) if B else 0):
        active = step < seq_len
        t_idx = np.where(active, start - 1 - step, 0) if reverse else np.full(B, step)
        z = zx[rows, t_idx] + (h @ wh if hp is None else h[:, hp] @ wh[hp])
        i, j, f, o = z[:, :H], z[:, H:2 * H], z[:, 2 * H:3 * H], z[:, 3 * H:]
        c_new = (sig(f) * c + sig(i) * tanh(j)).astype(acc)
        h_new = (sig(o) * tanh(c_new)).astype(acc)
        m = active[:, None]
        c = np.where(m, c_new, c)
        h = np.where(m, h_new, h)
        out[rows[active], t_idx[active]] = h_new[active]
    return out


def rnn_layer(x, seq_len, spec, weights, layer, acc=np.float64, draw=None, gates="libm", mutate=None, fold=np.float32):
    """ONE layer of the recurrent stack: x = the layer's input ([B, T, C] features for layer 0, [B, T, 2H] above) -> [B, T, 2H].
    with fold float64 (either gate formula) it is nn_oracle.rnn_layer_forward."""
    r = spec["rnn"]
    H = r["hidden"]
    mutate = mutate or {}
    x = np.asarray(x, dtype=acc)
    outs = []
    for di, (d, rev) in enumerate((("fw", False), ("bw", True))):
        if r["kind"] == "stack":
            p = "BDLSTM_rnn/cell_%d/bidirectional_rnn/%s/lstm_cell/" % (layer, d)
            xin = x
        else:
            p = "BDGRU_rnn/%s/multi_rnn_cell/cell_%d/lstm_cell/" % (d, layer)
            xin = x if layer == 0 else x[:, :, di * H:(di + 1) * H]       # the MultiRNN's upper layers project each direction alone
        mut = {}
        for key in ("whh_column", "wx16", "whh16"):
            if mutate.get(key) is not None and tuple(mutate[key][:2]) == (layer, di):
                mut[key] = mutate[key][2] if len(mutate[key]) > 2 else True
        if mutate.get("bw_from_end") and rev:
            mut["bw_from_end"] = True
        outs.append(lstm_direction(np.ascontiguousarray(xin), seq_len, weights[p + "kernel"], weights[p + "bias"], rev, acc, draw, gates, mut, fold))
    return np.concatenate(outs, axis=2)


def compose(signal, seq_len, spec, weights, acc=np.float64, conv2b="direct", gates="libm", mutate=None):
    """every stage from the signal: (features, [each layer's output], logits)"""
    fea = cnn(signal, spec, weights, acc, None, conv2b, mutate)
    layers, x = [], fea
    for layer in range(spec["rnn"]["layers"]):
        x = rnn_layer(x, seq_len, spec, weights, layer, acc, None, gates, mutate)
        layers.append(x)
    return fea, layers, head(x, weights, acc)
