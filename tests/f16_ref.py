"""The network of the fp16 / fp16-w2 engines restated in numpy, with a rounding to halves exactly where the engine has one.

Built on the pieces of oracle/nn_oracle.py (conv1d_same, the LSTM cell's formula, fc_head).  Three stages, each judged on its own
by tests/test_gpu_f16_ref.py: cnn (signal -> features), rnn (ANY features -> lasth), head (lasth -> logits).  `acc` is the dtype
every product is accumulated in and every wide value is held in: float64 is the reference, float32 the yardstick (one float32
realisation of the same formula).  `draw` (a numpy Generator) permutes the channels of every K dimension, another float32
realisation of the same sums (tools/f16_ref_accuracy.py).

Rounding sites, read from chiron_amd/csrc (weight_pack.h WeightPacker::stem_and_blocks / lstm_layer, engine.hip run_cnn / run_rnn and the kernels
they launch), not from the documents:

  folding     BN folds in fp32: inv = (1 / sqrtf(var + 1e-5f)) * scale, sh = offset - mean * inv, W' = W * inv (weight_pack.h fold_bn / fold_filter).  Shifts stay
              fp32; where two sites share one accumulator their shifts are added in fp32 (sh2c + sh1).  forget_bias is added to the
              LSTM bias in fp32.
  weights     every GEMM operand is f16(W') (WeightPacker::gemm); fp16-w2 stores hi = f16(W'), lo = f16(W' - hi) and multiplies by both,
              so the weight is hi + lo.  NOT rounded: the stem's filter (launch_stem_conv reads fp32), and the first block's
              lift_a / lift_b (conv2a of the one-channel signal) and res_a (its branch1), which are fp32 epilogue / loader operands.
  block 1     (one-channel input)  table form (default, pwl.hip): conv2a's activation is never stored and conv2b's filter never
              rounded -- the table's entries are float64 sums of the unrounded folded taps -- the only rounding is conv2b's output
              to halves.  CHIRON_NO_PWL=1 (launch_lift): conv2a's output is stored as halves, conv2b runs on the GEMM with rounded
              weights.  conv2c: rounded weights, shift = sh2c + sh1, + sig * res_a, ReLU, halves.
  blocks      conv2a, conv2b and the block's output (conv2c and branch1 as one GEMM along K) are stored as halves; fp32 accumulation,
              shift, ReLU, then one rounding.  The streaming kernels (stream16.hip) and the tiled GEMM (gemm.hip) differ in
              accumulation order only.
  stem        fp32 filter, fp32 sum, shift, ReLU, halves.
  recurrence  W_x and W_hh as halves (hi + lo in fp16-w2).  z = x W_x + bias is stored as halves by the projection GEMM where the
              form has a z (z16: the unfused fp16 forms; fp16-w2 only with CHIRON_W2_ZF16=1); the fused form adds the bias and both
              products in one fp32 accumulator.  Gates and c fp32.  The recurrent operand h is a half at every step; a layer's stored
              output is halves except the last layer's, which is fp32 unless CHIRON_F16_LASTH16=1.
  head        fp32 throughout.

The gate math of the kernels (lstm.hip, form 0) is within 2e-7 of exp / tanh, far below a half's ulp: exact functions here."""
import numpy as np

from oracle import nn_oracle

MODES = ("fp16", "fp16-w2")


def f16(a):
    """round to the nearest half, keep the dtype"""
    a = np.asarray(a)
    return a.astype(np.float16).astype(a.dtype)


def ident(a):
    return np.asarray(a)


def hilo(a32):
    """(hi, lo) halves of a float32 array as weight_pack.h split_half forms them: hi = f16(v), lo = f16(v - float(hi)), the difference in fp32"""
    a32 = np.asarray(a32, dtype=np.float32)
    hi = a32.astype(np.float16)
    lo = (a32 - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def weight_rounding(mode):
    """float32 array -> the weight an engine of this mode multiplies by, as float64 (None: unrounded)"""
    if mode is None:
        return lambda a: np.asarray(a, dtype=np.float64)
    assert mode in MODES, mode
    if mode == "fp16":
        return lambda a: np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float64)

    def w2(a):
        hi, lo = hilo(a)
        return hi.astype(np.float64) + lo.astype(np.float64)
    return w2


def fold_bn(weights, site, bn, ft=np.float32):
    """-> (inv, sh) in `ft` (the engine: float32), in fold_bn's association order; (1, 0) for a site without BN"""
    w = weights[site + "/weights"]
    co = w.shape[-1]
    if not bn:
        return np.ones(co, ft), np.zeros(co, ft)
    g = lambda leaf: np.asarray(weights[site + "_bn/" + leaf], dtype=ft)
    inv = (ft(1.0) / np.sqrt(g("pop_var") + ft(np.float32(1e-5)))) * g("scale")        # float32(1e-5) = nn_oracle.BN_EPS
    return inv.astype(ft), (g("offset") - g("pop_mean") * inv).astype(ft)


def folded(weights, site, bn, ft=np.float32):
    """-> (W' [k, Cin, Cout] with the BN scale folded, shift [Cout]), both in `ft`"""
    w = np.asarray(weights[site + "/weights"], dtype=ft)
    w = w.reshape(w.shape[-3], w.shape[-2], w.shape[-1])
    inv, sh = fold_bn(weights, site, bn, ft)
    return (w * inv).astype(ft), sh


def _conv(x, w, stride, draw):
    """conv1d_same with the K dimension (input channels) in the draw's order"""
    w = w.astype(x.dtype)
    if draw is not None and x.shape[2] > 1:
        p = draw.permutation(x.shape[2])
        x, w = np.ascontiguousarray(x[:, :, p]), np.ascontiguousarray(w[:, p, :])
    return nn_oracle.conv1d_same(x, w, stride)


def _mm(x, w, draw):
    w = w.astype(x.dtype)
    if draw is not None:
        p = draw.permutation(x.shape[-1])
        x, w = np.ascontiguousarray(x[..., p]), np.ascontiguousarray(w[p])
    return x @ w


def cnn(signal, spec, weights, acc=np.float64, draw=None, mode="fp16", table=True, aq=f16, mutate=None, fold=np.float32):
    """signal [B, L] -> features [B, T, C].  spec: the plain dict of nn_oracle; mode: "fp16" | "fp16-w2" | None (weights unrounded);
    table: block 1 in the table form (False: the lifted form of CHIRON_NO_PWL=1); aq: the rounding of every stored activation
    (ident: none); fold: the dtype BN is folded in (the engine: float32).  mode None, aq ident and fold float64 is nn_oracle.cnn_forward.  mutate: a dict of deliberate defects for the sensitivity tests
    (tests/test_f16_ref_cpu.py), never set otherwise."""
    assert spec["bn_mode"] == "population"
    mutate = mutate or {}
    wq = weight_rounding(mode)
    dt = np.dtype(acc).type
    sig = np.asarray(signal, dtype=acc)
    wide = lambda a: np.asarray(a, dtype=acc)
    sites = [0]

    def stored(a):
        """one stored activation site; mutation "wide_site" = n leaves the n-th one unrounded"""
        n = sites[0]
        sites[0] += 1
        return a if mutate.get("wide_site") == n else aq(a)

    def shift(sh, site):
        sh = wide(sh).copy()
        if mutate.get("no_shift") and mutate["no_shift"][0] == site:
            sh[mutate["no_shift"][1]] = 0
        return sh

    x = sig[:, :, None]
    if spec.get("stem"):
        w, sh = folded(weights, "conv_layer/conv1", True, fold)
        x = stored(np.maximum(_conv(x, wide(w), spec["stem"]["stride"], draw) + shift(sh, "conv_layer/conv1"), dt(0)))
    for blk in spec["cnn"]:
        n, s = blk["name"], blk.get("stride", 1)
        w1, sh1 = folded(weights, n + "/branch1/conv1", blk["i_bn"], fold)
        wa, sha = folded(weights, n + "/branch2/conv2a", True, fold)
        wb, shb = folded(weights, n + "/branch2/conv2b", True, fold)
        wc, shc = folded(weights, n + "/branch2/conv2c", True, fold)
        shc1 = (shc + sh1).astype(fold)                      # one accumulator: the shifts are added in fp32 (engine.hip)
        if x.shape[2] == 1:
            a = np.maximum(x * wide(wa[0, 0]) + shift(sha, n + "/branch2/conv2a"), dt(0))       # lift_a, lift_b: fp32, unrounded
            if table:
                b = _conv2b(a, wide(wb), s, draw, mutate)          # the table: sums of the unrounded folded taps
            else:
                b = _conv2b(stored(a), wq(wb).astype(acc), s, draw, mutate)
            b = stored(np.maximum(b + shift(shb, n + "/branch2/conv2b"), dt(0)))
            t_out = b.shape[1]
            res = x[:, 0:(t_out - 1) * s + 1:s] * wide(w1[0, 0])   # sig[t * stride] * res_a: fp32, unrounded (k = 1: no padding)
            c = _conv(b, wq(wc).astype(acc), 1, draw) + shift(shc1, n + "/branch2/conv2c") + res
        else:
            a = stored(np.maximum(_conv(x, wq(wa).astype(acc), 1, draw) + shift(sha, n + "/branch2/conv2a"), dt(0)))
            b = stored(np.maximum(_conv2b(a, wq(wb).astype(acc), s, draw, mutate) + shift(shb, n + "/branch2/conv2b"), dt(0)))
            c = _conv(b, wq(wc).astype(acc), 1, draw) + _conv(x, wq(w1).astype(acc), s, draw) + shift(shc1, n + "/branch2/conv2c")
        x = stored(np.maximum(c, dt(0)))
    return x


def _conv2b(a, w, stride, draw, mutate):
    """the 1 x k convolution; mutation "tap_leak": the first tap of every window but the first reads the previous window's last
    frame where SAME padding has a zero (what a kernel that walks the batch as one long row does wrong)"""
    y = _conv(a, w, stride, draw)
    if mutate.get("tap_leak"):
        _, left, _ = nn_oracle.same_padding(a.shape[1], w.shape[0], stride)
        assert left >= 1
        y[1:, 0] += a[:-1, -1] @ w[left - 1].astype(a.dtype)
    return y


def lstm_direction(x, seq_len, kernel, bias, reverse, acc, draw, wq, z16, hq, oq, mutate=None, fold=np.float32):
    """nn_oracle.lstm_direction with the engine's operands: z_x = x W_x + (bias + forget_bias) for all frames at once (rounded to
    halves if z16), z = z_x + hq(h) W_hh, gates and c wide, the recurrent operand hq(h), the stored output oq(h)."""
    mutate = mutate or {}
    B, T, nin = x.shape
    H = kernel.shape[1] // 4
    k32 = np.asarray(kernel, dtype=fold)
    wx, wh = wq(k32[:nin]).astype(acc), wq(k32[nin:]).astype(acc)
    if mutate.get("whh_column") is not None:
        col = mutate["whh_column"]
        wh = wh.copy()
        wh[:, col] = wh[:, col + 1]
    b32 = np.asarray(bias, dtype=fold).copy()
    b32[2 * H:3 * H] += fold(nn_oracle.FORGET_BIAS)          # folded into the projection's shift in fp32 (WeightPacker::lstm_layer)
    zx = _mm(np.asarray(x, dtype=acc), wx, draw) + b32.astype(acc)
    if z16:
        zx = f16(zx)
    hp = draw.permutation(H) if draw is not None else None
    out = np.zeros((B, T, H), dtype=acc)
    h = np.zeros((B, H), dtype=acc)
    c = np.zeros((B, H), dtype=acc)
    seq_len = np.minimum(np.asarray(seq_len).astype(np.int64), T)
    rows = np.arange(B)
    start = np.full(B, T, np.int64) if mutate.get("bw_from_end") else seq_len
    sig = nn_oracle._sigmoid
    for step in range(int(seq_len.max()) if B else 0):
        active = step < seq_len
        t_idx = np.where(active, start - 1 - step, 0) if reverse else np.full(B, step)
        z = zx[rows, t_idx] + (h @ wh if hp is None else h[:, hp] @ wh[hp])
        i, j, f, o = z[:, :H], z[:, H:2 * H], z[:, 2 * H:3 * H], z[:, 3 * H:]
        c_new = sig(f) * c + sig(i) * np.tanh(j)
        h_new = (sig(o) * np.tanh(c_new)).astype(acc)
        m = active[:, None]
        c = np.where(m, c_new, c).astype(acc)
        h = np.where(m, hq(h_new), h)
        out[rows[active], t_idx[active]] = oq(h_new)[active]
    return out


def rnn(features, seq_len, spec, weights, acc=np.float64, draw=None, mode="fp16", z16=True, lasth16=False, hq=f16, oq=f16, mutate=None, fold=np.float32):
    """features [B, T, C] (any: the tests pass the engine's own) -> lasth [B, T, 2H].  z16: bool, or one bool per layer (the RNA
    topology fuses layer 0 only); lasth16: the last layer's output as halves (CHIRON_F16_LASTH16=1).  hq / oq = ident with mode
    None, z16 False and fold float64 is nn_oracle.rnn_forward."""
    r = spec["rnn"]
    H, L = r["hidden"], r["layers"]
    wq = weight_rounding(mode)
    z16 = [bool(z16)] * L if np.isscalar(z16) or isinstance(z16, bool) else [bool(v) for v in z16]
    assert len(z16) == L
    mutate = mutate or {}
    x = np.asarray(features, dtype=acc)
    for layer in range(L):
        outs = []
        last = layer + 1 == L
        out_q = oq if (not last or lasth16) else ident
        if mutate.get("lasth_half") and last:
            out_q = f16
        for di, (d, rev) in enumerate((("fw", False), ("bw", True))):
            if r["kind"] == "stack":
                p = "BDLSTM_rnn/cell_%d/bidirectional_rnn/%s/lstm_cell/" % (layer, d)
                xin = x
            else:
                p = "BDGRU_rnn/%s/multi_rnn_cell/cell_%d/lstm_cell/" % (d, layer)
                xin = x if layer == 0 else x[:, :, di * H:(di + 1) * H]       # the MultiRNN's upper layers project each direction alone
            mut = {}
            if mutate.get("whh_column") is not None and mutate["whh_column"][:2] == (layer, di):
                mut["whh_column"] = mutate["whh_column"][2]
            if mutate.get("bw_from_end") and rev:
                mut["bw_from_end"] = True
            zq = z16[layer] if not mutate.get("flip_z16") else not z16[layer]
            outs.append(lstm_direction(np.ascontiguousarray(xin), seq_len, weights[p + "kernel"], weights[p + "bias"], rev, acc, draw, wq,
                                       zq, hq, out_q, mut, fold))
        x = np.concatenate(outs, axis=2)
    return x


def head(lasth, weights, acc=np.float64):
    """lasth [B, T, 2H] -> logits [B, T, K]: nn_oracle.fc_head in `acc` (the engine's head is fp32 throughout)"""
    return nn_oracle.fc_head(np.asarray(lasth, dtype=acc), weights)


def head_constant(weights, hidden, acc=np.float64):
    """the logits of a frame whose lasth is 0 (every frame at and past a row's seq_len)"""
    return head(np.zeros((1, 1, 2 * hidden)), weights, acc)[0, 0]


def compose(signal, seq_len, spec, weights, acc=np.float64, draw=None, mode="fp16", table=True, z16=True, lasth16=False):
    """the three stages from the signal: (features, lasth, logits)"""
    fea = cnn(signal, spec, weights, acc, draw, mode, table)
    lasth = rnn(fea, seq_len, spec, weights, acc, draw, mode, z16, lasth16)
    return fea, lasth, head(lasth, weights, acc)
