#!/usr/bin/env python
"""Distributional parity of the engine's logits on trained-checkpoint-like weights (round-5 review, item 1).

north_star: "pre-CTC logits within 1e-4 in fp32".  On the seeded synthetic weights the engine meets that against the float64
oracle (6e-6 .. 2.6e-5).  On trained-like weights (tests/regimes.py) NO float32 pipeline does: the recurrent stack amplifies
the features' rounding error, ill-conditioned per window (one window can carry 1000 x), so "engine / ONE float32 restatement"
is a ratio of two draws of a heavy-tailed quantity.  Round 5 answered a failed bound by admitting a second and a third
summation order -- a max over references that a genuine 2 .. 3 x excess would also pass.  This tool replaces that rule by the
distribution itself:

  realise   (CPU: numpy + torch's CPU sgemm -- no GPU, no product code on the arithmetic path)  For every case = topology x weight set, R
            float32 REALISATIONS of the same formulas (cnn.py:234-262, rnn.py:44-97) on N windows.  A realisation draws, per
            convolution: BN applied to the rounded sum or folded into the filters (weight_pack.h:fold_bn), a random permutation of the
            K = taps x channels accumulation order, a random K-blocking (32 .. K; block partials by BLAS, the blocks accumulated
            in float32 one after the other), the shift as the accumulator's start or added last; per LSTM direction: hoisted
            x-projection (bias inside / outside) or TF's concatenated [x, h] @ kernel, permuted / blocked K again, and one of two
            float32 forms of sigmoid and of tanh.  Per window it records the logits' max |error| and sum of squared errors against
            the float64 oracle, plain and peaked head -> tests/golden/parity_dist/<topology>_<seed>.npz (a fixture: numbers only).
  engine    (GPU)  the HIP engine (dtype fp32 and fp32-split) on the same seeded inputs -> the same per-window statistics.
  chain     (CPU, many cores)  32 more realisations per case: oracle/chiron_oracle.c -- plain C loops, ONE strictly sequential chain per
            output -- on channel-permuted weights (permute_channels: the same function, another accumulation order) -> <case>_chain.npz
  judge     combines the two (also inside tests/test_gpu_parity.py::test_distributional_parity), four statistics (statistics(), BARS):
              bulk     set rms without the implementation's own 3 worst windows / the ensemble's p90 of the same
              typical  median over windows of (error / the ensemble's median error in that window)
              tail     fraction of windows whose error exceeds the ensemble's p99 for THAT window
              worst    max over windows of (error / the ensemble's largest error in that window)
            The review asked for tail <= 1 % and (untrimmed) set rms <= p90.  Read literally, tail <= 1 % is a coin flip for a PERFECT
            implementation: an exchangeable draw exceeds the p99 of R others with probability 1 / (R + 1) .. 2 / (R + 1), so its expected
            exceedance EQUALS the bar; and the untrimmed set rms is one ill-conditioned window.  The bars are therefore calibrated on the
            ensembles themselves: leave-one-out (each realisation judged against the others) gives the null distribution, the same
            realisation with its error DOUBLED (the logits' error is linear in a small perturbation) the alternative the round-5 rule could
            not reject; `judge` prints, per case, the share of null draws passing and of doubled draws rejected next to the engine's figures.

  python tools/parity_dist.py realise [--cases dna:5,...] [--realisations 64] [--windows 256]
  python tools/parity_dist.py chain   [--realisations 32]
  python tools/parity_dist.py engine  [--dtypes fp32,fp32-split] [--engine-draws 8]     ->  gpurun_out/parity_dist_engine.npz
  python tools/parity_dist.py judge   gpurun_out/parity_dist_engine.npz  ->  gpurun_out/parity_dist_report.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import nn_oracle     # noqa: E402  (checker only: this is test infrastructure, not a product path)

F32 = np.float32
FIXTURES = os.path.join(ROOT, "tests", "golden", "parity_dist")
CASES = [(t, s) for t in ("dna", "rna") for s in (5, 6, 7, 8)]
N_WINDOWS, N_REAL = 256, 64


# ------------------------------------------------------------------ the cases (same (signal, weight) seed pairs as parity_budget)
def case_inputs(topology, weight_seed, n_windows=N_WINDOWS):
    import chiron_amd as ca
    from chiron_amd import signal_io
    import regimes
    spec = ca.dna_default_spec() if topology == "dna" else ca.rna_default_spec()
    L, jump = (400, 390) if topology == "dna" else (500, 490)
    sig = ca.synthetic_signal(1, jump * (n_windows - 1) + 200, seed=67 + 10 * (weight_seed - 5))[0]
    ev, ln = signal_io.window_signal(sig, 0, jump, L)
    x, ln = np.array(ev, dtype=np.float32), np.asarray(ln, dtype=np.int64).copy()
    ln[2], ln[5] = L // 3, 0                                 # a ragged and an empty row stay in
    w, _ = regimes.trained_like_weights(spec, x[:24], seed=weight_seed)
    T = spec.output_len(L)
    sl = ca.seq_len_for_engine(ln, L / float(T))
    return spec, L, x, sl, w


def peaked(w):
    import regimes
    return regimes.peaked_head(w)


def reference64(spec, w, x, sl):
    """float64 oracle: features, recurrent output, logits under the plain and the peaked head"""
    sd = spec.to_dict()
    w64 = {k: np.asarray(v, dtype=np.float64) for k, v in w.items()}
    fea = nn_oracle.cnn_forward(np.asarray(x, dtype=np.float64), sd, w64)
    h = nn_oracle.rnn_forward(fea, sl, sd, w64)
    wp = {k: np.asarray(v, dtype=np.float64) for k, v in peaked(w).items()}
    return {"features": fea, "lasth": h, "plain": nn_oracle.fc_head(h, w64), "peaked": nn_oracle.fc_head(h, wp)}


def window_stats(logits, ref, sl):
    """per window over its valid frames: max |error|, sum of squared errors, number of values"""
    d = np.asarray(logits, dtype=np.float64) - ref
    T = ref.shape[1]
    m = (np.arange(T)[None, :] < np.asarray(sl)[:, None])[..., None]
    d = d * m
    return np.abs(d).max(axis=(1, 2)), (d * d).sum(axis=(1, 2)), (np.asarray(sl) * ref.shape[2]).astype(np.float64)


# ------------------------------------------------------------------ one float32 realisation of the same formulas
BLOCKS = (32, 64, 128, 256, 1 << 30)


def matmul_f32(a, wt, rng, acc0=None, blocks=BLOCKS, rows=16384):
    """fl32(a @ wt (+ acc0)) in ONE of its float32 accumulation orders: K permuted at random, cut into blocks of a random size, block
    partials by BLAS sgemm, the blocks accumulated one after the other in float32 starting from acc0 (or from the first block).
    (torch's CPU sgemm only because it takes strided blocks without a copy and gathers columns with all cores: 33 -> 9 s per realisation)"""
    import torch
    M, K = a.shape
    perm = torch.from_numpy(rng.permutation(K))
    bs = min(int(rng.choice(blocks)), K)
    ap = torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).index_select(1, perm)
    wp = torch.from_numpy(np.ascontiguousarray(wt, dtype=F32)).index_select(0, perm)
    out = torch.empty((M, wt.shape[1]), dtype=torch.float32)
    a0 = None if acc0 is None else torch.from_numpy(np.ascontiguousarray(acc0, dtype=F32))
    for r0 in range(0, M, rows):
        r1 = min(M, r0 + rows)
        acc = out[r0:r1]
        first = True
        if a0 is not None:
            acc.copy_(a0.expand(r1 - r0, -1))
            first = False
        for k0 in range(0, K, bs):
            if first:
                torch.mm(ap[r0:r1, k0:k0 + bs], wp[k0:k0 + bs], out=acc)
                first = False
            else:
                acc.addmm_(ap[r0:r1, k0:k0 + bs], wp[k0:k0 + bs])        # acc = fl32(acc + block partial)
    return out.numpy()


def conv_f32(x, w, site, stride, bn, relu, rng):
    """conv_layer (cnn.py:15-83) + population BN (cnn.py:125-163) in float32, one realisation"""
    W = w[site + "/weights"]
    W = W.reshape(W.shape[-3], W.shape[-2], W.shape[-1]).astype(F32)
    k, cin, cout = W.shape
    B, width, _ = x.shape
    out, left, right = nn_oracle.same_padding(width, k, stride)
    xp = np.zeros((B, width + left + right, cin), dtype=F32)
    xp[:, left:left + width] = x
    cols = np.concatenate([xp[:, tap:tap + (out - 1) * stride + 1:stride] for tap in range(k)], axis=2).reshape(B * out, k * cin)
    wt = W.reshape(k * cin, cout)
    if bn:
        sc, of, mu, var = [w[site + "_bn/" + n].astype(F32) for n in ("scale", "offset", "pop_mean", "pop_var")]
        inv = ((F32(1.0) / np.sqrt(var + F32(nn_oracle.BN_EPS))).astype(F32) * sc).astype(F32)
        shift = (of - (mu * inv).astype(F32)).astype(F32)
        if rng.rand() < 0.5:                                   # natural: BN applied to the rounded sum (tf.nn.batch_normalization)
            y = matmul_f32(cols, wt, rng)
            y = (y * inv).astype(F32) + shift
        else:                                                  # folded into the filters (any inference runtime; weight_pack.h:fold_bn)
            wf = (wt * inv[None, :]).astype(F32)
            if rng.rand() < 0.5:
                y = matmul_f32(cols, wf, rng, acc0=shift)      # the shift is where the accumulator starts
            else:
                y = matmul_f32(cols, wf, rng) + shift
    else:
        y = matmul_f32(cols, wt, rng)
    y = y.astype(F32).reshape(B, out, cout)
    return np.maximum(y, F32(0)) if relu else y


def cnn_f32(x, sd, w, rng):
    p = np.asarray(x, dtype=F32)[:, :, None]
    for blk in sd["cnn"]:
        n, s = blk["name"], blk.get("stride", 1)
        b1 = conv_f32(p, w, n + "/branch1/conv1", s, blk["i_bn"], False, rng)
        a = conv_f32(p, w, n + "/branch2/conv2a", 1, True, True, rng)
        b = conv_f32(a, w, n + "/branch2/conv2b", s, True, True, rng)
        c = conv_f32(b, w, n + "/branch2/conv2c", 1, True, False, rng)
        p = np.maximum((b1 + c).astype(F32), F32(0))
    return p


def _sig_a(v):
    with np.errstate(over="ignore"):                           # exp(-v) = inf for v < -88: 1 / inf = 0, the value float32 arithmetic gives
        return (F32(1.0) / (F32(1.0) + np.exp(-v))).astype(F32)


def _sig_b(v):
    return (F32(0.5) * np.tanh(F32(0.5) * v) + F32(0.5)).astype(F32)


def _tanh_a(v):
    return np.tanh(v)


def _tanh_b(v):
    return (F32(1.0) - F32(2.0) / (np.exp(np.minimum(F32(2.0) * v, F32(80.0))) + F32(1.0))).astype(F32)


def lstm_f32(x, seq_len, kernel, bias, reverse, rng):
    """LSTMCell under dynamic_rnn with sequence_length (rnn.py:44-65) in float32, one realisation"""
    B, T, nin = x.shape
    H = kernel.shape[1] // 4
    kernel, bias = kernel.astype(F32), bias.astype(F32).copy()
    bias[2 * H:3 * H] += F32(nn_oracle.FORGET_BIAS)            # + 1.0 on f: added to the bias here, to the pre-activation by TF -- one rounding either way
    seq_len = np.asarray(seq_len).astype(np.int64)
    form = int(rng.randint(3))                                 # 0 / 1: hoisted projection, bias inside / outside; 2: TF's [x, h] @ kernel
    sig = _sig_a if rng.rand() < 0.5 else _sig_b
    tanh = _tanh_a if rng.rand() < 0.5 else _tanh_b
    hperm = rng.permutation(H)
    hbs = int(rng.choice((25, 50, 100)))
    wh = np.ascontiguousarray(kernel[nin:][hperm])
    if form < 2:
        zx = matmul_f32(x.reshape(B * T, nin), kernel[:nin], rng, acc0=bias if form == 0 else None).reshape(B, T, 4 * H)
    else:
        kperm = rng.permutation(nin + H)
        kbs = min(int(rng.choice(BLOCKS)), nin + H)
        wk = np.ascontiguousarray(kernel[kperm])
    out = np.zeros((B, T, H), dtype=F32)
    h = np.zeros((B, H), dtype=F32)
    c = np.zeros((B, H), dtype=F32)
    rows = np.arange(B)
    for step in range(T):
        active = step < seq_len
        if not active.any():
            break
        t_idx = np.where(active, seq_len - 1 - step, 0) if reverse else np.full(B, step)
        if form < 2:
            hp = h[:, hperm]
            z = zx[rows, t_idx]
            for k0 in range(0, H, hbs):
                z = z + hp[:, k0:k0 + hbs] @ wh[k0:k0 + hbs]
            if form == 1:
                z = z + bias
        else:
            xh = np.concatenate([x[rows, t_idx], h], axis=1)[:, kperm]
            z = None
            for k0 in range(0, nin + H, kbs):
                part = xh[:, k0:k0 + kbs] @ wk[k0:k0 + kbs]
                z = part if z is None else z + part
            z = z + bias
        i, j, f, o = z[:, :H], z[:, H:2 * H], z[:, 2 * H:3 * H], z[:, 3 * H:]
        c_new = (sig(f) * c + sig(i) * tanh(j)).astype(F32)
        h_new = (sig(o) * tanh(c_new)).astype(F32)
        m = active[:, None]
        c = np.where(m, c_new, c)
        h = np.where(m, h_new, h)
        out[rows[active], t_idx[active]] = h_new[active]
    return out


def rnn_f32(fea, sl, sd, w, rng):
    r = sd["rnn"]
    H = r["hidden"]
    x = fea
    for layer in range(r["layers"]):
        outs = []
        for di, (d, rev) in enumerate((("fw", False), ("bw", True))):
            if r["kind"] == "stack":
                p, xin = "BDLSTM_rnn/cell_%d/bidirectional_rnn/%s/lstm_cell/" % (layer, d), x
            else:
                p = "BDGRU_rnn/%s/multi_rnn_cell/cell_%d/lstm_cell/" % (d, layer)
                xin = x if layer == 0 else x[:, :, di * H:(di + 1) * H]
            outs.append(lstm_f32(np.ascontiguousarray(xin), sl, w[p + "kernel"], w[p + "bias"], rev, rng))
        x = np.concatenate(outs, axis=2)
    return x


def realisation(spec, w, x, sl, rng):
    sd = spec.to_dict()
    fea = cnn_f32(x, sd, w, rng)
    h = rnn_f32(fea, sl, sd, w, rng)
    w32 = {k: np.asarray(v, dtype=F32) for k, v in w.items()}
    wp = {k: np.asarray(v, dtype=F32) for k, v in peaked(w).items()}
    return fea, {"plain": nn_oracle.fc_head(h, w32), "peaked": nn_oracle.fc_head(h, wp)}


def permute_channels(spec, w, rng):
    """A function-preserving reparametrisation: every hidden channel axis of the network (the 256 channels behind each convolution,
    the H units of each LSTM direction) is permuted, producers' outputs and consumers' inputs alike.  Exactly the same function in
    real arithmetic -- and a DIFFERENT order of every K accumulation for whatever implementation evaluates it, the C oracle's plain
    sequential loops and the HIP engine's MFMA chains included.  -> weights dict"""
    sd = spec.to_dict()
    out = {k: np.array(v) for k, v in w.items()}
    H = sd["rnn"]["hidden"]

    def conv(site, pin, pout, bn):
        W = out[site + "/weights"]
        out[site + "/weights"] = np.ascontiguousarray(W[:, :, pin][:, :, :, pout])
        if bn:
            for n in ("scale", "offset", "pop_mean", "pop_var"):
                out[site + "_bn/" + n] = out[site + "_bn/" + n][pout]

    pin = np.arange(sd["cnn"][0]["in"])
    for blk in sd["cnn"]:
        n, c = blk["name"], blk["out"]
        pa, pb, po = rng.permutation(c), rng.permutation(c), rng.permutation(c)
        conv(n + "/branch1/conv1", pin, po, blk["i_bn"])
        conv(n + "/branch2/conv2a", pin, pa, True)
        conv(n + "/branch2/conv2b", pa, pb, True)
        conv(n + "/branch2/conv2c", pb, po, True)
        pin = po

    def cell(prefix, pin_x, pd):
        k, b = out[prefix + "kernel"], out[prefix + "bias"]
        nin = k.shape[0] - H
        rows = np.concatenate([pin_x, nin + pd])
        cols = np.concatenate([g * H + pd for g in range(4)])
        out[prefix + "kernel"] = np.ascontiguousarray(k[rows][:, cols])
        out[prefix + "bias"] = b[cols]

    L = sd["rnn"]["layers"]
    plast = rng.permutation(H)
    if sd["rnn"]["kind"] == "stack":
        px = pin
        for l in range(L):
            pf, pbw = (plast, plast) if l == L - 1 else (rng.permutation(H), rng.permutation(H))
            cell("BDLSTM_rnn/cell_%d/bidirectional_rnn/fw/lstm_cell/" % l, px, pf)
            cell("BDLSTM_rnn/cell_%d/bidirectional_rnn/bw/lstm_cell/" % l, px, pbw)
            px = np.concatenate([pf, H + pbw])
    else:
        for d in ("fw", "bw"):
            px = pin
            for l in range(L):
                pd_ = plast if l == L - 1 else rng.permutation(H)
                cell("BDGRU_rnn/%s/multi_rnn_cell/cell_%d/lstm_cell/" % (d, l), px, pd_)
                px = pd_
    out["rnn_fnn_layer/weights"] = np.ascontiguousarray(out["rnn_fnn_layer/weights"][:, plast])
    out["rnn_fnn_layer/bias"] = out["rnn_fnn_layer/bias"][plast]
    out["rnn_fnn_layer/weights_class"] = np.ascontiguousarray(out["rnn_fnn_layer/weights_class"][plast])
    return out


def fixture_path(topology, seed):
    return os.path.join(FIXTURES, "%s_%d.npz" % (topology, seed))


def cmd_realise(a):
    os.makedirs(FIXTURES, exist_ok=True)
    for topology, seed in a.cases:
        path = fixture_path(topology, seed)
        if os.path.exists(path) and not a.force:
            print("have", path)
            continue
        t0 = time.time()
        spec, L, x, sl, w = case_inputs(topology, seed, a.windows)
        ref = reference64(spec, w, x, sl)
        out = {"windows": a.windows, "realisations": a.realisations, "seq_len": np.asarray(sl)}
        acc = {h: {"max": [], "sumsq": []} for h in ("plain", "peaked")}
        fea_rms = []
        part = path + ".partial.npy"                              # a killed run resumes at the realisation it was in
        if os.path.exists(part):
            saved = np.load(part, allow_pickle=True).item()
            if saved["windows"] == a.windows:
                acc, fea_rms = saved["acc"], saved["fea_rms"]
        cnt = window_stats(ref["plain"], ref["plain"], sl)[2]
        for r in range(len(fea_rms), a.realisations):
            rng = np.random.RandomState(100003 * seed + 7919 * r + (0 if topology == "dna" else 1))
            fea, lg = realisation(spec, w, x, sl, rng)
            fea_rms.append(np.sqrt(((fea.astype(np.float64) - ref["features"]) ** 2).mean(axis=(1, 2))))
            for h in acc:
                mx, sq, cnt = window_stats(lg[h], ref[h], sl)
                acc[h]["max"].append(mx)
                acc[h]["sumsq"].append(sq)
            np.save(part, {"windows": a.windows, "acc": acc, "fea_rms": fea_rms}, allow_pickle=True)
            print("%s %d realisation %d/%d  %.0f s  logits max %.3g rms %.3g" % (topology, seed, r + 1, a.realisations, time.time() - t0,
                  acc["plain"]["max"][-1].max(), np.sqrt(acc["plain"]["sumsq"][-1].sum() / cnt.sum())), flush=True)
        for h in acc:
            out[h + "_max"] = np.asarray(acc[h]["max"], dtype=np.float32)          # [R, N]
            out[h + "_sumsq"] = np.asarray(acc[h]["sumsq"], dtype=np.float32)
        out["count"] = cnt.astype(np.float32)
        out["features_rms"] = np.asarray(fea_rms, dtype=np.float32)
        out["logits_scale_rms"] = np.asarray([np.sqrt((ref[h] ** 2).mean()) for h in ("plain", "peaked")])
        np.savez_compressed(path, **out)
        if os.path.exists(part):
            os.remove(part)
        print("wrote %s (%.0f s)" % (path, time.time() - t0), flush=True)


def cmd_chain(a):
    """`chain` realisations: oracle/chiron_oracle.c -- plain C loops, ONE strictly sequential multiply-then-add chain per output over
    taps x channels, BN applied to the rounded sum, libm expf / tanhf -- on channel-permuted weights (permute_channels): the most
    literal float32 reading of the formulas, in a fresh accumulation order per draw.  (C with OpenMP over windows: seconds per draw
    on a many-core host, which is why these are generated where the cores are: the GPU box's host.)"""
    from oracle import c_oracle
    os.makedirs(FIXTURES, exist_ok=True)
    for topology, seed in a.cases:
        path = fixture_path(topology, seed).replace(".npz", "_chain.npz")
        if os.path.exists(path) and not a.force:
            print("have", path)
            continue
        t0 = time.time()
        spec, L, x, sl, w = case_inputs(topology, seed, a.windows)
        ref = reference64(spec, w, x, sl)
        sd, T = spec.to_dict(), spec.output_len(L)
        acc = {h: {"max": [], "sumsq": []} for h in ("plain", "peaked")}
        for r in range(a.realisations):
            rng = np.random.RandomState(200003 * seed + 104729 * r + (0 if topology == "dna" else 1))
            wp = permute_channels(spec, w, rng)
            for h, ww in (("plain", wp), ("peaked", peaked(wp))):
                lg = c_oracle.forward(x, sl, sd, spec.pack(ww), T)
                mx, sq, cnt = window_stats(lg, ref[h], sl)
                acc[h]["max"].append(mx)
                acc[h]["sumsq"].append(sq)
            print("%s %d chain %d/%d  %.0f s  logits max %.3g rms %.3g" % (topology, seed, r + 1, a.realisations, time.time() - t0,
                  acc["plain"]["max"][-1].max(), np.sqrt(acc["plain"]["sumsq"][-1].sum() / cnt.sum())), flush=True)
        out = {"windows": a.windows, "realisations": a.realisations, "count": cnt.astype(np.float32)}
        for h in acc:
            out[h + "_max"] = np.asarray(acc[h]["max"], dtype=np.float32)
            out[h + "_sumsq"] = np.asarray(acc[h]["sumsq"], dtype=np.float32)
        np.savez_compressed(path, **out)
        print("wrote %s (%.0f s)" % (path, time.time() - t0), flush=True)


def load_ensemble(topology, seed):
    """the realisations a case is judged against: the blocked-BLAS draws + (when generated) the sequential-chain draws"""
    fix = dict(np.load(fixture_path(topology, seed)))
    kinds = ["blocked"] * fix["plain_max"].shape[0]
    cpath = fixture_path(topology, seed).replace(".npz", "_chain.npz")
    if os.path.exists(cpath):
        ch = np.load(cpath)
        for k in ("plain_max", "plain_sumsq", "peaked_max", "peaked_sumsq"):
            fix[k] = np.concatenate([fix[k], ch[k]], axis=0)
        kinds += ["chain"] * ch["plain_max"].shape[0]
    fix["kinds"] = np.asarray(kinds)
    return fix


# ------------------------------------------------------------------ the engine on the same inputs (GPU)
def cmd_engine(a):
    import chiron_amd as ca
    out, meta = {}, {"dtypes": a.dtypes, "cases": ["%s:%d" % c for c in a.cases], "seconds": {}}
    for topology, seed in a.cases:
        t0 = time.time()
        spec, L, x, sl, w = case_inputs(topology, seed, a.windows)
        ref = reference64(spec, w, x, sl)
        for dtype in a.dtypes:
            for head, ww in (("plain", w), ("peaked", peaked(w))):
                with ca.Engine(spec, ww, max_batch=x.shape[0], segment_len=L, dtype=dtype) as eng:
                    res = eng.infer(x, sl, want_logits=True)
                    fea = eng.features() if (head == "plain" and dtype == "fp32") else None
                mx, sq, cnt = window_stats(res.logits, ref[head], sl)
                key = "%s_%d_%s_%s" % (topology, seed, dtype, head)
                out[key + "_max"], out[key + "_sumsq"] = mx.astype(np.float32), sq.astype(np.float32)
                if fea is not None:
                    out["%s_%d_features_rms" % (topology, seed)] = np.sqrt(((fea.astype(np.float64) - ref["features"]) ** 2).mean(axis=(1, 2))).astype(np.float32)
                print("%s %d %-10s %-6s logits max %.3g rms %.3g" % (topology, seed, dtype, head, mx.max(), np.sqrt(sq.sum() / cnt.sum())), flush=True)
            # the engine's OWN rounding distribution: the same network with its hidden channels permuted (permute_channels) is the same
            # function in another accumulation order.  What the draws have in common (their mean error) is the engine's SYSTEMATIC
            # part -- rounded BN-folded / Winograd-transformed weights, the table, the gate approximations; the rest is accumulation noise
            if a.engine_draws > 0:
                dm, dq, esum = [], [], 0.0
                for r in range(a.engine_draws):
                    wp = permute_channels(spec, w, np.random.RandomState(300007 * seed + 15485863 * r + (0 if topology == "dna" else 1)))
                    with ca.Engine(spec, wp, max_batch=x.shape[0], segment_len=L, dtype=dtype) as eng:
                        lg = eng.infer(x, sl, want_logits=True).logits
                    mx, sq, cnt = window_stats(lg, ref["plain"], sl)
                    dm.append(mx)
                    dq.append(sq)
                    esum = esum + (lg.astype(np.float64) - ref["plain"])
                key = "%s_%d_%s_" % (topology, seed, dtype)
                out[key + "draws_max"], out[key + "draws_sumsq"] = np.asarray(dm, dtype=np.float32), np.asarray(dq, dtype=np.float32)
                mx, sq, cnt = window_stats(esum / a.engine_draws + ref["plain"], ref["plain"], sl)
                out[key + "drawmean_max"], out[key + "drawmean_sumsq"] = mx.astype(np.float32), sq.astype(np.float32)
                print("%s %d %-10s %d permuted draws: set rms %s; rms of their MEAN error %.3g" % (
                    topology, seed, dtype, a.engine_draws, " ".join("%.3g" % np.sqrt(q.sum() / cnt.sum()) for q in dq), np.sqrt(sq.sum() / cnt.sum())), flush=True)
        out["%s_%d_count" % (topology, seed)] = cnt.astype(np.float32)
        meta["seconds"]["%s:%d" % (topology, seed)] = round(time.time() - t0, 1)
    d = os.path.join(ROOT, "gpurun_out")
    os.makedirs(d, exist_ok=True)
    np.savez_compressed(os.path.join(d, "parity_dist_engine%s.npz" % a.tag), **out)
    json.dump(meta, open(os.path.join(d, "parity_dist_engine%s_meta.json" % a.tag), "w"), indent=1)


# ------------------------------------------------------------------ the judgement
TRIM = 3      # windows dropped from the top of every implementation's own squared errors before its set rms is taken


def trimmed_rms(sumsq, count, k=TRIM):
    """rms over the set without the implementation's own k worst windows: one ill-conditioned window (error 100 .. 1000 x the typical
    window's, for EVERY float32 implementation) otherwise IS the set rms -- 96 % of it on DNA set 7"""
    o = np.sort(np.asarray(sumsq, dtype=np.float64), axis=-1)
    return np.sqrt(o[..., :o.shape[-1] - k].sum(axis=-1) / count.sum())


def statistics(e_max, e_sumsq, r_max, r_sumsq, count):
    """e_*: [N] of the implementation under test; r_*: [R, N] of the realisations it is judged against"""
    valid = count > 0
    p99 = np.quantile(r_max, 0.99, axis=0)
    med = np.median(r_max, axis=0)
    top = r_max.max(axis=0)
    set_rms = np.sqrt(r_sumsq.sum(axis=1) / count.sum())
    e_rms = float(np.sqrt(e_sumsq.sum() / count.sum()))
    r_trim, e_trim = trimmed_rms(r_sumsq, count), float(trimmed_rms(e_sumsq, count))
    return {"exceeds_p99_frac": float((e_max[valid] > p99[valid]).mean()),
            "median_window_ratio_to_realisations_median": float(np.median(e_max[valid] / np.maximum(med[valid], 1e-30))),
            "trimmed_rms": e_trim, "trimmed_rms_over_p90": float(e_trim / np.quantile(r_trim, 0.9)), "trimmed_rms_percentile": float((r_trim < e_trim).mean()),
            "worst_ratio_to_realisations_max": float((e_max[valid] / np.maximum(top[valid], 1e-30)).max()),
            "set_rms": e_rms, "set_rms_percentile": float((set_rms < e_rms).mean()), "set_max": float(e_max.max()),
            "realisations_trimmed_rms_p50_p90_max": [float(np.quantile(r_trim, q)) for q in (0.5, 0.9, 1.0)],
            "realisations_set_rms_p50_p90_max": [float(np.quantile(set_rms, q)) for q in (0.5, 0.9, 1.0)],
            "realisations_set_max_p50_p90_max": [float(np.quantile(r_max.max(axis=1), q)) for q in (0.5, 0.9, 1.0)]}


# The bars (fp32 engine).  Calibrated on the ensembles themselves (judge_case: leave-one-out draws = the null, the same draws with their
# error doubled = the alternative); `judge` prints, per case, how many null draws pass and how many doubled draws are rejected.
BARS = {"trimmed_rms_over_p90": 1.25,                          # bulk: set rms without the implementation's own 3 worst windows <= 1.25 x the ensemble's p90
        "median_window_ratio_to_realisations_median": 1.5,      # typical window: median over windows of error / the ensemble's median error there
        "exceeds_p99_frac": 0.15,                               # tail: windows above the ensemble's p99 for that window
        "worst_ratio_to_realisations_max": 3.0}                 # no window further out than 3 x the ensemble's worst draw there
# dtype fp32-split carries 22-bit operands (hi + lo halves): held to wider bars, and reported against the fp32 bars as well
BARS_SPLIT = {"trimmed_rms_over_p90": 1.5, "median_window_ratio_to_realisations_median": 1.75, "exceeds_p99_frac": 0.25, "worst_ratio_to_realisations_max": 3.0}


def passes(st, bars=BARS):
    return all(st[k] <= v for k, v in bars.items())


def calibration(r_max, r_sumsq, count, inflate=2.0):
    """null (leave-one-out) and alternative (the left-out realisation's error x `inflate`) distributions of the statistics"""
    R = r_max.shape[0]
    null, alt = [], []
    for r in range(R):
        keep = np.arange(R) != r
        null.append(statistics(r_max[r], r_sumsq[r], r_max[keep], r_sumsq[keep], count))
        alt.append(statistics(r_max[r] * inflate, r_sumsq[r] * inflate * inflate, r_max[keep], r_sumsq[keep], count))
    return null, alt


def judge_case(fix, e_max, e_sumsq, bars=BARS):
    out = {}
    keys = tuple(BARS) + ("set_rms_percentile", "trimmed_rms_percentile")
    for head in ("plain", "peaked"):
        r_max, r_sumsq, count = fix[head + "_max"].astype(np.float64), fix[head + "_sumsq"].astype(np.float64), fix["count"].astype(np.float64)
        st = statistics(e_max[head].astype(np.float64), e_sumsq[head].astype(np.float64), r_max, r_sumsq, count)
        null, alt = calibration(r_max, r_sumsq, count)
        for name, draws in (("leave_one_out", null), ("doubled", alt)):
            st[name] = {k: [float(np.quantile([d[k] for d in draws], q)) for q in (0.0, 0.5, 0.9, 1.0)] for k in keys}
        st["bars"] = dict(bars)
        st["passes"] = bool(passes(st, bars))
        st["passes_fp32_bars"] = bool(passes(st, BARS))
        st["leave_one_out_draws_passing_frac"] = float(np.mean([passes(d, BARS) for d in null]))
        st["doubled_draws_rejected_frac"] = float(np.mean([not passes(d, BARS) for d in alt]))
        if "kinds" in fix:
            kinds = np.asarray(fix["kinds"])
            st["doubled_draws_rejected_frac_by_kind"] = {k: float(np.mean([not passes(d, BARS) for d, kk in zip(alt, kinds) if kk == k])) for k in sorted(set(kinds.tolist()))}
            st["leave_one_out_draws_passing_frac_by_kind"] = {k: float(np.mean([passes(d, BARS) for d, kk in zip(null, kinds) if kk == k])) for k in sorted(set(kinds.tolist()))}
        out[head] = st
    return out


def cmd_judge(a):
    eng = np.load(a.engine_npz)
    rep = {}
    for topology, seed in a.cases:
        fix = load_ensemble(topology, seed)
        for dtype in a.dtypes:
            key = "%s_%d_%s_" % (topology, seed, dtype)
            if key + "plain_max" not in eng:
                continue
            rep["%s:%d:%s" % (topology, seed, dtype)] = judge_case(
                fix, {h: eng[key + h + "_max"] for h in ("plain", "peaked")}, {h: eng[key + h + "_sumsq"] for h in ("plain", "peaked")},
                BARS if dtype == "fp32" else BARS_SPLIT)
    path = os.path.join(ROOT, "gpurun_out", "parity_dist_report.json")
    json.dump(rep, open(path, "w"), indent=1, sort_keys=True)
    for k, v in rep.items():
        for h, st in v.items():
            print("%-20s %-6s bulk %.2f x p90 (pct %.2f) | typical %.2f | tail %.3f | worst %.2f x max | null passing %.2f, doubled rejected %.2f | set rms %.3g (pct %.2f) max %.3g  %s" % (
                k, h, st["trimmed_rms_over_p90"], st["trimmed_rms_percentile"], st["median_window_ratio_to_realisations_median"], st["exceeds_p99_frac"],
                st["worst_ratio_to_realisations_max"], st["leave_one_out_draws_passing_frac"], st["doubled_draws_rejected_frac"], st["set_rms"],
                st["set_rms_percentile"], st["set_max"], "PASS" if st["passes"] else "FAIL"))
    print("wrote", path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=("realise", "chain", "engine", "judge"))
    ap.add_argument("--engine-draws", type=int, default=0, help="engine: also run the engine on this many channel-permuted copies of the weights")
    ap.add_argument("engine_npz", nargs="?", default=os.path.join(ROOT, "gpurun_out", "parity_dist_engine.npz"))
    ap.add_argument("--cases", default=",".join("%s:%d" % c for c in CASES))
    ap.add_argument("--realisations", type=int, default=N_REAL)
    ap.add_argument("--windows", type=int, default=N_WINDOWS)
    ap.add_argument("--dtypes", default="fp32,fp32-split")
    ap.add_argument("--force", action="store_true")
    ap.add_argument("--tag", default="", help="engine: suffix of the output file (A/B runs)")
    a = ap.parse_args()
    a.cases = [(c.split(":")[0], int(c.split(":")[1])) for c in a.cases.split(",")]
    a.dtypes = a.dtypes.split(",")
    {"realise": cmd_realise, "chain": cmd_chain, "engine": cmd_engine, "judge": cmd_judge}[a.cmd](a)


if __name__ == "__main__":
    main()
