"""Block 1's table convolution (csrc/pwl.hip, the table of csrc/weight_pack.h) against the formula it tabulates.  numpy only.

With population BN the first block's conv2a + conv2b are evaluated as a piecewise-linear table of the signal value s:
    y2b[pos][n] = relu(sh[n] + sum_tap f[tap][n](s[pos * stride + tap - left])),   f[tap][n](s) = sum_c W2b'[tap][c][n] relu(s a[c] + b[c]).
`formula` is f, from the weights (folding: f16_ref.folded); `table_eval` restates what the kernel computes from the packed table, which
tests/native/pwl_table_dump.cpp reads back on the host (`dump`); `samples_for` lists the signal values at which a table can go wrong:
on, next to and between the breakpoints, at and around 0, and far outside.

The bar (tests/test_pwl_cpu.py, tests/test_gpu_pwl.py) is that of tests/fp32_cases.py, taken PER POSITION:
    ||got - ref64||_2 over the channels of one position  <=  FACTOR * ||ref32 - ref64||_2  +  FLOOR * ||ref64||_2,      FLOOR = 1e-6,
ref32 = e32 = the same formula accumulated in float32.  FACTOR = fp32_cases.factors_from's max(4, 1.5 x largest) over the largest
err / e32 that `table_eval` reaches on the CPU, at the level of y2b and chained through the rest of the block (conv2c + the signal
branch in float32), over WEIGHT_SETS and DRAWS channel orders of the float32 yardstick (tools/pwl_table_accuracy.py writes
profiles/pwl_table_accuracy.json; no HIP result enters it).  Positions whose error is below the floor do not enter a ratio.

The half format (fp16 engine) cannot be held per position by a ratio of two roundings to halves: a value within accumulation noise of
a rounding tie flips in one realisation and not in the other, the float32 yardstick is exactly right at most positions and a whole
half-ulp off at the others, and so is every correct engine, at other positions.  `half_check` is therefore per ELEMENT and aware of
ties: with F the float64 restatement's value BEFORE its rounding to a half (f16_ref.cnn, its own roundings up to there),
    |got - F| <= ulp16(F) / 2 + FACTOR * e32(pos) + FLOOR * ||F(pos)||_2 + amb(pos, n),
e32(pos) the per-position float32 error of the unrounded stage, amb the effect of the conv2b outputs of that position that lie within
their own allowance of a tie (either neighbour is a correct rounding): the result must be a nearest half of the reference wherever the
reference is further from a tie than float32 arithmetic can move it."""
import atexit
import functools
import json
import os
import shutil
import subprocess
import tempfile
from collections import OrderedDict

import numpy as np

import chiron_amd as ca
from oracle import nn_oracle

import f16_ref
import fp32_ref
from f16_cases import FLOOR, ROOT

JSON = os.path.join(ROOT, "profiles", "pwl_table_accuracy.json")
DRAWS = 8
HALF_CAP = 3e4                 # the half formats: |y2b| and |features| of the float64 reference stay below it (65504 is a half's largest)
BLOCK = "res_layer1"
DTYPES = {"fp32": 0, "fp16": 1, "fp32-split": 2}


# ---- the weight sets

def one_block(spec):
    """the first block alone, one recurrent layer behind it: Engine.features() is then block 1's output"""
    return ca.ModelSpec(spec.blocks[:1], spec.rnn_kind, 1, spec.hidden, spec.classes, spec.bn_mode)


def _copy(w):
    return OrderedDict((k, np.array(v, copy=True)) for k, v in w.items())


def _random(spec, plant):
    import test_weight_pack_cpu as wp
    w = wp.random_weights(spec, 1000)
    if plant:
        clean = _copy(w)
        w = wp.planted(spec, w)
        # planted() also gives one conv2c row a shift of 1e30 (the split GEMM's row scaling): one channel of 1e30 would be the whole of
        # every position's norm and hide the table behind it; block 1's conv2c is put back, every plant of conv2a stays
        for k in w:
            if k.startswith(BLOCK + "/branch2/conv2c"):
                w[k] = clean[k]
    else:
        w[BLOCK + "/branch2/conv2a_bn/pop_mean"][:] = 0.0          # zero-centred: breakpoints -offset / (W inv) on both sides of 0
    return w


def _equal_breakpoints(spec):
    w = _copy(ca.synthetic_weights(spec, seed=7))
    a, bn = BLOCK + "/branch2/conv2a/weights", BLOCK + "/branch2/conv2a_bn/"
    w[a][0, 0, 0, 1] = w[a][0, 0, 0, 0]                            # channels 0 and 1: the same (a, b)
    for leaf in ("scale", "offset", "pop_mean", "pop_var"):
        w[bn + leaf][1] = w[bn + leaf][0]
    w[a][0, 0, 0, 3] = w[a][0, 0, 0, 2]                            # channel 3 = (2 a, 2 b) of channel 2: scale and offset doubled, exactly
    for leaf in ("pop_mean", "pop_var"):
        w[bn + leaf][3] = w[bn + leaf][2]
    for leaf in ("scale", "offset"):
        w[bn + leaf][3] = 2 * w[bn + leaf][2]
    return w


def _no_breakpoints(spec):
    w = _copy(ca.synthetic_weights(spec, seed=7))
    w[BLOCK + "/branch2/conv2a/weights"][:] = 0.0                  # every a == 0: constant channels of either sign of b, one row
    return w


# name -> (topology, weights of the three-block spec); the engines and the restatements take the first block of it
WEIGHT_SETS = OrderedDict([
    ("synthetic-dna", ("dna", lambda s: ca.synthetic_weights(s, seed=7))),
    ("synthetic-rna", ("rna", lambda s: ca.synthetic_weights(s, seed=7))),
    ("zero-centred", ("dna", lambda s: _random(s, False))),
    ("planted", ("dna", lambda s: _random(s, True))),
    ("equal-breakpoints", ("dna", _equal_breakpoints)),
    ("no-breakpoints", ("dna", _no_breakpoints)),
])


@functools.lru_cache(maxsize=None)
def weight_set(name):
    """-> (the one-block spec, weights); shared: read only"""
    topology, make = WEIGHT_SETS[name]
    full = {"dna": ca.dna_default_spec, "rna": ca.rna_default_spec}[topology]()
    return one_block(full), make(full)


# ---- the table, read back from the packer

def rocm_prefix():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")     # csrc/Makefile's
    return os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))


@functools.lru_cache(maxsize=None)
def dump_exe():
    """tests/native/pwl_table_dump.cpp, built plain with the ROCm host compiler into a temporary directory, once per process"""
    rocm = rocm_prefix()
    where = tempfile.mkdtemp(prefix="pwl_table_dump_")
    atexit.register(shutil.rmtree, where, ignore_errors=True)
    exe = os.path.join(where, "pwl_table_dump")
    cmd = [os.path.join(rocm, "llvm", "bin", "clang++"), "-x", "c++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
           os.path.join(ROOT, "tests", "native", "pwl_table_dump.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def dump(spec, weights, segment_len, dtype="fp32", switches="-"):
    """block 1's table as the packer builds it -> {"nbp", "k", "c", "stride", "left", "bp" [max(nbp, 1)], "ref" [nbp + 1],
    "tab" [nbp + 1, k, c, 2] (alpha, f(ref)), "shift" [c]}"""
    with tempfile.TemporaryDirectory(prefix="pwl_dump_") as d:
        with open(os.path.join(d, "desc"), "wb") as f:
            f.write(bytes(spec.to_c()))
        spec.pack(weights).tofile(os.path.join(d, "blob"))
        out = os.path.join(d, "out")
        r = subprocess.run([dump_exe(), os.path.join(d, "desc"), os.path.join(d, "blob"), str(segment_len), str(DTYPES[dtype]), switches, out],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
        head = np.fromfile(out, dtype=np.int32, count=9)
        body = np.fromfile(out, dtype=np.float32, offset=36)
    nbp, k, c, stride, left = (int(v) for v in head[:5])
    n = [int(v) for v in head[5:]]
    assert body.size == sum(n) and n == [max(nbp, 1), nbp + 1, (nbp + 1) * k * c * 2, c], (head, body.size)
    at = np.cumsum([0] + n)
    bp, ref, tab, shift = (body[at[i]:at[i + 1]] for i in range(4))
    return {"nbp": nbp, "k": k, "c": c, "stride": stride, "left": left, "bp": bp, "ref": ref, "tab": tab.reshape(nbp + 1, k, c, 2), "shift": shift}


@functools.lru_cache(maxsize=None)
def set_dump(name, segment_len):
    spec, w = weight_set(name)
    return dump(spec, w, segment_len)


# ---- the formula

def folded_block(weights, block=BLOCK, i_bn=True):
    """-> {"a", "b" [C]: conv2a's folded scale and shift; "w2b" [k, C, C], "sh2b"; "w2c" [C, C], "sh2c"; "w1", "sh1" [C]} in float32"""
    wa, sha = f16_ref.folded(weights, block + "/branch2/conv2a", True)
    wb, shb = f16_ref.folded(weights, block + "/branch2/conv2b", True)
    wc, shc = f16_ref.folded(weights, block + "/branch2/conv2c", True)
    w1, sh1 = f16_ref.folded(weights, block + "/branch1/conv1", i_bn)
    return {"a": wa[0, 0], "b": sha, "w2b": wb, "sh2b": shb, "w2c": wc[0], "sh2c": shc, "w1": w1[0, 0], "sh1": sh1}


def formula(s, weights, spec, acc=np.float64, draw=None, scale=False):
    """y2b's pre-activation per tap, f[tap][n](s) = sum_c W2b'[tap][c][n] relu(s a[c] + b[c]) -> [len(s), k, C] in `acc`: float64 is the
    reference, float32 the yardstick e32.  draw: the channels c in a drawn order (another float32 realisation).  scale: the sum of
    the terms' magnitudes instead, sum_c |W2b'| relu(.), what a rounding of this sum is relative to."""
    fb = folded_block(weights, spec.blocks[0]["name"], spec.blocks[0]["i_bn"])
    dt = np.dtype(acc).type
    a1 = np.maximum(np.asarray(s, dtype=acc)[:, None] * fb["a"].astype(acc) + fb["b"].astype(acc), dt(0))
    w = fb["w2b"].astype(acc)
    if scale:
        w = np.abs(w)
    if draw is not None:
        p = draw.permutation(a1.shape[1])
        a1, w = np.ascontiguousarray(a1[:, p]), np.ascontiguousarray(w[:, p])
    return np.stack([a1 @ w[tap] for tap in range(w.shape[0])], axis=1)


def sum_taps(taps, shift, stride, left, acc, pad_taps=None):
    """taps [B, L, k, C]: every sample's k tap values -> y2b [B, T, C] in `acc`: onto `shift`, the taps in order, ReLU.  A tap in
    the SAME padding is skipped (the padding is of conv2a's OUTPUT: zeros), or takes pad_taps [k, C] (the mutation)."""
    B, L, k, C = taps.shape
    T = -(-L // stride)
    dt = np.dtype(acc).type
    y = np.broadcast_to(np.asarray(shift, dtype=acc), (B, T, C)).copy()
    t = np.arange(T)
    for tap in range(k):
        idx = t * stride + tap - left
        ok = (idx >= 0) & (idx < L)
        y[:, ok] = y[:, ok] + taps[:, idx[ok], tap].astype(acc)
        if pad_taps is not None and (~ok).any():
            y[:, ~ok] = y[:, ~ok] + pad_taps[tap].astype(acc)
    return np.maximum(y, dt(0))


def y2b_formula(x, weights, spec, acc=np.float64, draw=None):
    """conv2b's output of the windows x [B, L] by the formula, in `acc`; the left pad is nn_oracle.same_padding's"""
    blk = spec.blocks[0]
    B, L = x.shape
    taps = formula(x.reshape(-1), weights, spec, acc, draw).reshape(B, L, blk["k"], -1)
    sh = f16_ref.fold_bn(weights, blk["name"] + "/branch2/conv2b", True)[1]
    return sum_taps(taps, sh, blk["stride"], nn_oracle.same_padding(L, blk["k"], blk["stride"])[1], acc)


def y2b_magnitude(x, weights, spec):
    """|sh[n]| + sum over the taps inside the window of sum_c |W2b'[tap][c][n]| relu(.): what a rounding of conv2b's sum is relative to"""
    blk = spec.blocks[0]
    B, L = x.shape
    taps = formula(x.reshape(-1), weights, spec, scale=True).reshape(B, L, blk["k"], -1)
    sh = np.abs(f16_ref.fold_bn(weights, blk["name"] + "/branch2/conv2b", True)[1].astype(np.float64))
    return sum_taps(taps, sh, blk["stride"], nn_oracle.same_padding(L, blk["k"], blk["stride"])[1], np.float64)


def block_tail(y2b, x, weights, spec, acc, mode=None):
    """the rest of the block from conv2b's output: conv2c + the signal branch, BEFORE the ReLU, in `acc`.  mode None: the fp32 engine
    (fp32_ref.cnn: sig * res_a + res_b added to the finished sum); "fp16": conv2c's weights as halves, both shifts folded in fp32
    into one (f16_ref.cnn)."""
    blk = spec.blocks[0]
    fb = folded_block(weights, blk["name"], blk["i_bn"])
    s = blk["stride"]
    sig = np.asarray(x, dtype=acc)[:, 0:(y2b.shape[1] - 1) * s + 1:s, None]
    y = np.asarray(y2b, dtype=acc)
    if mode is None:
        return y @ fb["w2c"].astype(acc) + fb["sh2c"].astype(acc) + (sig * fb["w1"].astype(acc) + fb["sh1"].astype(acc))
    wc = f16_ref.weight_rounding(mode)(fb["w2c"]).astype(acc)
    return y @ wc + (fb["sh2c"] + fb["sh1"]).astype(np.float32).astype(acc) + sig * fb["w1"].astype(acc)


# ---- the kernel's arithmetic

MUTATIONS = OrderedDict([
    ("row+1", "the row above the sample's interval"),
    ("neighbour-ref", "the sample's own row, the reference point of the row above"),
    ("pitch", "the row pitch off by one tap: row iv at (iv * (k - 1) + tap) * C"),
    ("pad-at-zero", "the taps in the SAME padding evaluated at s = 0 instead of skipped"),
    ("ref-lower", "s - ref with ref forced to the interval's lower bound"),
])


def intervals(s, d, tie="<"):
    """the row of every sample: the number of breakpoints < s (pwl.hip's binary search); tie "<=": the harmless variant"""
    return np.searchsorted(d["bp"][:d["nbp"]], np.asarray(s, dtype=np.float32), side="left" if tie == "<" else "right")


def table_taps(s, d, mutate=None, tie="<"):
    """-> [len(s), k, C] float32: per sample and tap fmaf(alpha, s - ref, f(ref)) from the sample's row, ss = s - ref in float32.  The
    product of two floats is exact in float64 and the sum is rounded to float64 and then to float32: fmaf up to a double rounding."""
    s = np.asarray(s, dtype=np.float32)
    nbp, k, C = d["nbp"], d["k"], d["c"]
    iv = intervals(s, d, tie)
    row, ref = iv, d["ref"][iv]
    if mutate == "row+1":
        row = np.minimum(iv + 1, nbp)
    elif mutate == "neighbour-ref":
        ref = d["ref"][np.minimum(iv + 1, nbp)]
    elif mutate == "ref-lower":
        lower = np.concatenate([d["ref"][:1], d["bp"][:nbp]]).astype(np.float32)       # row 0 has none: it keeps its own
        ref = np.where(np.isfinite(lower[iv]), lower[iv], d["ref"][iv])
    ss = (s - ref).astype(np.float32)
    if mutate == "pitch":
        flat = d["tab"].reshape(-1, C, 2)
        tab = flat[(iv * (k - 1))[:, None] + np.arange(k)[None, :]]
    else:
        tab = d["tab"][row]
    return (tab[..., 0].astype(np.float64) * ss[:, None, None].astype(np.float64) + tab[..., 1].astype(np.float64)).astype(np.float32)


def table_eval(x, d, mutate=None, tie="<"):
    """the kernel restated on windows x [B, L] -> y2b [B, T, C] float32: the interval of every sample, one fused multiply-add per tap,
    the taps added in order onto the shift, the taps in the SAME padding skipped, ReLU"""
    x = np.asarray(x, dtype=np.float32)
    B, L = x.shape
    taps = table_taps(x.reshape(-1), d, mutate, tie).reshape(B, L, d["k"], d["c"])
    pad = table_taps(np.zeros(1, np.float32), d)[0] if mutate == "pad-at-zero" else None
    return sum_taps(taps, d["shift"], d["stride"], d["left"], np.float32, pad)


def applies(mutation, d, x):
    """whether a mutation changes anything the windows x can show: a row above to take, a padded tap, a row whose reference point is
    not its lower bound"""
    if mutation in ("row+1", "neighbour-ref", "pitch"):
        return d["nbp"] >= 1
    if mutation == "pad-at-zero":
        L = x.shape[1]
        return (-(-L // d["stride"]) - 1) * d["stride"] + d["k"] > L
    rows = np.unique(intervals(x.reshape(-1), d))
    rows = rows[rows > 0]
    return bool(np.any(np.isfinite(d["bp"][rows - 1]) & (d["bp"][rows - 1] != d["ref"][rows])))


# ---- the samples

def _bits_unique(v):
    v = np.asarray(v, dtype=np.float32)
    _, keep = np.unique(v.view(np.uint32), return_index=True)
    return v[np.sort(keep)]


EXTRAS = (0.0, -0.0, 1e-30, -1e-30, 0.37, -0.37, 2.5, -2.5, 123.456, -77.77, 511.5, 200.0, 1000.0, 1e4, -1e4, -32768.0, 32767.0)


def samples_for(d):
    """float32 values: every finite breakpoint, its two nextafter neighbours, every midpoint of neighbouring finite breakpoints, one
    below the first and one above the last, +-0, +-1e-30, non-integers of either sign, and the ends of the signal's range"""
    bp = d["bp"][:d["nbp"]]
    bp = bp[np.isfinite(bp)]
    parts = [np.asarray(EXTRAS, dtype=np.float32)]
    if bp.size:
        inf = np.float32(np.inf)
        parts += [bp, np.nextafter(bp, -inf), np.nextafter(bp, inf), ((bp[:-1].astype(np.float64) + bp[1:]) / 2).astype(np.float32),
                  np.asarray([bp[0] - np.float32(1), bp[-1] + np.float32(1)], dtype=np.float32)]
    v = _bits_unique(np.concatenate(parts))
    assert np.isfinite(v).all()
    return v


def samples_capped(d, weights, spec, cap=HALF_CAP):
    """samples_for without the values at which the float64 reference of a constant window, |shift| + sum_tap |f[tap][n](s)| or the
    block's output, passes `cap`: the half formats' set -> (kept, dropped)"""
    s = samples_for(d)
    blk = spec.blocks[0]
    f = formula(s, weights, spec)
    sh = f16_ref.fold_bn(weights, blk["name"] + "/branch2/conv2b", True)[1].astype(np.float64)
    y = np.maximum(sh + f.sum(axis=1), 0.0)
    fea = block_tail(y[:, None, :], s[:, None], weights, spec, np.float64)[:, 0]
    big = np.maximum((np.abs(sh) + np.abs(f).sum(axis=1)).max(axis=1), np.abs(fea).max(axis=1)) > cap
    return s[~big], s[big]


def reachable_rows(d):
    """the rows 0 .. nbp whose interval (bp[iv - 1], bp[iv]] holds a finite float32 value"""
    nbp, bp = d["nbp"], d["bp"]
    out = []
    for iv in range(nbp + 1):
        if nbp and ((iv == 0 and bp[0] == -np.inf) or (iv == nbp and bp[nbp - 1] == np.inf) or (0 < iv < nbp and bp[iv - 1] == bp[iv])):
            continue
        out.append(iv)
    return out


def ref_kinds(d, rows):
    """how many of `rows` have their reference point at 0, at their lower bound, at their upper bound"""
    nbp, bp, ref = d["nbp"], d["bp"], d["ref"]
    n = {"zero": 0, "lower": 0, "upper": 0}
    for iv in rows:
        if ref[iv] == 0 and not (iv > 0 and bp[iv - 1] == 0) and not (iv < nbp and bp[iv] == 0):
            n["zero"] += 1
        elif iv > 0 and ref[iv] == bp[iv - 1]:
            n["lower"] += 1
        elif iv < nbp and ref[iv] == bp[iv]:
            n["upper"] += 1
    return n


# ---- the windows

def windows(samples, spec, L, B, seed):
    """B ragged windows of L samples holding `samples` in a shuffled order, cyclically: lengths as f16_cases.ragged cuts them (L, one
    frame's worth, 0, then random; the last one whole again from B = 4), zero past each window's samples.  The first and the last k
    samples of the whole windows hold the values of largest magnitude of either sign, so that padded taps sit next to them.
    -> (x [B, L] float32, lengths, how many distinct samples were placed)"""
    blk = spec.blocks[0]
    k, T = blk["k"], spec.output_len(L)
    rng = np.random.RandomState(seed)
    order = np.asarray(samples, dtype=np.float32)[rng.permutation(len(samples))]
    ln = rng.randint(0, L + 1, size=B)
    head = [L, min(L, int(np.ceil(L / T))), 0][:B]
    ln[:len(head)] = head
    if B >= 4:
        ln[B - 1] = L
    by_size = order[np.argsort(-np.abs(order.astype(np.float64)), kind="stable")]
    extremes = np.concatenate([by_size[by_size > 0][:2], by_size[by_size < 0][:2]])
    if extremes.size == 0:
        extremes = by_size[:1]
    x = np.zeros((B, L), dtype=np.float32)
    reserved = np.zeros((B, L), dtype=bool)
    n = 0
    for b in np.flatnonzero(ln == L):
        for i in sorted(set(list(range(min(k, L))) + list(range(max(0, L - k), L)))):
            x[b, i] = extremes[n % extremes.size]
            reserved[b, i] = True
            n += 1
    free = (np.arange(L)[None, :] < ln[:, None]) & ~reserved
    x[free] = order[np.arange(int(free.sum())) % len(order)]
    return x, ln, min(int(free.sum()), len(order))


# ---- the bar

def per_position(got, ref64, ref32, factor):
    """-> {"err", "e32", "scale" [positions], "ok" [positions], "ratio": the largest err / e32 over the positions above the floor (inf
    where the yardstick is exact and the result is not), "worst": its position}"""
    g, r, q = (np.asarray(v, dtype=np.float64).reshape(-1, np.shape(v)[-1]) for v in (got, ref64, ref32))
    err, e32, scale = np.linalg.norm(g - r, axis=1), np.linalg.norm(q - r, axis=1), np.linalg.norm(r, axis=1)
    ok = err <= factor * e32 + FLOOR * scale
    above = err > FLOOR * scale
    with np.errstate(divide="ignore", invalid="ignore"):
        ratios = np.where(above, err / e32, 0.0)
        raw = np.where(e32 > 0, err / e32, 0.0)                    # for the record: the positions below the floor too
    worst = int(np.argmax(ratios)) if ratios.size else 0
    return {"err": err, "e32": e32, "scale": scale, "ok": ok, "ratio": float(ratios.max()) if ratios.size else 0.0, "worst": worst,
            "raw": float(raw.max()) if raw.size else 0.0, "finite": bool(np.isfinite(g).all())}


def ulp16(v):
    """the spacing of halves at |v| (subnormal spacing 2^-24 below 2^-14)"""
    v = np.abs(np.asarray(v, dtype=np.float64))
    _, e = np.frexp(v)
    return np.ldexp(1.0, np.where(v > 0, np.maximum(e - 11, -24), -24))


def half_sites(x, weights, spec, table=True, acc=np.float64):
    """f16_ref.cnn of the one-block spec -> (the values BEFORE each stored rounding, in order; the output).  Table form: [y2b, the
    block's output]; lifted: [conv2a, y2b, the output]."""
    rec = []

    def aq(a):
        rec.append(np.array(a, copy=True))
        return f16_ref.f16(a)
    out = f16_ref.cnn(x, spec.to_dict(), weights, acc, None, "fp16", table, aq=aq)
    return rec, out


def half_check(got, x, weights, spec, factor):
    """the fp16 engine's table form, per element (module docstring) -> {"ok" [B, T, C], "ambiguous": positions with a live conv2b output within its
    allowance of a tie, "ratio": the largest (|got - F| - ulp16 / 2 - amb) / e32(pos) over the elements above the floor}"""
    (B64, F64), _ = half_sites(x, weights, spec)
    y32 = y2b_formula(x, weights, spec, np.float32)                                     # the float32 yardstick of conv2b, unrounded
    nrm = lambda a: np.linalg.norm(np.asarray(a, dtype=np.float64), axis=-1, keepdims=True)
    # per element: the bar with the sum of the terms' magnitudes as the scale, |sh| + sum_tap sum_c |W2b'| relu(.)
    allow_b = factor * np.abs(y32 - B64) + FLOOR * y2b_magnitude(x, weights, spec)
    b16 = f16_ref.f16(B64)
    pre32 = np.maximum(block_tail(b16, x, weights, spec, np.float32, "fp16"), np.float32(0))   # the rest in float32 from the SAME halves
    pre64 = np.maximum(block_tail(b16, x, weights, spec, np.float64, "fp16"), 0.0)
    assert np.allclose(pre64, F64, rtol=1e-12, atol=1e-12)                              # block_tail is f16_ref.cnn's arithmetic
    e32, scale = nrm(pre32 - F64), nrm(F64)
    # a conv2b output within its allowance of a tie may round either way: its other neighbour moves the output by one ulp16 times the weight
    lo = b16 - ulp16(B64) * (b16 > B64)                                                 # the half below B64 (b16 is below or above it)
    tie = lo + ulp16(B64) / 2
    amb_c = np.abs(B64 - tie) <= allow_b
    wc = np.abs(f16_ref.weight_rounding("fp16")(folded_block(weights, spec.blocks[0]["name"], spec.blocks[0]["i_bn"])["w2c"]))
    amb = (amb_c * ulp16(B64)) @ wc
    dev = np.abs(np.asarray(got, dtype=np.float64) - F64)
    wide = dev - ulp16(F64) / 2 - amb                                                   # what float32 arithmetic has to answer for
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(wide > FLOOR * scale, wide / e32, 0.0)
    return {"ok": wide <= factor * e32 + FLOOR * scale, "ambiguous": int((amb_c & (B64 > 0)).any(axis=-1).sum()),
            "ambiguous_share_of_live_elements": float((amb_c & (B64 > 0)).sum() / max(1, int((B64 > 0).sum()))),
            "ratio": float(ratio.max()) if ratio.size else 0.0, "elements": int(dev.size), "finite": bool(np.isfinite(got).all())}


# ---- the committed factor

def committed():
    with open(JSON) as f:
        return json.load(f)


def factor_of(largest):
    """fp32_cases.factors_from's construction on one figure: max(4, 1.5 x the largest ratio)"""
    import fp32_cases
    row = {"stage": "cnn", "l2": {"max_over_median": largest}, "channel": {"max_over_median": largest}}
    return fp32_cases.factors_from({"pwl": {"cnn": row}})[1]["cnn"]["l2"]


CPU_L = {"dna": 130, "rna": 160}        # the window the CPU ensemble lays the samples out in
CPU_SEED = 20


def cpu_case(name, capped=False):
    """-> (spec, weights, dump, x [B, L]): every sample of the set at least once, in ragged windows"""
    spec, w = weight_set(name)
    L = CPU_L[WEIGHT_SETS[name][0]]
    d = set_dump(name, L)
    s = samples_capped(d, w, spec)[0] if capped else samples_for(d)
    B = 4
    while True:
        x, ln, placed = windows(s, spec, L, B, CPU_SEED)
        if placed == len(s):
            return spec, w, d, x
        B += 2


def cpu_ratios(name, draws=DRAWS):
    """the largest err / e32 of table_eval on one weight set, over the plain float32 yardstick and `draws` drawn ones ->
    {"taps": per sample and tap, "y2b": per position, "features": per position, chained through the rest of the block}"""
    spec, w, d, x = cpu_case(name)
    sd = spec.to_dict()
    s = _bits_unique(x.reshape(-1))
    t64, tt = formula(s, w, spec), table_taps(s, d)
    y64, f64 = y2b_formula(x, w, spec), fp32_ref.cnn(x, sd, w)
    y = table_eval(x, d)
    fea = np.maximum(block_tail(y, x, w, spec, np.float32), np.float32(0))
    out = {"taps": 0.0, "y2b": 0.0, "features": 0.0, "samples": int(len(s)), "positions": int(y.shape[0] * y.shape[1]),
           "below_the_floor_too": {"taps": 0.0, "y2b": 0.0, "features": 0.0}}
    for seed in [None] + [100 + i for i in range(draws)]:
        draw = (lambda: None if seed is None else np.random.default_rng(seed))
        for level, j in (("taps", per_position(tt, t64, formula(s, w, spec, np.float32, draw()), 1.0)),
                         ("y2b", per_position(y, y64, y2b_formula(x, w, spec, np.float32, draw()), 1.0)),
                         ("features", per_position(fea, f64, fp32_ref.cnn(x, sd, w, np.float32, draw()), 1.0))):
            out[level] = max(out[level], j["ratio"])
            out["below_the_floor_too"][level] = max(out["below_the_floor_too"][level], j["raw"])
    return out
