"""The topologies the engine's descriptor accepts, as one table: tests/test_gpu_topology.py runs every row on the GPU against the
float64 oracle, tests/test_topology_cpu.py checks the oracle, the descriptor round trip and the packer on every row without one.

validate_desc (csrc/model_layout.h) accepts 1 to 8 blocks of any channel count that is a multiple of 4, conv2b widths 1 to 16, any
stride, i_bn on any block, a stem of any multiple of 8 channels, 1 to 8 recurrent layers of either kind, 2 to 5 classes and both BN
modes; the engine picks its kernels from those numbers.  The rest of the suite runs 256 channels, three blocks and five classes.  A row
here is the smallest model that reaches one of the other paths; its `why` names the path.

The bar is not taken from the engine.  Per window b, err_b = ||y_b - y64_b||_2 against oracle/nn_oracle.py in float64 (logits: over
the window's valid frames; features: over all T frames, every one of which the CNN computes); the yardstick e32 is the largest
per-window error of the same oracle run in float32 on the CPU, and a row passes with
    err_b <= FACTOR * e32 + FLOOR * ||y64_b||,    FACTOR = 4 (tests/train_cases.py: accumulation order), FLOOR = 1e-6.

What the half-precision dtypes admit is 1 -> 256 and 256 -> 256 blocks only (csrc/weight_pack.h), the shapes of the rest of the suite:
their other shapes are REFUSED rows, pinned on the CPU."""
import functools
from collections import namedtuple

import numpy as np

import chiron_amd as ca

from f16_cases import ragged

FACTOR = 4.0
FLOOR = 1e-6
WEIGHT_SEED = 83

Case = namedtuple("Case", "name spec dtype B L max_beam why")


def blocks(channels, k=3, stride=1, i_bn=None):
    """channels [c0, c1, ...] -> blocks c0 -> c1, c1 -> c2, ...; k / stride / i_bn: one value, or {block index: value} over the
    defaults 3 / 1 / first block only"""
    def pick(v, i, default):
        return v.get(i, default) if isinstance(v, dict) else default if v is None else v
    return [{"name": "res_layer%d" % (i + 1), "in": channels[i], "out": channels[i + 1], "k": pick(k, i, 3), "stride": pick(stride, i, 1),
             "i_bn": bool(pick(i_bn, i, i == 0))} for i in range(len(channels) - 1)]


def _spec(channels, k=3, stride=1, i_bn=None, kind="stack", layers=2, classes=5, bn="population", stem=None):
    return ca.ModelSpec(blocks(channels, k, stride, i_bn), kind, layers, 100, classes, bn, stem=stem)


def _table():
    rows = []

    def add(name, spec, B, L, why, max_beam=0, dtype="fp32"):
        rows.append(Case(name, spec, dtype, B, L, max_beam, why))

    # channel counts, the same in every block
    add("c128", _spec([1, 128, 128, 128]), 5, 126, "generic GEMM, no K tail, N = one tile; F(2,3) with 2 column tiles; projection K = 128", 5)
    add("c64", _spec([1, 64, 64, 64]), 5, 126, "N = half a tile; F(2,3) with 1 column tile and 2 chunks; projection K = 64", 5)
    add("c64-odd", _spec([1, 64, 64, 64]), 3, 67, "odd T: conv2b as three shifted K-segments of the generic GEMM")
    add("c320", _spec([1, 320, 320, 320]), 4, 62, "N = 2.5 tiles; F(2,3) with 5 column tiles; projection K = 320")
    add("c192", _spec([1, 192, 192, 192]), 5, 126, "N = 128 + 64: a partial column tile; F(2,3) with 3 column tiles")
    add("c192-odd", _spec([1, 192, 192, 192]), 3, 67, "the partial column tile under the shifted taps")
    add("c64-f4", _spec([1, 64, 64]), 2, 256, "F(4,3) (T = 256) with 1 column tile and 4 chunks of 16")
    add("c36", _spec([1, 36, 36, 36]), 5, 126, "K tail in every segment (cin 36 < kpad 64); N far below a tile; table of 36 breakpoints", 5)
    add("c12", _spec([1, 12, 12, 12]), 5, 67, "cin 12 < kpad 32: a row narrower than a loader lane's channel offset; odd T")
    add("c4", _spec([1, 4, 4, 4]), 4, 61, "cin 4: one float4 per row; table of 4 breakpoints")
    # channel counts that change from block to block
    add("widen", _spec([1, 64, 128, 256]), 5, 126, "conv2c + branch1 segments of different widths (128 + 64, 256 + 128); cmax is the last block's")
    add("narrow", _spec([1, 256, 192, 256]), 4, 62, "256 -> 192 on the DMA kernel with N % 128 != 0; 256 + 192 segments; cmax is not the last C")
    add("last200-stack", _spec([1, 64, 200]), 5, 61, "layer-0 projection K = 200 from a batch-major source: gemm_proj_bf16x3_kernel<13, true>; M tail")
    add("last200-multi", _spec([1, 64, 200], kind="multi"), 5, 61, "the same under the MultiRNN")
    add("last100-multi", _spec([1, 64, 100], kind="multi"), 5, 61, "layer-0 projection K = 100: the 128-tail DMA form, batch-major source")
    add("last100-stack", _spec([1, 64, 100]), 4, 62, "the same under the stack")
    add("c576", _spec([1, 576, 64]), 3, 30, "above PWL_MAX_BP: no table, conv2a lifted, conv2b on the GEMM with 3 x 18 chunks")
    # block counts
    add("blocks1", _spec([1, 64]), 5, 126, "one block: the lifted block's output is the feature tensor")
    add("blocks2", _spec([1, 64, 64]), 5, 126, "two blocks")
    add("blocks5", _spec([1] + [64] * 5), 4, 62, "five blocks: the activation buffers rotate past their count")
    add("blocks8", _spec([1] + [64] * 8), 3, 126, "CHIRON_MAX_BLOCKS blocks: MAX_SITES sites")
    # conv2b widths
    for k in (1, 2, 4, 5, 16):
        add("k%d" % k, _spec([1, 64, 64], k={1: k}), 4, 61 if k % 2 else 62,
            "conv2b of width %d on a 64-channel block: %s" % (k, "GEMM_MAX_SEG K-segments" if k == 16 else "SAME pad left %d, right %d" % ((k - 1) // 2, k // 2)))
    add("lift-k2", _spec([1, 64, 64], k={0: 2}), 4, 61, "the table with two taps: SAME pad 0 left, 1 right")
    add("lift-k16", _spec([1, 64, 64], k={0: 16}), 4, 62, "the table with 16 taps on a window shorter than four of them")
    add("lift-s16-k16", _spec([1, 64, 64], k={0: 16}, stride={0: 16}), 3, 640, "(PWL_TP - 1) * 16 + 16 = PWL_MAX_S samples: the table's limit")
    add("lift-s17", _spec([1, 64, 64], k={0: 1}, stride={0: 17}), 3, 520, "(PWL_TP - 1) * 17 + 1 > PWL_MAX_S: lifted, strided conv2b on the GEMM")
    # strides on a block with a real input tensor
    for s, Ls in ((2, (126, 127)), (3, (126, 127, 128))):
        for L in Ls:
            add("stride%d-L%d" % (s, L), _spec([1, 64, 64, 64], stride={1: s}), 4, L,
                "stride %d on block 2, L mod %d = %d: strided taps and strided branch1 on a 64-channel tensor" % (s, s, L % s))
    # BN on the shortcut
    add("ibn-block2", _spec([1, 64, 64], i_bn={0: True, 1: True}), 4, 62, "i_bn on block 2: BN folded into the fused-K shortcut segment")
    add("no-ibn-block1", _spec([1, 64, 64], i_bn={0: False, 1: False}), 4, 62, "no BN on the lifted block's shortcut: res_a = the raw filter, res_b = 0")
    # stems
    add("stem64-k1", _spec([64, 64, 64], kind="multi", stem={"k": 1, "stride": 1, "out": 64}), 4, 62, "stem of 64 channels, width 1")
    add("stem8-k64", _spec([8, 64, 64], kind="multi", stem={"k": 64, "stride": 3, "out": 8}), 4, 185, "stem of 8 channels, width 64, L mod 3 = 2; K = 8 segments")
    add("stem64-narrowing", _spec([64, 32, 32], kind="multi", stem={"k": 9, "stride": 5, "out": 64}), 4, 311,
        "the stem's output is wider than every block's: the activation buffers must hold it")
    # recurrent stacks
    for kind in ("stack", "multi"):
        for n in (1, 2, 4, 8):
            add("%s%d" % (kind, n), _spec([1, 64, 64], kind=kind, layers=n), 5, 62, "%d recurrent layers, %s: lasth ping-pong%s"
                % (n, kind, ", per-direction projections" if kind == "multi" and n > 1 else ""))
    # classes
    for K in (2, 3, 4):
        add("classes%d" % K, _spec([1, 64, 64], classes=K), 5, 62, "FC head lanes 16 .. %d, logits of stride %d, greedy over %d classes" % (16 + K - 1, K, K))
    # batch statistics
    add("batch-c192", _spec([1, 192, 192, 192], bn="batch"), 5, 126, "bn_batch.hip with 5 rows per block and 16 idle threads")
    add("batch-c64", _spec([1, 64, 64, 64], bn="batch"), 5, 126, "16 rows per block")
    add("batch-c48", _spec([1, 48, 48, 48], bn="batch"), 5, 67, "21 rows per block, 4 idle threads")
    add("batch-c1024", _spec([1, 1024, 1024], bn="batch", layers=1), 3, 20, "BN_BATCH_MAX_C: one row per block")
    add("batch-c192-wrap", _spec([1, 192], bn="batch", layers=1), 26, 400, "10 400 rows > 2048 blocks x 5: the last block's idle threads point at block 0's next row")
    add("batch-stem64", _spec([64, 32, 32], kind="multi", bn="batch", stem={"k": 9, "stride": 5, "out": 64}), 4, 311, "batch BN of a stem wider than the blocks")
    return rows


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# What the descriptor accepts and the engine refuses when it is planned or packed, before any kernel runs: (name, spec, dtype, max_beam,
# switches of the packer, "plan" | "pack", the text).  tests/test_topology_cpu.py pins every text.
_F16_NARROW = "dtype %s: block %d has %d -> %d channels; its convolution kernels are built for 1 -> 256 and 256 -> 256"
REFUSED = [
    ("fp16-192", _spec([1, 256, 192]), "fp16", 0, "", "pack", "dtype f16: block 1 has 256 -> 192 channels; the f16 kernels need multiples of 64 / 128"),
    ("split-192", _spec([1, 256, 192]), "fp32-split", 0, "", "pack", "dtype f16: block 1 has 256 -> 192 channels; the f16 kernels need multiples of 64 / 128"),
    ("fp16-in32", _spec([32, 256], stem={"k": 9, "stride": 5, "out": 32}), "fp16", 0, "", "pack",
     "dtype f16: block 0 has 32 -> 256 channels; the f16 kernels need multiples of 64 / 128"),
    ("split-in32", _spec([32, 256], stem={"k": 9, "stride": 5, "out": 32}), "fp32-split", 0, "", "pack",
     "dtype f16: block 0 has 32 -> 256 channels; the f16 kernels need multiples of 64 / 128"),
    ("fp16-128-128", _spec([1, 128, 128]), "fp16", 0, "", "pack", _F16_NARROW % ("f16", 0, 1, 128)),
    ("w2-128-128", _spec([1, 128, 128]), "fp16-w2", 0, "", "pack", _F16_NARROW % ("f16", 0, 1, 128)),
    ("split-128-128", _spec([1, 128, 128]), "fp32-split", 0, "", "pack", _F16_NARROW % ("f32-split", 0, 1, 128)),
    ("fp16-128-256", _spec([1, 128, 256]), "fp16", 0, "", "pack", _F16_NARROW % ("f16", 0, 1, 128)),
    ("w2-128-256", _spec([1, 128, 256]), "fp16-w2", 0, "", "pack", _F16_NARROW % ("f16", 0, 1, 128)),
    ("split-128-256", _spec([1, 128, 256]), "fp32-split", 0, "", "pack", _F16_NARROW % ("f32-split", 0, 1, 128)),
    ("split-256-128-in", _spec([1, 256, 256, 128]), "fp32-split", 0, "", "pack", _F16_NARROW % ("f32-split", 2, 256, 128)),
    ("w2-k9", _spec([1, 256, 256], k={1: 9}), "fp16-w2", 0, "", "pack",
     "dtype f16-w2: block 1: conv2b width 9 unsupported (1..8: hi and lo weights take two K-segments per tap)"),
    ("w2-lift-k13-nopwl", ca.rna_default_spec(), "fp16-w2", 0, "p", "pack",
     "dtype f16-w2: block 0: conv2b width 13 unsupported (1..8: hi and lo weights take two K-segments per tap)"),
    ("batch-fp16", ca.dna_default_spec(bn_mode="batch"), "fp16", 0, "", "pack", "bn_mode=batch is implemented for dtype f32 only"),
    ("batch-split", ca.dna_default_spec(bn_mode="batch"), "fp32-split", 0, "", "pack", "bn_mode=batch is implemented for dtype f32 only"),
    ("batch-c1028", _spec([1, 1028], bn="batch", layers=1), "fp32", 0, "", "plan",
     "bn_mode=batch: a convolution with 1028 output channels; the batch-statistics kernels cover at most 1024"),
    ("batch-stem1032", _spec([1032, 64], bn="batch", layers=1, stem={"k": 3, "stride": 1, "out": 1032}), "fp32", 0, "", "plan",
     "bn_mode=batch: a convolution with 1032 output channels; the batch-statistics kernels cover at most 1024"),
    ("beam-classes4", _spec([1, 64, 64], classes=4), "fp32", 5, "", "plan",
     "max_beam 5 with classes 4: the beam search kernels are built for 5 classes (greedy decoding takes 2..5)"),
]
# the packer takes these (the table's k13 / w2 row runs on the GPU in the rest of the suite): fp16-w2 with a wide conv2b in the table form
ADMITTED_BY_THE_PACKER = [("w2-lift-k13", ca.rna_default_spec(), "fp16-w2", "")]


# ---- the rules the engine's profile and the packer's geometry are held to (csrc/weight_pack.h, csrc/kernels.h pwl_covers)

def block_lengths(spec, L):
    """[(t_in, t_out)] of every block"""
    t = L
    if spec.stem:
        t = -(-t // spec.stem["stride"])
    out = []
    for b in spec.blocks:
        out.append((t, -(-t // b["stride"])))
        t = out[-1][1]
    return out


def wino_blocks(spec, L, dtype="fp32"):
    """indices of the blocks whose conv2b runs in a Winograd form: 1 x 3, stride 1, in == out, a multiple of 64 channels, not the
    lifted block, an even input length, fp32 with population BN"""
    if dtype != "fp32" or spec.bn_mode != "population":
        return []
    return [i for i, (b, (t_in, _)) in enumerate(zip(spec.blocks, block_lengths(spec, L)))
            if b["in"] > 1 and b["k"] == 3 and b["stride"] == 1 and b["in"] == b["out"] and b["out"] % 64 == 0 and t_in % 2 == 0]


PWL_TP, PWL_MAX_BP, PWL_MAX_S = 32, 512, 512      # csrc/kernels.h; tests/test_topology_cpu.py reads them out of the source


def table_block(spec):
    """the lifted block runs as the piecewise-linear table"""
    b = spec.blocks[0]
    return (b["in"] == 1 and spec.bn_mode == "population" and b["out"] <= PWL_MAX_BP and (PWL_TP - 1) * b["stride"] + b["k"] <= PWL_MAX_S)


def expected_profile(spec, L, dtype="fp32"):
    """{bucket: launches} of one batch for the buckets that tell the forms apart"""
    lifted = spec.blocks[0]["in"] == 1
    pop = spec.bn_mode == "population"
    return {"conv_wino": len(wino_blocks(spec, L, dtype)), "conv1_pwl": 1 if table_block(spec) else 0,
            "conv_lift": 1 if pop and (spec.stem or (lifted and not table_block(spec))) else 0,
            "lstm_recurrence": spec.rnn_layers, "fc_head": 1}


# ---- inputs and references, computed once per case and shared (read only)

@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> (spec, weights, signal [B, L], seq_len [B], T): ragged windows (seq_len T, 1, 0 first) as tests/f16_cases.ragged builds them"""
    c = BY_NAME[name]
    x, sl, T = ragged(c.spec, c.L, c.B, seed=7000 + c.L + 7 * c.B)
    w = ca.synthetic_weights(c.spec, seed=WEIGHT_SEED)
    first = c.spec.blocks[0]
    if first["in"] == 1 and not first["i_bn"]:
        # synthetic_weights leaves a shortcut without BN at the raw signal's scale (~500 x the filter): bring it to O(1), where the
        # recurrent gates do not saturate and an error in the features still reaches the logits
        w[first["name"] + "/branch1/conv1/weights"] = (w[first["name"] + "/branch1/conv1/weights"] / ca.model.SIGNAL_MEAN).astype(np.float32)
    return c.spec, w, x, sl, T


@functools.lru_cache(maxsize=None)
def reference(name, acc="float64"):
    """-> (features [B, T, C], logits [B, T, K]) of oracle/nn_oracle.py accumulating in `acc`"""
    from oracle import nn_oracle
    spec, w, x, sl, T = inputs(name)
    logits, _, fea, _ = nn_oracle.inference(x, sl, spec.to_dict(), w, dtype=np.dtype(acc).type, return_all=True)
    return fea, logits


def window_errors(got, ref64, sl=None):
    """-> (err_b, norm_b): per window the L2 error and the L2 norm of the reference, over the first sl[b] frames (None: all)"""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    B, T = ref64.shape[:2]
    mask = np.ones((B, T), bool) if sl is None else np.arange(T)[None, :] < np.asarray(sl)[:, None]
    d = np.where(mask[..., None], got - ref64, 0.0).reshape(B, -1)
    r = np.where(mask[..., None], ref64, 0.0).reshape(B, -1)
    return np.sqrt((d * d).sum(axis=1)), np.sqrt((r * r).sum(axis=1))


def yardstick(name):
    """-> {"features": e32, "logits": e32}: the largest per-window error of the float32 oracle against the float64 one"""
    _, _, _, sl, _ = inputs(name)
    f64, l64 = reference(name)
    f32, l32 = reference(name, "float32")
    return {"features": float(window_errors(f32, f64)[0].max()), "logits": float(window_errors(l32, l64, sl)[0].max())}


def judge(got, ref64, e32, sl=None):
    """-> (passes, largest err_b / e32, err_b, bound_b)"""
    err, norm = window_errors(got, ref64, sl)
    bound = FACTOR * e32 + FLOOR * norm
    return bool((err <= bound).all()), float(err.max() / e32) if e32 > 0 else 0.0, err, bound
