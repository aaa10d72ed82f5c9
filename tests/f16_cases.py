"""Shared set-up of the f16-engine reference tests: the cases, the forms, the metrics and the bar.

tests/f16_ref.py restates the fp16 / fp16-w2 engines in float64 with their own roundings; the bar of tests/test_gpu_f16_ref.py is not
derived from the code under test: per case and stage, e_q = the error of the SAME restatement accumulated in float32 against the
float64 one, and the HIP result must satisfy
    m(got - ref64) <= FACTOR * m(ref32 - ref64) + FLOOR * scale,        FLOOR = 1e-6,
for two metrics m: "l2" (the tensor's L2 norm; scale = ||ref64||) and "channel" (the largest per-output-channel L2 norm; scale =
rms(ref64) * sqrt(rows) = ||ref64|| / sqrt(channels): per-channel RELATIVE error is useless where ReLU leaves dead channels).
Both run over the distinct (reference row, result row) pairs of a tensor (`measures`): repeated rows would let one rounding tie count
hundreds of times and the ensemble's factor grow to 40, under which a lost shift passes at most conv sites.
FACTOR = max(4, 1.5 x the largest max / median of a float32 ensemble), per stage and metric, is computed on the CPU by
tools/f16_ref_accuracy.py and committed in profiles/f16_ref_accuracy.json.  lasth and the logits are compared on the valid frames;
at and past a row's seq_len lasth is 0 and the logits are the head's constant, bit for bit the same in every such frame."""
import json
import os

import numpy as np

import chiron_amd as ca

import f16_ref

FLOOR = 1e-6
HEAD_FACTOR = 4.0          # stage C is fp32 against float64: the float32 fc_head is the yardstick, as in tests/train_cases.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JSON = os.path.join(ROOT, "profiles", "f16_ref_accuracy.json")
WEIGHT_SEED = 7
CUS = 256                  # compute units of an MI355X: launch_lstm takes lstm16w_kernel when 2 * (BP / 16) workgroups fill them

SWITCHES = ("CHIRON_NO_STREAM16", "CHIRON_NO_PWL", "CHIRON_LSTM16_NARROW", "CHIRON_LSTM16_FUSED_MIN", "CHIRON_LSTM16_PAIR",
            "CHIRON_LSTM16_UNFUSED", "CHIRON_F16_LASTH16", "CHIRON_W2_ZF16", "CHIRON_STATIC_TILES")

# form name -> (dtype, switches).  All are read at engine creation.
FORMS = {
    "default": ("fp16", {}),
    "no-stream16": ("fp16", {"CHIRON_NO_STREAM16": "1"}),                  # every convolution on the tiled GEMM (gemm.hip)
    "no-pwl": ("fp16", {"CHIRON_NO_PWL": "1"}),                            # block 1 lifted: launch_lift + GEMM conv2b
    "narrow": ("fp16", {"CHIRON_LSTM16_NARROW": "1"}),                     # lstm16_kernel, 4-row workgroups (= the default's kernel below WIDE_BATCH)
    "fused": ("fp16", {"CHIRON_LSTM16_FUSED_MIN": "1"}),                   # lstm16f_kernel: no z
    "fused-pair": ("fp16", {"CHIRON_LSTM16_FUSED_MIN": "1", "CHIRON_LSTM16_PAIR": "1"}),   # two 16-row groups per workgroup
    "wide-unfused": ("fp16", {"CHIRON_LSTM16_UNFUSED": "1"}),              # lstm16w_kernel reading z (needs max_batch that fills the CUs)
    "lasth16": ("fp16", {"CHIRON_F16_LASTH16": "1"}),                      # the last layer's output as halves
    "w2": ("fp16-w2", {}),
    "w2-zf16": ("fp16-w2", {"CHIRON_W2_ZF16": "1"}),
}

_CNN_FORMS = ("default", "no-stream16")
_RNN_FORMS = ("default", "narrow", "fused", "fused-pair", "wide-unfused", "lasth16")
_W2_FORMS = ("w2", "w2-zf16")
STREAM3_MIN_T = 32             # S_ROWS of stream16.hip: from here on conv2b streams (below, the tiled GEMM takes it in either form)
WIDE_BATCH = 16 * CUS // 2     # the smallest max_batch at which CHIRON_LSTM16_UNFUSED=1 selects lstm16w_kernel: 2 * (BP / 16) >= CUS

# (topology, L, B, max_batch, forms, end_to_end, the edge).  Engines of "fused-pair" and "wide-unfused" get their own max_batch
# (pair_batch / WIDE_BATCH): the rule of launch_lstm, pinned in tests/test_f16_ref_cpu.py.
CASES = [
    ("dna", 1, 101, 101, _CNN_FORMS, False, "T = 1: below the conv width, conv2b on the tiled GEMM, recurrence of one step (a row is ONE frame: "
     "about a hundred of them, as the smallest other case has, or a single rounding flip of the float32 yardstick is the whole of e_q)"),
    ("dna", 2, 21, 48, _CNN_FORMS, False, "T = 2: both taps of conv2b at a window border; 27 inert rows"),
    ("dna", 31, 5, 5, _CNN_FORMS, False, "one below stream16's 1 x 3 minimum: tiled conv2b, streaming 1 x 1; 155 rows: partial last tile"),
    ("dna", 32, 5, 5, _CNN_FORMS, False, "at the minimum: one window border in every 30-row tile; 160 rows = 5 whole 32-row tiles + partial 30-row tile"),
    ("dna", 33, 7, 7, _CNN_FORMS + ("no-pwl",), False, "one above the minimum; 231 rows: partial last tile of both tile sizes"),
    ("dna", 48, 37, 37, _CNN_FORMS + _RNN_FORMS[1:] + _W2_FORMS, True, "1776 rows; the first 16 rows all shorter than T / 4: a whole 16-row group finishes early"),
    ("dna", 100, 5, 16, _CNN_FORMS, False, "500 rows, window borders inside tiles of both sizes; 11 inert rows"),
    ("rna", 156, 5, 5, _CNN_FORMS + ("no-pwl",), False, "T = 32, L mod 5 = 1: left pad of the strided table conv"),
    ("rna", 157, 3, 3, _CNN_FORMS + ("no-pwl",), False, "L mod 5 = 2"),
    ("rna", 158, 7, 7, _CNN_FORMS + ("no-pwl",), False, "L mod 5 = 3"),
    ("rna", 159, 9, 9, _CNN_FORMS + ("no-pwl",), False, "L mod 5 = 4"),
    ("rna", 160, 4, 4, _CNN_FORMS + ("no-pwl",), False, "L mod 5 = 0"),
    ("rna", 500, 16, 16, _CNN_FORMS + ("no-pwl",), True, "RNA_default's own window, T = 100, one whole 16-row group"),
    ("rna", 500, 20, 20, ("default",) + _RNN_FORMS[1:] + _W2_FORMS, False, "the MultiRNN's per-direction projections in every recurrence form"),
    ("rna_model3", 694, 3, 4, _CNN_FORMS, True, "stem k 14 / stride 7, L mod 7 = 1"),
    ("rna_model3", 700, 3, 4, _CNN_FORMS, False, "stem, L mod 7 = 0"),
    ("rna_model2", 486, 3, 4, _CNN_FORMS, True, "stem k 9 / stride 5, T = 98"),
]


def case_id(c):
    return "%s-L%d-B%d-mb%d" % c[:4]


def specs():
    return {"dna": ca.dna_default_spec(), "rna": ca.rna_default_spec(),
            "rna_model2": ca.rna_head_spec("rna_model2"), "rna_model3": ca.rna_head_spec("rna_model3")}


def ragged(spec, L, B, seed, early_group=False):
    """B windows of L samples as tests/test_gpu_geometry._ragged builds them: seq_len T, 1 and 0 in the first rows, random lengths
    after, the signal zeroed past each window's samples.  early_group: rows 0 .. 15 all shorter than T / 4 (a whole 16-row group of
    the recurrence leaves its step loop early), the full-length row moved behind them."""
    T = spec.output_len(L)
    ratio = L / T
    x = ca.synthetic_signal(1, L * B, seed=seed)[0].reshape(B, L).copy()
    rng = np.random.RandomState(seed)
    ln = rng.randint(0, L + 1, size=B)
    head = [L, min(L, int(np.ceil(ratio))), 0][:B]
    ln[:len(head)] = head
    sl = np.minimum(ca.seq_len_for_engine(ln, ratio), T).astype(np.int32)
    sl[:len(head)] = [T, 1, 0][:B]
    if early_group:
        assert B > 17
        short = rng.randint(0, (T - 1) // 4 + 1, size=16)
        short[1:3] = (1, 0)
        sl[:16] = short
        ln[:16] = np.minimum(np.ceil(short * ratio).astype(np.int64), L)
        sl[16], ln[16] = T, L
    for b in range(B):
        x[b, ln[b]:] = 0
    return x, sl, T


def case_inputs(c):
    """-> (spec, weights, signal, seq_len, T) of one CASES row"""
    topology, L, B = c[:3]
    spec = specs()[topology]
    x, sl, T = ragged(spec, L, B, seed=4000 + L + 7 * B, early_group=(topology, L, B) == ("dna", 48, 37))
    return spec, ca.synthetic_weights(spec, seed=WEIGHT_SEED), x, sl, T


def launch_rules():
    """the numbers of the recurrence's launch rules, read out of the source so that a retuned one fails tests/test_f16_ref_cpu.py:
    rows the batch is padded to, rows per wide / fused workgroup, groups per paired workgroup, the fused form's default threshold"""
    import re
    csrc = os.path.join(ROOT, "chiron_amd", "csrc")
    eng, lstm = open(os.path.join(csrc, "engine.hip")).read(), open(os.path.join(csrc, "lstm.hip")).read()

    def one(pattern, text):
        found = re.findall(pattern, text)
        assert len(found) == 1, (pattern, found)
        return int(found[0])
    return {"pad": one(r"e->BP = roundup\(opts->max_batch, (\d+)\);", eng),
            "fused_min": one(r'atoi\(getenv\("CHIRON_LSTM16_FUSED_MIN"\)\) : (\d+);', eng),
            "fused_rows": one(r"\(e->BP / (\d+)\) \* 2 >= min_groups", eng),
            "wide_rows": one(r"\(p\.BP / (\d+)\) \* p\.ndir >= lstm_cu_count\(\)\) \? p\.BP / \1 : 0;", lstm),
            "pair_rows": one(r"const int g16 = p\.BP / (\d+);", lstm),
            "pair_groups": one(r"if \(g16 % (\d+) == 0 && p\.fused_pair\)", lstm)}


def pair_batch(max_batch):
    """lstm16f_kernel<*, 2> needs whole 32-row pairs of the padded batch"""
    return -(-max_batch // 32) * 32


def engine_batch(c, form):
    return WIDE_BATCH if form == "wide-unfused" else pair_batch(c[3]) if form == "fused-pair" else c[3]


def fused_layers(spec, form):
    """which layers lstm16f_kernel runs (engine.hip run_rnn: lstm16_fused and a projection over the whole input, in_w 256 or 200):
    every layer of the stacked topology, layer 0 only of the MultiRNN (its upper layers project each direction on its own)"""
    if form not in ("fused", "fused-pair"):
        return [False] * spec.rnn_layers
    return [True] * spec.rnn_layers if spec.to_dict()["rnn"]["kind"] == "stack" else [l == 0 for l in range(spec.rnn_layers)]


def arithmetic(spec, form):
    """-> the reference's arguments for a form: {"mode", "table", "z16" (per layer), "lasth16"}"""
    dtype, env = FORMS[form]
    fused = fused_layers(spec, form)
    if dtype == "fp16-w2":
        z16 = ["CHIRON_W2_ZF16" in env] * spec.rnn_layers
    else:
        z16 = [not f for f in fused]
    return {"mode": dtype, "table": "CHIRON_NO_PWL" not in env and not spec.stem, "z16": z16, "lasth16": "CHIRON_F16_LASTH16" in env}


def expected_profile(spec, form, prof):
    """the engine's own launch counts prove which form ran (one batch): block 1 as the table or lifted; the projection GEMMs of
    exactly the unfused layers"""
    dtype, env = FORMS[form]
    lifted = spec.blocks[0]["in"] == 1
    assert prof.get("conv1_pwl", 0) == (1 if lifted and "CHIRON_NO_PWL" not in env else 0), (form, prof)
    assert prof.get("conv_lift", 0) == (1 if (lifted and "CHIRON_NO_PWL" in env) or spec.stem else 0), (form, prof)
    fused = fused_layers(spec, form)
    nproj = [1 if (l == 0 or spec.to_dict()["rnn"]["kind"] == "stack") else 2 for l in range(spec.rnn_layers)]
    assert prof.get("lstm_proj0_dma", 0) == (0 if fused[0] else 1), (form, prof)
    assert prof.get("lstm_proj_dma", 0) == sum(n for l, (n, f) in enumerate(zip(nproj, fused)) if l > 0 and not f), (form, prof)
    assert prof.get("lstm_recurrence", 0) == spec.rnn_layers and prof.get("fc_head", 0) == 1, (form, prof)


# ---- metrics and the bar

def _rows(a, mask):
    a = np.asarray(a, dtype=np.float64)
    return a.reshape(-1, a.shape[-1]) if mask is None else a[mask]


def measures(got, ref, mask=None):
    """-> {"l2", "channel", "norm", "channels"}: the L2 norm of got - ref, the largest per-channel L2 norm of it, ||ref||, all over
    the DISTINCT (ref row, got row) pairs.  A window is zero past its samples, so hundreds of rows of a tensor repeat one
    computation on one input; a value within accumulation noise of a rounding tie then flips in all of them at once and one tie
    would weigh like hundreds (measured: one channel's error norm 0.51 against a median channel's 0.04, ensemble members 5 x
    apart for that alone).  Each distinct computation-and-result enters once; a defect that depends on the POSITION of a repeated
    row gives that row another result, so it stays in."""
    g, r = _rows(got, mask), _rows(ref, mask)
    if len(r):
        _, keep = np.unique(np.concatenate([r, g], axis=1), axis=0, return_index=True)
        g, r = g[np.sort(keep)], r[np.sort(keep)]
    d = g - r
    return {"l2": float(np.linalg.norm(d)), "channel": float(np.sqrt((d * d).sum(axis=0)).max()) if d.size else 0.0,
            "norm": float(np.linalg.norm(r)), "channels": int(r.shape[-1]), "rows": int(len(r))}


def judge(got, ref64, ref32, factor, mask=None):
    """-> per metric {"err", "e_q", "ratio", "ok"}; factor: {"l2": .., "channel": ..}"""
    g, q = measures(got, ref64, mask), measures(ref32, ref64, mask)
    out = {"norm": g["norm"]}
    for m in ("l2", "channel"):
        scale = g["norm"] if m == "l2" else g["norm"] / np.sqrt(g["channels"])
        out[m] = {"err": g[m], "e_q": q[m], "rel": g[m] / max(scale, 1e-300), "ratio": g[m] / q[m] if q[m] > 0 else (0.0 if g[m] == 0 else float("inf")),
                  "ok": bool(g[m] <= factor[m] * q[m] + FLOOR * scale)}
    return out


def valid_mask(sl, T):
    return np.arange(T)[None, :] < np.asarray(sl)[:, None]


def committed():
    with open(JSON) as f:
        return json.load(f)


def stage_refs(stage, spec, weights, arith, x, sl, fea=None, lasth=None, draw=None, acc=np.float64, mutate=None):
    """one stage of the restatement in `acc`: "cnn" from the signal, "rnn" from `fea`, "head" from `lasth`"""
    sd = spec.to_dict()
    if stage == "cnn":
        return f16_ref.cnn(x, sd, weights, acc, draw, arith["mode"], arith["table"], mutate=mutate)
    if stage == "rnn":
        return f16_ref.rnn(fea, sl, sd, weights, acc, draw, arith["mode"], arith["z16"], arith["lasth16"], mutate=mutate)
    return f16_ref.head(lasth, weights, acc)


# ---- the float32 ensemble (tools/f16_ref_accuracy.py) and the sensitivity of the bar (tests/test_f16_ref_cpu.py)

def arith_key(stage, a):
    if stage == "cnn":
        return "cnn %s %s" % (a["mode"], "table" if a["table"] else "lifted")
    if stage == "rnn":
        return "rnn %s z16=%s%s" % (a["mode"], "".join("1" if v else "0" for v in a["z16"]), " lasth16" if a["lasth16"] else "")
    return stage


def case_arithmetics(c):
    """-> {key: (stage, arithmetic)}: the distinct reference configurations a case's forms need, stage by stage, and the end-to-end row"""
    spec = specs()[c[0]]
    out = {}
    for form in c[4]:
        a = arithmetic(spec, form)
        for stage in ("cnn", "rnn"):
            out.setdefault(arith_key(stage, a), (stage, a))
    out["head"] = ("head", arithmetic(spec, "default"))
    if c[5]:
        out["e2e"] = ("e2e", arithmetic(spec, "default"))
    return out


def run_stage(stage, spec, weights, a, x, sl, fea, lasth, acc, draw_seed=None):
    """the stage in `acc`; draw_seed: channels of every product in a drawn order, the batch in another order"""
    if draw_seed is None:
        draw, order = None, np.arange(len(sl))
    else:
        draw = np.random.default_rng(draw_seed)
        order = draw.permutation(len(sl))
    inv = np.argsort(order)
    pick = lambda t: None if t is None else np.ascontiguousarray(t[order])
    if stage == "e2e":
        sd = spec.to_dict()
        out = f16_ref.compose(pick(x), sl[order], sd, weights, acc, draw, a["mode"], a["table"], a["z16"], a["lasth16"])[2]
    else:
        out = stage_refs(stage, spec, weights, a, pick(x), sl[order], pick(fea), pick(lasth), draw, acc)
    return out[inv]


def ensemble(c, draws=8):
    """-> {key: {"l2": spread, "channel": spread}} over the plain float32 run and `draws` drawn ones, against float64.  Stage B reads
    the float64 restatement's own features (default form), stage C its lasth: on the GPU they read the engine's."""
    spec, w, x, sl, T = case_inputs(c)
    mask = valid_mask(sl, T)
    base = arithmetic(spec, "default")
    fea = stage_refs("cnn", spec, w, base, x, sl)
    lasth = stage_refs("rnn", spec, w, base, x, sl, fea=fea)
    out = {}
    for key, (stage, a) in case_arithmetics(c).items():
        m = None if stage == "cnn" else mask
        ref = run_stage(stage, spec, w, a, x, sl, fea, lasth, np.float64)
        members = [measures(run_stage(stage, spec, w, a, x, sl, fea, lasth, np.float32, s), ref, m) for s in [None] + [100 + d for d in range(draws)]]
        out[key] = {"stage": stage}
        for metric in ("l2", "channel"):
            errs = [v[metric] for v in members]
            med = float(np.median(errs))
            out[key][metric] = {"norm": members[0]["norm"], "plain_err": errs[0], "median_err": med, "max_err": max(errs),
                                "max_over_median": max(errs) / med if med > 0 else 0.0}
    return out


def factors_from(rows):
    """{case: ensemble(case)} -> (largest max / median, FACTOR = max(4, 1.5 x it)) per stage and metric; the head's factor is fixed"""
    largest = {s: {"l2": 0.0, "channel": 0.0} for s in ("cnn", "rnn", "e2e")}
    for per_case in rows.values():
        for r in per_case.values():
            if r["stage"] in largest:
                for m in ("l2", "channel"):
                    largest[r["stage"]][m] = max(largest[r["stage"]][m], r[m]["max_over_median"])
    factor = {s: {m: max(4.0, 1.5 * v) for m, v in d.items()} for s, d in largest.items()}
    factor["head"] = {"l2": HEAD_FACTOR, "channel": HEAD_FACTOR}
    return largest, factor


REQUIRED = ("a", "a-last", "a-all", "b", "c", "d")
MUTATIONS = {
    "a": ("cnn", "one output channel of one conv site loses its shift: block 1's last accumulator (conv2c's and branch1's, folded into one)"),
    "a-mid": ("cnn", "the same at conv2b of the middle block"),
    "a-last": ("cnn", "the same at the last block's output"),
    "a-all": ("cnn", "every channel of the middle block's conv2b loses its shift"),
    "b": ("cnn", "conv2b's first tap reads the previous window's last frame instead of the padding zero"),
    "c": ("rnn", "one column of W_hh takes its neighbour's values"),
    "d": ("rnn", "the backward direction starts at frame T - 1 instead of seq_len - 1 on ragged rows"),
    "e": ("rnn", "z rounded to halves where the form does not round it (and not rounded where it does)"),
    "f": ("cnn", "one stored activation site left wide"),
    "g": ("rnn", "the last layer's output rounded to halves"),
}


def mutation(name, spec, weights, features=None):
    """the `mutate` argument of f16_ref for one row of the table"""
    blocks = spec.to_dict()["cnn"]
    if name in ("a", "a-mid", "a-last", "a-all"):
        # the channel whose shift is the MEDIAN of its site's positive ones: not the most visible one, and not one that ReLU keeps at
        # 0 with or without its shift (a channel with a negative shift is often dead: losing it changes no output at all).
        # "a": the first block's last accumulator, where the f16 engines fold conv2c's and branch1's shifts into one;
        # "a-mid": conv2b of the middle block; "a-last": the accumulator the features leave
        # "a-all": every channel of the middle block's conv2b (a shift applied twice, or not at all, is a defect of the whole site)
        blk, conv = {"a": (blocks[0], "conv2c"), "a-mid": (blocks[len(blocks) // 2], "conv2b"), "a-last": (blocks[-1], "conv2c"),
                     "a-all": (blocks[len(blocks) // 2], "conv2b")}[name]
        site = blk["name"] + "/branch2/" + conv
        sh = f16_ref.fold_bn(weights, site, True)[1]
        if conv == "conv2c":
            sh = sh + f16_ref.fold_bn(weights, blk["name"] + "/branch1/conv1", blk["i_bn"])[1]
        if name == "a-all":
            return {"no_shift": (site, slice(None))}
        pos = np.flatnonzero(sh > 0)
        if name == "a-last" and features is not None:      # ... and, where it can be told, one that is alive in a quarter of the frames
            alive = (np.asarray(features) > 0).reshape(-1, len(sh)).mean(axis=0) >= 0.25
            pos = np.flatnonzero((sh > 0) & alive)
        return {"no_shift": (site, int(pos[np.argsort(sh[pos])[len(pos) // 2]]))}
    return {"b": {"tap_leak": True}, "c": {"whh_column": (1, 0, 17)}, "d": {"bw_from_end": True}, "e": {"flip_z16": True},
            "f": {"wide_site": 3}, "g": {"lasth_half": True}}[name]


def applies(name, c, sl, T):
    if name == "b":
        return c[2] >= 2
    if name == "c":
        return bool((sl >= 2).any())                  # the first step multiplies W_hh by h = 0
    if name == "d":
        return bool(((sl > 0) & (sl < T)).any())      # no ragged row exists at T = 1
    return True


def sensitivity(c, factor, names):
    """the float64 restatement with one defect against the unmutated one, under the bar: {name: {"rejected", "l2", "channel"}}"""
    spec, w, x, sl, T = case_inputs(c)
    a = arithmetic(spec, "default")
    mask = valid_mask(sl, T)
    fea = stage_refs("cnn", spec, w, a, x, sl)
    ref = {"cnn": fea, "rnn": stage_refs("rnn", spec, w, a, x, sl, fea=fea)}
    r32 = {"cnn": stage_refs("cnn", spec, w, a, x, sl, acc=np.float32), "rnn": stage_refs("rnn", spec, w, a, x, sl, fea=fea, acc=np.float32)}
    out = {}
    for name in names:
        stage = MUTATIONS[name][0]
        if not applies(name, c, sl, T):
            continue
        got = stage_refs(stage, spec, w, a, x, sl, fea=fea, mutate=mutation(name, spec, w, fea))
        j = judge(got, ref[stage], r32[stage], factor[stage], None if stage == "cnn" else mask)
        out[name] = {"rejected": not (j["l2"]["ok"] and j["channel"]["ok"]), "l2_over_e_q": j["l2"]["ratio"], "channel_over_e_q": j["channel"]["ratio"]}
    return out
