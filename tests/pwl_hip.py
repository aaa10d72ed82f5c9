"""The GPU side of block 1's table tests: the cases, one engine run per (case, form), and its judgement against tests/pwl_ref.py.
Shared by tests/test_gpu_pwl.py (asserts) and tools/pwl_table_accuracy.py --hip (records the ratios)."""
import functools
import os

import numpy as np

import chiron_amd as ca

import fp32_ref
import pwl_ref as pr

SWITCHES = ("CHIRON_NO_PWL",)
# form -> (dtype, switches, the bucket of the engine's profile that proves it, the reference's arithmetic)
FORMS = {
    "fp32": ("fp32", {}, "conv1_pwl"),                             # pwl_conv_kernel<0>
    "fp32-lifted": ("fp32", {"CHIRON_NO_PWL": "1"}, "conv_lift"),  # conv2a stored, conv2b on the GEMM: the same inputs, the same bar
    "fp16": ("fp16", {}, "conv1_pwl"),                             # pwl_conv_kernel<1>
    "fp32-split": ("fp32-split", {}, "conv1_pwl"),                 # pwl_conv_kernel<2>
}
HALF_FORMS = ("fp16", "fp32-split")                                # their values pass through halves: the capped sample set
ALL = tuple(FORMS)
WIDE = ("fp32", "fp32-lifted")                                     # planted(): a constant channel of 1e9, far above a half's 65504

# (weight set, L, B or None: as many windows as hold every sample once, forms, the edge)
CASES = [
    ("synthetic-dna", 1, 3, ALL, "T = 1: every tap but the middle one in the padding"),
    ("synthetic-dna", 31, 3, ALL, "one position short of the 32-position tile"),
    ("synthetic-dna", 32, 3, ALL, "one whole tile per window: block index = window"),
    ("synthetic-dna", 33, 3, ALL, "a second tile of one position"),
    ("synthetic-dna", 65, 3, ALL, "three tiles per window, the last of one position"),
    ("synthetic-dna", 130, None, ALL, "every sample of the set: all 257 rows"),
    ("zero-centred", 130, None, ALL, "breakpoints on both sides of 0: reference points at the upper bound, at 0, at the lower bound"),
    ("planted", 130, None, WIDE, "a == 0 of either sign of b, a negative scale, breakpoints at +-inf and at -7e29"),
    ("equal-breakpoints", 130, None, ALL, "two pairs of equal breakpoints: rows no sample can select"),
    ("no-breakpoints", 130, 4, ALL, "nbp == 0: one row"),
    ("synthetic-rna", 156, 3, ALL, "k 13 / stride 5, L mod 5 = 1: left pad 4"),
    ("synthetic-rna", 157, 3, ALL, "L mod 5 = 2"),
    ("synthetic-rna", 158, 3, ALL, "L mod 5 = 3"),
    ("synthetic-rna", 159, 3, ALL, "L mod 5 = 4"),
    ("synthetic-rna", 160, 3, ALL, "L mod 5 = 0"),
    ("synthetic-rna", 160, None, ALL, "every sample of the set through the strided table"),
]
RUNS = [(c, form) for c in CASES for form in c[3]]


def case_id(c):
    return "%s-L%d-B%s" % (c[0], c[1], "all" if c[2] is None else c[2])


@functools.lru_cache(maxsize=None)
def case_inputs(c, capped):
    """-> (spec, weights, x [B, L], seq_len, samples, how many of them the windows hold); shared: read only"""
    name, L, B = c[:3]
    spec, w = pr.weight_set(name)
    d = pr.set_dump(name, L)
    s = pr.samples_capped(d, w, spec)[0] if capped else pr.samples_for(d)
    seed = 3000 + L
    if B is None:
        B = 4
        while pr.windows(s, spec, L, B, seed)[2] < len(s):
            B += 2
    x, ln, placed = pr.windows(s, spec, L, B, seed)
    T = spec.output_len(L)
    sl = np.minimum(ca.seq_len_for_engine(ln, L / T), T).astype(np.int32)
    return spec, w, x, sl, s, placed


def _environ_set(k, v):
    os.environ[k] = v


def _environ_del(k, raising=False):
    os.environ.pop(k, None)


def engine_of(c, form, batch, setenv=_environ_set, delenv=_environ_del):
    """the one-block engine of a case in a form; the switch is read at creation: set around it, cleared afterwards"""
    spec, w = pr.weight_set(c[0])
    dtype, env, _ = FORMS[form]
    for v in SWITCHES:
        delenv(v, raising=False)
    for k, v in env.items():
        setenv(k, v)
    try:
        return ca.Engine(spec, w, max_batch=batch, segment_len=c[1], dtype=dtype)
    finally:
        for k in env:
            delenv(k, raising=False)


WRONG_CHANNEL, WRONG_BY = 17, 1e-3


def one_channel_wrong(w):
    """the weights with ONE conv2a channel's BN offset off by 1e-3 (its breakpoint by a third of the mean gap to the next one; conv2b's
    output by up to 3e-4 of its norm where the channel is active): a table both judgements must reject (tests/test_pwl_cpu.py)"""
    w = type(w)((k, v.copy()) for k, v in w.items())
    w[pr.BLOCK + "/branch2/conv2a_bn/offset"][WRONG_CHANNEL] += np.float32(WRONG_BY)
    return w


def run_form(c, form, setenv=_environ_set, delenv=_environ_del):
    """-> {"features": block 1's output [B, T, C] of the whole batch, "again": of the same batch run a second time, "alone": of the
    last whole window run as a batch of one, "alone_index", "profile": launches per bucket of the first run}"""
    spec, w, x, sl, s, placed = case_inputs(c, form in HALF_FORMS)
    eng = engine_of(c, form, x.shape[0], setenv, delenv)
    try:
        eng.profile(True)
        eng.infer(x, sl, want_prob=False)
        out = {"profile": {k: v["launches"] for k, v in eng.profile_read().items()}, "features": eng.features().copy()}
        eng.profile(False)
        eng.infer(x, sl, want_prob=False)
        out["again"] = eng.features().copy()
        b = x.shape[0] - 1 if x.shape[0] >= 4 else 0                # pwl_ref.windows: whole windows
        eng.infer(x[b:b + 1], sl[b:b + 1], want_prob=False)
        out["alone"], out["alone_index"] = eng.features().copy(), b
    finally:
        eng.close()
    return out


@functools.lru_cache(maxsize=None)
def _refs(c, capped):
    """the float64 restatement of the one-block network and its float32 realisation: fp32_ref.cnn, the same for every wide form"""
    spec, w, x = case_inputs(c, capped)[:3]
    sd = spec.to_dict()
    return fp32_ref.cnn(x, sd, w), fp32_ref.cnn(x, sd, w, np.float32)


def judge_form(c, form, out, factor):
    """-> ({"ratio": the largest err / e32, "bad": positions (fp16: elements) over the bar, "n", ...}, [failed exact checks])"""
    spec, w, x, sl, s, placed = case_inputs(c, form in HALF_FORMS)
    fea = out["features"]
    exact = []
    if not np.isfinite(fea).all():
        exact.append("not finite")
    if not np.array_equal(fea.view(np.uint32), out["again"].view(np.uint32)):
        exact.append("two runs of one batch differ")
    b = out["alone_index"]
    if not np.array_equal(fea[b].view(np.uint32), out["alone"][0].view(np.uint32)):
        exact.append("window %d differs alone and in the batch" % b)
    if form == "fp16":
        h = pr.half_check(fea, x, w, spec, factor["features"])
        row = {"ratio": h["ratio"], "bad": int((~h["ok"]).sum()), "n": h["elements"], "unit": "elements", "ambiguous_positions": h["ambiguous"],
               "ambiguous_share_of_live_elements": h["ambiguous_share_of_live_elements"]}
    else:
        r64, r32 = _refs(c, form in HALF_FORMS)
        j = pr.per_position(fea, r64, r32, factor["features"])
        with np.errstate(divide="ignore", invalid="ignore"):
            raw = np.where(j["e32"] > 0, j["err"] / j["e32"], 0.0)
        row = {"ratio": j["ratio"], "bad": int((~j["ok"]).sum()), "n": int(j["ok"].size), "unit": "positions",
               "largest_err_over_scale": float(np.max(j["err"] / np.maximum(j["scale"], 1e-300))),
               "largest_err_over_e32_below_the_floor_too": float(raw.max()), "worst_position": j["worst"]}
    row["samples"], row["samples_placed"], row["windows"] = int(len(s)), int(placed), int(x.shape[0])
    return row, exact


def measure_all(factor):
    """every case in every form -> (largest ratio per form, {case: {form: row}})"""
    worst, table = {}, {}
    for c, form in RUNS:
        out = run_form(c, form)
        assert out["profile"].get(FORMS[form][2], 0) == 1, (case_id(c), form, out["profile"])
        row, exact = judge_form(c, form, out, factor)
        row["exact_checks_failed"] = exact
        table.setdefault(case_id(c), {})[form] = row
        worst[form] = max(worst.get(form, 0.0), row["ratio"])
        print(case_id(c), form, row, flush=True)
    return worst, table
