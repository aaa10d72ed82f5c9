"""The GPU side of the f16-engine reference tests: run one case in one form, judge its three stages against tests/f16_ref.py.
Shared by tests/test_gpu_f16_ref.py (asserts) and tools/f16_ref_accuracy.py --hip (records the ratios)."""
import functools
import os

import numpy as np

import chiron_amd as ca

import f16_cases as fc
import f16_ref


def _environ_set(k, v):
    os.environ[k] = v


def _environ_del(k, raising=False):
    os.environ.pop(k, None)


def run_form(c, form, setenv=_environ_set, delenv=_environ_del):
    """one engine of the form, one batch -> {"features", "lasth", "logits", "profile", "T"}.  The switches are read at engine
    creation: set around ca.Engine(...) and cleared afterwards."""
    spec, w, x, sl, T = fc.case_inputs(c)
    dtype, env = fc.FORMS[form]
    for v in fc.SWITCHES:
        delenv(v, raising=False)
    for k, v in env.items():
        setenv(k, v)
    try:
        eng = ca.Engine(spec, w, max_batch=fc.engine_batch(c, form), segment_len=c[1], dtype=dtype)
    finally:
        for k in env:
            delenv(k, raising=False)
    try:
        assert eng.T == T
        eng.profile(True)
        res = eng.infer(x, sl, want_prob=False, want_logits=True)
        prof = {k: v["launches"] for k, v in eng.profile_read().items()}
        return {"features": eng.features().copy(), "lasth": eng.rnn_output().copy(), "logits": res.logits.copy(), "profile": prof, "T": T}
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def _cnn_refs(case_index, key):
    """the CNN stage's float64 and float32 restatements: the same for every form of one arithmetic"""
    c = fc.CASES[case_index]
    spec, w, x, sl, T = fc.case_inputs(c)
    stage, a = fc.case_arithmetics(c)[key]
    return tuple(fc.stage_refs("cnn", spec, w, a, x, sl, acc=acc) for acc in (np.float64, np.float32))


@functools.lru_cache(maxsize=None)
def _e2e_refs(case_index):
    c = fc.CASES[case_index]
    spec, w, x, sl, T = fc.case_inputs(c)
    a = fc.arithmetic(spec, "default")
    return tuple(f16_ref.compose(x, sl, spec.to_dict(), w, acc, None, a["mode"], a["table"], a["z16"], a["lasth16"])[2] for acc in (np.float64, np.float32))


def judge_form(c, form, out, factor):
    """-> ({stage: judge rows}, [failed exact checks]).  Stage A: features against cnn(signal); B: lasth against rnn(the engine's
    own features); C: logits against head(the engine's own lasth); end to end (cases that ask for it, default form): logits
    against the three reference stages composed from the signal."""
    spec, w, x, sl, T = fc.case_inputs(c)
    a = fc.arithmetic(spec, form)
    mask = fc.valid_mask(sl, T)
    i = fc.CASES.index(c)
    rows, exact = {}, []
    r64, r32 = _cnn_refs(i, fc.arith_key("cnn", a))
    rows["cnn"] = fc.judge(out["features"], r64, r32, factor["cnn"])
    fea = out["features"]
    rows["rnn"] = fc.judge(out["lasth"], fc.stage_refs("rnn", spec, w, a, x, sl, fea=fea), fc.stage_refs("rnn", spec, w, a, x, sl, fea=fea, acc=np.float32),
                           factor["rnn"], mask)
    rows["head"] = fc.judge(out["logits"], f16_ref.head(out["lasth"], w), f16_ref.head(out["lasth"], w, np.float32), factor["head"], mask)
    if c[5] and form == "default":
        e64, e32 = _e2e_refs(i)
        rows["e2e"] = fc.judge(out["logits"], e64, e32, factor["e2e"], mask)
    # exactly: nothing but finite numbers; halves where the form stores halves; at and past seq_len lasth is 0 and the logits are
    # one constant, the head of a zero frame
    if not all(np.isfinite(out[k]).all() for k in ("features", "lasth", "logits")):
        exact.append("not finite")
    if not np.array_equal(out["features"], f16_ref.f16(out["features"])):
        exact.append("features are not halves")
    if a["lasth16"] and not np.array_equal(out["lasth"], f16_ref.f16(out["lasth"])):
        exact.append("lasth is not halves under CHIRON_F16_LASTH16")
    if not a["lasth16"] and np.array_equal(out["lasth"], f16_ref.f16(out["lasth"])) and mask.sum() * out["lasth"].shape[-1] >= 1000:
        exact.append("lasth holds nothing but halves: the last layer was not written as fp32")
    if (~mask).any():
        if np.any(out["lasth"][~mask] != 0):
            exact.append("lasth is not 0 past seq_len")
        tail = out["logits"][~mask]
        if not np.array_equal(tail.view(np.uint32), np.broadcast_to(tail[0], tail.shape).view(np.uint32)):
            exact.append("the logits past seq_len are not one constant")
        k64, k32 = f16_ref.head_constant(w, spec.hidden), f16_ref.head_constant(w, spec.hidden, np.float32)
        err, e32, norm = (float(np.linalg.norm(v)) for v in (tail[0] - k64, k32 - k64, k64))
        if not err <= fc.HEAD_FACTOR * e32 + fc.FLOOR * norm:
            exact.append("the head's constant: err %.3g against e32 %.3g, norm %.3g" % (err, e32, norm))
    return rows, exact


def measure_all(factor):
    """every case in every form -> (largest err / e_q, {case: {form: {stage: {metric: ..}}}})"""
    worst, table = 0.0, {}
    for c in fc.CASES:
        for form in c[4]:
            out = run_form(c, form)
            fc.expected_profile(fc.specs()[c[0]], form, out["profile"])
            rows, exact = judge_form(c, form, out, factor)
            rec = {st: {m: {"err_over_e_q": r[m]["ratio"], "err_rel": r[m]["rel"], "ok": r[m]["ok"]} for m in ("l2", "channel")} for st, r in rows.items()}
            rec["exact_checks_failed"] = exact
            table.setdefault(fc.case_id(c), {})[form] = rec
            top = max(r[m]["ratio"] for r in rows.values() for m in ("l2", "channel") if np.isfinite(r[m]["ratio"]))
            worst = max(worst, top)
            print(fc.case_id(c), form, {st: "%.3g / %.3g" % (r["l2"]["ratio"], r["channel"]["ratio"]) for st, r in rows.items()}, exact, flush=True)
    return worst, table
