"""The GPU side of the fp32 engine's stage tests: run one case in one form, judge every stage against tests/fp32_ref.py.
Shared by tests/test_gpu_fp32_ref.py (asserts) and tools/fp32_stage_accuracy.py --hip (records the ratios)."""
import functools
import os

import numpy as np

import chiron_amd as ca

import fp32_cases as pc
import fp32_ref


def _environ_set(k, v):
    os.environ[k] = v


def _environ_del(k, raising=False):
    os.environ.pop(k, None)


def run_form(c, form, setenv=_environ_set, delenv=_environ_del, weights=None):
    """engines of 1 .. n rnn_layers in the form, one batch each -> {"features", "layers" (each layer's output: the output of the engine
    that ends in it), "logits", "profiles" (per engine), "T"}.  The switches are read at engine creation: set around ca.Engine(...)
    and cleared afterwards.  weights: other weights than the case's (the test that feeds the engine a deliberately coarse operand)."""
    spec, w, x, sl, T = pc.case_inputs(c)
    w = w if weights is None else weights
    env = pc.form_env(c, form)
    out = {"layers": [], "profiles": [], "features_all": [], "T": T}
    for n in range(1, spec.rnn_layers + 1):
        for v in pc.SWITCHES:
            delenv(v, raising=False)
        for k, v in env.items():
            setenv(k, v)
        try:
            eng = ca.Engine(pc.spec_with_layers(spec, n), w, max_batch=c[2], segment_len=c[1])
        finally:
            for k in env:
                delenv(k, raising=False)
        try:
            assert eng.T == T
            eng.profile(True)
            res = eng.infer(x, sl, want_prob=False, want_logits=True)
            out["profiles"].append({k: v["launches"] for k, v in eng.profile_read().items()})
            out["layers"].append(eng.rnn_output().copy())
            out["features_all"].append(eng.features().copy())
            out["logits"] = res.logits.copy()          # the last engine's: the whole network
        finally:
            eng.close()
    out["features"] = out["features_all"][-1]
    return out


@functools.lru_cache(maxsize=None)
def _cnn_refs(case_index):
    """the CNN stage's float64 and float32 restatements: the same for every form of a case"""
    c = pc.CASES[case_index]
    spec, w, x, sl, T = pc.case_inputs(c)
    return tuple(pc.run_stage("cnn", spec, w, c, x, sl, None, acc) for acc in (np.float64, np.float32))


def judge_form(c, form, out, factor, gates=None):
    """-> ({stage: judge rows}, [failed exact checks]).  cnn: features against cnn(signal); rnn<l>: the l-layer engine's output
    against layer l applied to the engine's own previous output (the features, or the (l - 1)-layer engine's output); head: logits
    against head(the engine's own lasth)."""
    spec, w, x, sl, T = pc.case_inputs(c)
    mask = pc.valid_mask(sl, T)
    rows, exact = {}, []
    r64, r32 = _cnn_refs(pc.CASES.index(c))
    rows["cnn"] = pc.judge(out["features"], r64, r32, factor["cnn"])
    prev = out["features"]
    for l, got in enumerate(out["layers"]):
        stage = "rnn%d" % (l + 1)
        rows[stage] = pc.judge(got, pc.run_stage(stage, spec, w, c, x, sl, prev, gates=gates), pc.run_stage(stage, spec, w, c, x, sl, prev, np.float32, gates=gates),
                               factor["rnn"], mask)
        prev = got
    rows["head"] = pc.judge(out["logits"], fp32_ref.head(prev, w), fp32_ref.head(prev, w, np.float32), factor["head"], mask)
    # exactly: nothing but finite numbers; every engine of the run computed the same features; at and past seq_len lasth is 0 and the
    # logits are one constant, the head of a zero frame
    if not all(np.isfinite(v).all() for v in [out["features"], out["logits"]] + out["layers"]):
        exact.append("not finite")
    if not all(np.array_equal(f.view(np.uint32), out["features"].view(np.uint32)) for f in out["features_all"]):
        exact.append("engines of one form disagree on the features")
    if (~mask).any():
        if any(np.any(h[~mask] != 0) for h in out["layers"]):
            exact.append("a layer's output is not 0 past seq_len")
        tail = out["logits"][~mask]
        if not np.array_equal(tail.view(np.uint32), np.broadcast_to(tail[0], tail.shape).view(np.uint32)):
            exact.append("the logits past seq_len are not one constant")
        k64, k32 = fp32_ref.head_constant(w, spec.hidden), fp32_ref.head_constant(w, spec.hidden, np.float32)
        err, e32, norm = (float(np.linalg.norm(v)) for v in (tail[0] - k64, k32 - k64, k64))
        if not err <= pc.HEAD_FACTOR * e32 + pc.FLOOR * norm:
            exact.append("the head's constant: err %.3g against e32 %.3g, norm %.3g" % (err, e32, norm))
    return rows, exact


def report(rows, exact):
    """what a run leaves on file: every ratio err / e32, per stage and metric"""
    rec = {st: {m: {"err_over_e32": r[m]["ratio"], "err": r[m]["err"], "e32": r[m]["e_q"], "err_rel": r[m]["rel"], "ok": r[m]["ok"]} for m in ("l2", "channel")}
           for st, r in rows.items()}
    rec["exact_checks_failed"] = list(exact)
    return rec


def measure_all(factor, gates=None):
    """every case in every form -> (largest err / e32 per stage kind and metric, {case: {form: report}})"""
    worst, table = {}, {}
    for c, form in pc.RUNS:
        out = run_form(c, form)
        spec = pc.specs()[c[0]]
        for n, prof in enumerate(out["profiles"]):
            pc.expected_profile(spec, c, n + 1, prof)
        rows, exact = judge_form(c, form, out, factor, gates)
        table.setdefault(pc.case_id(c), {})[form] = report(rows, exact)
        for st, r in rows.items():
            for m in ("l2", "channel"):
                if np.isfinite(r[m]["ratio"]):
                    key = "%s %s" % (pc.kind(st), m)
                    worst[key] = max(worst.get(key, 0.0), r[m]["ratio"])
        print(pc.case_id(c), form, {st: "%.3g / %.3g%s" % (r["l2"]["ratio"], r["channel"]["ratio"], "" if r["l2"]["ok"] and r["channel"]["ok"] else " FAIL")
                                    for st, r in rows.items()}, exact, flush=True)
    return worst, table
