"""How far apart are float32 realisations of the CNN's forward and of its gradients?  Sets the factors of tests/test_gpu_cnn_train.py.

Default mode, CPU only, the HIP result never enters: for every gradient case of tests/cnn_train_cases.py, float64 autograd of
tests/cnn_ref.py gives the exact values; then the plain float32 run of the same restatement and DRAWS more float32 realisations of
it (every convolution's channels in a permuted order, the batch in another order).  Per tensor: every member's error against
float64, the median member's, and the largest member's ratio to that median.
  forward    features and every site's moments, the network as it is;
  gradients  under FIXED ReLU masks (the signs of the float64 pre-activations), as the GPU test compares them: with free masks a ReLU
             whose pre-activation is within rounding of 0 flips between realisations and moves the gradient by a discrete amount
             (max / median up to 3e4 was measured that way), which no bar of a few rounding errors can absorb.
factor = max(4, 1.5 x the largest ratio), for the forward and for the gradients separately.
The same ensemble over CAP_GRAD_CASES (the shapes past the caps of the row reductions) gives "factor_cap" by the same rule, kept
apart so that the factor of the cases above stays what it was derived from; its rows are under "cap".  GEOMETRY_GRAD_CASES (every
'SAME' left pad of the strided sites, windows of 1 to 3 frames) give "factor_geometry" in the same way; under "geometry" each of the
21 cases keeps one row for the forward and one for the gradients: the tensor with the largest ratio.

--hip (needs a GPU): the HIP path's err / e32 on the same cases, merged into the same file under "hip"; the default mode keeps an
existing "hip" block.  The cap cases' rows go under "hip" / "cap_cases", the geometry cases' under "hip" / "geometry_cases" (one
row per case: the tensor with the largest err / e32 above the floor, and whether every tensor met its bar).

--cases grad | cap | geometry: only that list of cases; what the file holds for the others is kept.

    python tools/cnn_grad_accuracy.py [--draws 8] [--cases all|grad|cap|geometry] [--hip] [--out profiles/cnn_grad_accuracy.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cnn_ref                     # noqa: E402
import cnn_train_cases as cc       # noqa: E402


def spread(errs, norm):
    med = float(np.median(errs))
    return {"norm": norm, "plain_err": errs[0], "median_err": med, "max_err": max(errs), "max_over_median": max(errs) / med if med > 0 else 0.0}


def widest(rows):
    """One row for a case: the tensor with the largest max / median, with its figures."""
    name = max(rows, key=lambda k: rows[k]["max_over_median"])
    return dict(rows[name], tensor=name, tensors=len(rows))


def ensemble(draws, case_list, per_case=False):
    """-> (largest max / median of the forward and of the gradients, factors by the rule, rows per case).  per_case: one row per
    case and part (the tensor with the largest ratio) instead of one per tensor."""
    cases, largest = {}, {"forward": 0.0, "gradients": 0.0}
    for kind, B, L in case_list:
        spec, w, x, g = cc.grad_case(kind, B, L)
        pre = {}
        f64, g64 = cnn_ref.gradients(x, spec, w, g, torch.float64, pre=pre)
        masks = {k: v > 0 for k, v in pre.items()}
        _, m64 = cnn_ref.forward(x, spec, w, torch.float64)
        seeds = [None] + [100 + d for d in range(draws)]
        fwd = [cnn_ref.forward(x, spec, w, torch.float32, draw=s) for s in seeds]
        grd = [cnn_ref.gradients(x, spec, w, g, torch.float32, draw=s, masks=masks)[1] for s in seeds]
        forward = {"features": spread([float(np.linalg.norm(m[0] - f64)) for m in fwd], float(np.linalg.norm(f64)))}
        for site in m64:
            for i, leaf in enumerate(("mean", "var")):
                forward["%s %s" % (site, leaf)] = spread([float(np.linalg.norm(m[1][site][i] - m64[site][i])) for m in fwd],
                                                         float(np.linalg.norm(m64[site][i])))
        gradients = {name: spread([float(np.linalg.norm(m[name] - g64[name])) for m in grd], float(np.linalg.norm(g64[name]))) for name in g64}
        label = "%s B%d L%d" % (kind, B, L)
        cases[label] = {"forward": widest(forward), "gradients": widest(gradients)} if per_case else {"forward": forward, "gradients": gradients}
        for part, rows in (("forward", forward), ("gradients", gradients)):
            largest[part] = max(largest[part], max(r["max_over_median"] for r in rows.values()))
        print(label, "largest max/median: forward %.3g, gradients %.3g" % (max(r["max_over_median"] for r in forward.values()),
                                                                          max(r["max_over_median"] for r in gradients.values())), flush=True)
    return largest, {k: max(4.0, 1.5 * v) for k, v in largest.items()}, cases


def method(draws):
    return {"method": "float32 realisations of tests/cnn_ref.py (plain + %d draws: channel orders of every product, batch order) against "
                      "float64; gradients under fixed ReLU masks (signs of the float64 pre-activations); per tensor the largest member "
                      "error over the median member's" % draws,
            "draws": draws}


def hip(factor, case_list, per_case=False):
    """-> (largest err / e32 above the floor, rows per case).  per_case: one row per case (the tensor with the largest err / e32
    above the floor, and whether every tensor met its bar) instead of one per tensor."""
    out, worst = {}, 0.0
    for kind, B, L in case_list:
        spec, w, x, g = cc.grad_case(kind, B, L)
        fea, mom, dp, gu, masks = cc.hip_run(spec, w, x, g)
        label = "%s B%d L%d" % (kind, B, L)
        rows = dict(cc.forward_rows(spec, w, x, fea, mom, factor["forward"]))
        rows.update(cc.gradient_rows(spec, w, x, dp, gu, masks, factor["gradients"], label))
        out[label] = {k: {"err_over_e32": r["ratio"], "err_rel": r["err_rel"], "e32_rel": r["e32_rel"], "ok": r["ok"]} for k, r in rows.items()}
        if per_case:
            above = {k: v for k, v in out[label].items() if v["err_rel"] > cc.FLOOR} or out[label]
            name = max(above, key=lambda k: above[k]["err_over_e32"])
            out[label] = dict(above[name], tensor=name, tensors=len(rows), ok=all(v["ok"] for v in out[label].values()))
        worst = max(worst, max((r["ratio"] for r in rows.values() if r["err_rel"] > cc.FLOOR), default=0.0))
        print(label, "largest err/e32 %.3g" % max(r["ratio"] for r in rows.values()), flush=True)
    return worst, out


HIP_NOTE = ("chiron_cnn_train_forward / _backward against the same float64 values, error over the plain float32 run's (e32); gradients "
            "under the HIP run's own ReLU masks; measured after the factors were fixed")


def dump(out):
    """indent=1 as ever, except that a case of the one-row-per-case lists takes one line."""
    lines, flat = {}, json.loads(json.dumps(out))
    for rows in (flat.get("geometry", {}).get("cases"), flat.get("hip", {}).get("geometry_cases")):
        for label in rows or ():
            key = "@@%d@@" % len(lines)
            lines[key] = json.dumps(rows[label])
            rows[label] = key
    text = json.dumps(flat, indent=1)
    for key, line in lines.items():
        text = text.replace('"%s"' % key, line)
    return text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=8)
    ap.add_argument("--hip", action="store_true")
    ap.add_argument("--cases", choices=["all", "grad", "cap", "geometry"], default="all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cnn_grad_accuracy.json"))
    a = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    old = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out = old
    # the lists past the first: (name under --cases, its cases, key of its factors, key of its ensemble rows, prefix under "hip",
    # one row per case instead of one per tensor)
    extra = [("cap", cc.CAP_GRAD_CASES, "factor_cap", "cap", "cap_", False),
             ("geometry", cc.GEOMETRY_GRAD_CASES, "factor_geometry", "geometry", "geometry_", True)]
    chosen = [e for e in extra if a.cases in ("all", e[0])]
    if a.hip:
        if (a.cases in ("all", "grad") and not isinstance(old.get("factor"), dict)) or any(not isinstance(old.get(e[2]), dict) for e in chosen):
            raise SystemExit("run the CPU ensemble first: --hip reads its factors from %s" % a.out)
        h = out.setdefault("hip", {})
        h["note"] = HIP_NOTE
        if a.cases in ("all", "grad"):
            h["largest_err_over_e32_above_the_floor"], h["cases"] = hip(old["factor"], cc.GRAD_CASES)
        for _, case_list, factor_key, _, prefix, per_case in chosen:
            h[prefix + "largest_err_over_e32_above_the_floor"], h[prefix + "cases"] = hip(old[factor_key], case_list, per_case)
    else:
        if a.cases in ("all", "grad"):
            out = dict(method(a.draws))
            out["largest_max_over_median"], out["factor"], out["cases"] = ensemble(a.draws, cc.GRAD_CASES)
            out.update({k: old[k] for k in ("factor_cap", "cap", "factor_geometry", "geometry", "hip") if k in old})
            print("largest ratios %s -> factors %s" % (out["largest_max_over_median"], out["factor"]))
        for name, case_list, factor_key, rows_key, _, per_case in chosen:
            largest, out[factor_key], rows = ensemble(a.draws, case_list, per_case)
            out[rows_key] = {"draws": a.draws, "largest_max_over_median": largest, "cases": rows}
            print("%s cases: largest ratios %s -> %s %s" % (name, largest, factor_key, out[factor_key]))
    with open(a.out, "w") as f:
        f.write(dump(out))


if __name__ == "__main__":
    main()
