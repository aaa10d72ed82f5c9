#!/usr/bin/env python3
"""How far apart are float32 realisations of the f16 engines' arithmetic?  Sets the factors of tests/test_gpu_f16_ref.py.

Default mode, CPU only, the HIP result never enters: for every case of tests/f16_cases.py and every reference configuration its
forms need (tests/f16_ref.py: the network in float64 with the engine's own roundings to halves), the plain float32 run of the same
restatement and DRAWS more float32 realisations of it (the channels of every product in a permuted order, the batch in another
order).  Per stage (cnn: signal -> features; rnn: features -> lasth; e2e: signal -> logits) and metric (the tensor's L2 error; the
largest per-channel L2 error): every member's error against float64, the median member's, the largest member's ratio to it.
factor = max(4, 1.5 x the largest ratio) per stage and metric; the head (fp32 against float64) keeps the factor 4 of
tests/train_cases.py.  "sensitivity": the float64 restatement with one deliberate defect against the unmutated one under these
factors, every row of f16_cases.MUTATIONS on every case it applies to; the rows outside f16_cases.REQUIRED are recorded only.
The norms count each distinct (reference row, result row) pair once (f16_cases.measures).

--hip (needs a GPU): the HIP engines' err / e_q per case, form and stage, merged into the same file under "hip"; the default mode
keeps an existing "hip" block.

    python tools/f16_ref_accuracy.py [--draws 8] [--hip] [--out profiles/f16_ref_accuracy.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import f16_cases as fc             # noqa: E402

HIP_NOTE = ("the fp16 / fp16-w2 engines against the same float64 restatement, error over the plain float32 run's (e_q), per case, "
            "form, stage and metric; measured after the factors were fixed")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=8)
    ap.add_argument("--hip", action="store_true")
    ap.add_argument("--out", default=fc.JSON)
    a = ap.parse_args()
    old = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if a.hip:
        if "factor" not in old:
            raise SystemExit("run the CPU ensemble first: --hip reads its factors from %s" % a.out)
        import f16_hip
        out = old
        worst, rows = f16_hip.measure_all(old["factor"])
        out["hip"] = {"note": HIP_NOTE, "largest_err_over_e_q": worst, "cases": rows}
    else:
        rows = {}
        for c in fc.CASES:
            rows[fc.case_id(c)] = fc.ensemble(c, a.draws)
            print(fc.case_id(c), {k: round(max(v["l2"]["max_over_median"], v["channel"]["max_over_median"]), 3) for k, v in rows[fc.case_id(c)].items()}, flush=True)
        largest, factor = fc.factors_from(rows)
        sens = {}
        for c in fc.CASES:
            sens[fc.case_id(c)] = fc.sensitivity(c, factor, sorted(fc.MUTATIONS))
            print(fc.case_id(c), {k: v["rejected"] for k, v in sens[fc.case_id(c)].items()}, flush=True)
        out = {"method": "float32 realisations of tests/f16_ref.py (plain + %d draws: channel orders of every product, batch order) against "
                         "float64; per stage and metric the largest member error over the median member's" % a.draws,
               "draws": a.draws, "floor": fc.FLOOR, "largest_max_over_median": largest, "factor": factor,
               "case_list": [fc.case_id(c) for c in fc.CASES], "cases": rows,
               "mutations": {k: v[1] for k, v in fc.MUTATIONS.items()}, "sensitivity": sens}
        if "hip" in old:
            out["hip"] = old["hip"]
        print("largest ratios %s -> factors %s" % (largest, factor))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
