#!/usr/bin/env python3
"""How far apart are float32 realisations of the fp32 engine's stages?  Sets the factors of tests/test_gpu_fp32_ref.py.

Default mode, CPU only, the HIP result never enters: for every case of tests/fp32_cases.py and every stage (cnn: signal -> features,
in the case's own conv2b form; rnn<l>: layer l from the float64 restatement's previous output), the plain float32 run of
tests/fp32_ref.py and DRAWS more float32 realisations of it (the channels of every product in a permuted order, the batch in another
order).  Per stage and metric (the tensor's L2 error; the largest per-channel L2 error): every member's error against float64, the
median member's, the largest member's ratio to it.  factor = max(4, 1.5 x the largest ratio) per stage kind and metric; the head
keeps the factor 4 of tests/f16_cases.py.  "sensitivity": the float64 restatement with one deliberate defect against the unmutated
one under these factors, every row of fp32_cases.DEFECTS on every case it applies to, with the deviation the defect causes on the
logits (what the suite's older 1e-4 bar sees) for the operand defects; the rows outside fp32_cases.REQUIRED are recorded only.
The norms count each distinct (reference row, result row) pair once (f16_cases.measures).

--hip (needs a GPU): the fp32 engine's err / e32 per case, form and stage, merged into the same file under "hip"; the default mode
keeps an existing "hip" block.

    python tools/fp32_stage_accuracy.py [--draws 8] [--hip] [--out profiles/fp32_stage_accuracy.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fp32_cases as pc            # noqa: E402

HIP_NOTE = ("the fp32 engine against the float64 restatement of each stage applied to the engine's own previous output, error over the "
            "plain float32 run's (e32), per case, form, stage and metric; measured after the factors were fixed")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=pc.DRAWS)
    ap.add_argument("--hip", action="store_true")
    ap.add_argument("--out", default=pc.JSON)
    a = ap.parse_args()
    old = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if a.hip:
        if "factor" not in old:
            raise SystemExit("run the CPU ensemble first: --hip reads its factors from %s" % a.out)
        import fp32_hip
        out = old
        worst, rows = fp32_hip.measure_all(old["factor"])
        out["hip"] = {"note": HIP_NOTE, "largest_err_over_e32": worst, "cases": rows}
    else:
        rows = {}
        for c in pc.CASES:
            rows[pc.case_id(c)] = pc.ensemble(c, a.draws)
            print(pc.case_id(c), {k: round(max(v["l2"]["max_over_median"], v["channel"]["max_over_median"]), 3) for k, v in rows[pc.case_id(c)].items()}, flush=True)
        largest, factor = pc.factors_from(rows)
        sens = {}
        for c in pc.CASES:
            sens[pc.case_id(c)] = pc.sensitivity(c, factor, sorted(pc.DEFECTS))
            print(pc.case_id(c), {k: v["rejected"] for k, v in sens[pc.case_id(c)].items()}, flush=True)
        out = {"method": "float32 realisations of tests/fp32_ref.py (plain + %d draws: channel orders of every product, batch order) against "
                         "float64, each case in its own conv2b form; per stage and metric the largest member error over the median member's" % a.draws,
               "draws": a.draws, "floor": pc.FLOOR, "gates": pc.GATES, "weight_seed": pc.WEIGHT_SEED,
               "largest_max_over_median": largest, "factor": factor,
               "case_list": [pc.case_id(c) for c in pc.CASES], "conv2b_form": {pc.case_id(c): pc.conv2b_form(c) for c in pc.CASES},
               "cases": rows, "defects": {k: v[1] for k, v in pc.DEFECTS.items()}, "required": list(pc.REQUIRED), "p3_note": pc.P3_NOTE,
               "sensitivity": sens,
               "largest_logit_deviation": {n: max(r[n]["max_logit_deviation"] for r in sens.values() if n in r) for n in pc.LOGIT_RECORD}}
        if "hip" in old:
            out["hip"] = old["hip"]
        print("largest ratios %s -> factors %s" % (largest, factor))
        print("largest logit deviations", out["largest_logit_deviation"])
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
