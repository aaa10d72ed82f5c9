#!/usr/bin/env python3
"""How far is block 1's table (csrc/weight_pack.h, evaluated as csrc/pwl.hip evaluates it) from the formula it tabulates, measured in
float32 realisations of that formula?  Sets the factor of tests/test_pwl_cpu.py and tests/test_gpu_pwl.py.

Default mode, CPU only, the HIP result never enters: for every weight set of tests/pwl_ref.py the packed table is read back
(tests/native/pwl_table_dump.cpp), evaluated in the kernel's arithmetic (pwl_ref.table_eval) on windows that hold every sample of
pwl_ref.samples_for, and compared per position with the float64 formula -- per sample and tap, at conv2b's output, and chained
through the rest of the block in float32 -- over the plain float32 yardstick and DRAWS channel orders of it.  factor = max(4, 1.5 x
the largest err / e32), the construction of tests/fp32_cases.py; positions whose error is below the floor enter no ratio.

--hip (needs a GPU): the engines' err / e32 per case and form of tests/pwl_hip.py, merged into the same file under "hip"; the
default mode keeps an existing "hip" block.

    python tools/pwl_table_accuracy.py [--draws 8] [--hip] [--out profiles/pwl_table_accuracy.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pwl_ref as pr            # noqa: E402

LEVELS = ("taps", "y2b", "features")
HIP_NOTE = ("one-block engines against the float64 restatement, per position (fp16: per element, aware of rounding ties): the largest "
            "error over the plain float32 run's (e32) among the positions above the floor, per case and form; measured after the factor was fixed")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=pr.DRAWS)
    ap.add_argument("--hip", action="store_true")
    ap.add_argument("--out", default=pr.JSON)
    a = ap.parse_args()
    old = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if a.hip:
        if "factor" not in old:
            raise SystemExit("run the CPU ensemble first: --hip reads its factor from %s" % a.out)
        import pwl_hip
        out = old
        worst, rows = pwl_hip.measure_all(old["factor"])
        out["hip"] = {"note": HIP_NOTE, "largest_err_over_e32": worst, "cases": rows}
    else:
        sets = {}
        for name in pr.WEIGHT_SETS:
            sets[name] = pr.cpu_ratios(name, a.draws)
            print(name, sets[name], flush=True)
        largest = {lv: max(r[lv] for r in sets.values()) for lv in LEVELS}
        out = {"method": "pwl_ref.table_eval on the packed table against pwl_ref.formula in float64, per position; e32 = the formula in float32 "
                         "(plain + %d channel orders); the largest err / e32 over the positions whose error is above the floor" % a.draws,
               "draws": a.draws, "floor": pr.FLOOR, "weight_sets": list(pr.WEIGHT_SETS), "sets": sets,
               "largest_err_over_e32": largest, "factor": {lv: pr.factor_of(v) for lv, v in largest.items()}}
        if "hip" in old:
            out["hip"] = old["hip"]
        print("largest ratios %s -> factors %s" % (largest, out["factor"]))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
