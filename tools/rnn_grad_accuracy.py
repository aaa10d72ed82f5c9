#!/usr/bin/env python
"""Measure err / e32 per tensor of the HIP gradients (the cases and the yardstick of tests/train_cases.py and
tests/test_gpu_train.py) and write them to profiles/rnn_grad_accuracy.json.  Needs a GPU."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rnn_grad_accuracy.json")
    import torch
    torch.cuda.init()
    import chiron_amd as ca
    import regimes
    import train_cases as tc
    cases = {}
    for kind, spec in tc.specs().items():
        for T in (60, 400):
            for source in ("random", "ctc"):
                rng = np.random.default_rng(100 + T)
                w = ca.synthetic_weights(spec, seed=7)
                fea = tc.random_features(24, T, 256, rng)
                sl = tc.ragged_seq_len(24, T, rng)
                dl = rng.normal(size=(24, T, 5)).astype(np.float32) if source == "random" else tc.ctc_dlogits(sl, rng, T)[0]
                cases["%s T=%d %s" % (kind, T, source)] = tc.accuracy(spec, w, fea, sl, dl)
    spec = ca.dna_default_spec()
    for name in regimes.SATURATED:
        rng = np.random.default_rng(7)
        fea = tc.random_features(24, 60, 256, rng)
        sl = tc.ragged_seq_len(24, 60, rng)
        cases["saturated %s" % name] = tc.accuracy(spec, regimes.saturated_gate_weights(spec, name), fea, sl,
                                                   rng.normal(size=(24, 60, 5)).astype(np.float32))
    # past the caps of the reductions over the rows (tests/train_cases.py, CAP_CASES)
    for kind, B, T, what in tc.CAP_CASES:
        spec, w, fea, sl, dl = tc.cap_case(kind, B, T)
        cases["%s B=%d T=%d past the %s cap" % (kind, B, T, what)] = tc.accuracy(spec, w, fea, sl, dl)
    # the ratio says nothing where the float32 yardstick itself has lost the gradient (e32 of order 1: underflow of a saturated regime)
    worst = max(((c, n, r["ratio"]) for c, rows in cases.items() for n, r in rows.items()
                 if r["e32_rel"] < 0.01 and r["norm"] > 0), key=lambda x: x[2])
    report = {"bar": "err <= %g * e32 + %g * ||g64||" % (tc.FACTOR, tc.FLOOR), "worst": {"case": worst[0], "tensor": worst[1], "ratio": worst[2]},
              "all_ok": all(r["ok"] for rows in cases.values() for r in rows.values()), "cases": cases}
    with open(out_path, "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report["worst"]), report["all_ok"])


if __name__ == "__main__":
    main()
