"""GPU (-m gpu): the fp32 engine against a float64 restatement of each of its stages, in every kernel form, at the shape edges.

Every other test away from the headline geometry judges the fp32 engine at the end of the network, |logit - oracle| < 1e-4: 20 to 70
times what float32 arithmetic costs there, and a weight operand at 16 significant bits at one site passes it
(profiles/fp32_stage_accuracy.json "largest_logit_deviation").  Here every (case, form) of tests/fp32_cases.py builds engines of
1 .. n rnn_layers and reads the engine's own taps:
  cnn       Engine.features()                         against cnn(signal), in the case's conv2b form (direct, F(2,3), F(4,3))
  rnn<l>    the l-layer engine's Engine.rnn_output()  against layer l applied to the engine's own previous output
  head      the logits                                against head(the engine's own lasth)
The bar (tests/fp32_cases.py): err <= FACTOR * e32 + 1e-6 * scale for the tensor's L2 error and for the largest per-channel error,
e32 = the same restatement accumulated in float32 (tests/fp32_ref.py), FACTOR from the CPU ensemble committed in
profiles/fp32_stage_accuracy.json before any HIP result (the measured ratios are recorded there under "hip" and do not enter it).
Layer outputs and logits on the valid frames; past a row's seq_len every layer's output is 0 and the logits are the head's
constant, exactly.  The engine's profile proves what it can tell apart: conv2b in a Winograd form or not, block 1 as the table or
lifted, the projection GEMMs of every layer.  It has one bucket for every recurrence kernel and one for both projection kernels:
that "wide0" / "wide1" / "pair" take lstm_kernel<1> / lstm32w_kernel / lstm_kernel<2> follows from launch_lstm's rules, which
tests/test_fp32_ref_cpu.py reads out of the source; "proj-fp32" must give other bits than the six-term default.  Every ratio of a
run is written next to the other parity reports (test_gpu_parity._dump_report) as parity_fp32_ref_<case>_<form>.json.
The last test turns the bar on the engine itself: fed ONE weight tensor at 16 significant bits, it must miss the bar at the stage that
multiplies by it (measured 71 / 208, 56 / 105 and 9.8 / 12 x e32) and meet it at every other one."""
import functools

import numpy as np
import pytest

import fp32_cases as pc
import fp32_hip
from test_gpu_parity import _dump_report

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _default_lasth(case_index):
    """the default form's last layer of a case, whichever tests ran before (the switches are cleared around every engine's creation)"""
    return fp32_hip.run_form(pc.CASES[case_index], "default")["layers"][-1]


@pytest.fixture(scope="module")
def factor(built):
    return pc.committed()["factor"]


@pytest.mark.parametrize("c,form", pc.RUNS, ids=["%s-%s" % (pc.case_id(c), form) for c, form in pc.RUNS])
def test_fp32_engine_stages_against_their_float64_restatement(factor, monkeypatch, c, form):
    spec = pc.specs()[c[0]]
    out = fp32_hip.run_form(c, form, monkeypatch.setenv, monkeypatch.delenv)
    for n, prof in enumerate(out["profiles"]):
        pc.expected_profile(spec, c, n + 1, prof)
    B, T = c[2], out["T"]
    assert out["features"].shape[:2] == (B, T) and out["logits"].shape == (B, T, spec.classes)
    assert all(h.shape == (B, T, 2 * spec.hidden) for h in out["layers"]) and len(out["layers"]) == spec.rnn_layers
    if form == "proj-fp32":
        assert not np.array_equal(out["layers"][-1].view(np.uint32), _default_lasth(pc.CASES.index(c)).view(np.uint32)), \
            "CHIRON_PROJ_FP32 changed nothing: is the six-term form running?"
    rows, exact = fp32_hip.judge_form(c, form, out, factor)
    _dump_report("fp32_ref_%s_%s" % (pc.case_id(c), form), fp32_hip.report(rows, exact))
    for stage, r in rows.items():
        for m in ("l2", "channel"):
            print("%s %s %s %s: err %.3g (rel %.3g)  e32 %.3g  ratio %.3g  factor %.3g" % (pc.case_id(c), form, stage, m, r[m]["err"], r[m]["rel"],
                                                                                           r[m]["e_q"], r[m]["ratio"], factor[pc.kind(stage)][m]))
    assert not exact, exact
    bad = {(stage, m): r[m] for stage, r in rows.items() for m in ("l2", "channel") if not r[m]["ok"]}
    assert not bad, bad


@pytest.mark.parametrize("key,rows_of,stage", [("BDLSTM_rnn/cell_0/bidirectional_rnn/fw/lstm_cell/kernel", slice(0, 256), "rnn1"),
                                               ("BDLSTM_rnn/cell_1/bidirectional_rnn/fw/lstm_cell/kernel", slice(0, 200), "rnn2"),
                                               ("res_layer3/branch2/conv2c/weights", slice(None), "cnn")],
                         ids=["wx-layer0", "wx-layer1", "conv2c-last"])
def test_an_engine_fed_one_operand_at_16_bits_fails_that_stage_only(factor, monkeypatch, key, rows_of, stage):
    """the wiring of this file, on the engine itself: the engine gets ONE weight tensor rounded to 16 significant bits (W_x of a
    forward projection; the last block's conv2c filter), the reference keeps the true weights.  The stage that multiplies by it must
    miss the bar; every other stage, judged from the engine's own previous output, must still meet it."""
    import fp32_ref
    c = pc.CASES[[pc.case_id(v) for v in pc.CASES].index("dna-L61-B4")]
    spec, w, x, sl, T = pc.case_inputs(c)
    coarse = dict(w)
    k = np.array(w[key], copy=True)
    flat = k.reshape(-1, k.shape[-1])
    flat[rows_of] = fp32_ref.round_bits(flat[rows_of])
    coarse[key] = k
    assert not np.array_equal(k, w[key])
    out = fp32_hip.run_form(c, "default", monkeypatch.setenv, monkeypatch.delenv, weights=coarse)
    rows, exact = fp32_hip.judge_form(c, "default", out, factor)
    assert not exact, exact
    ok = {st: r["l2"]["ok"] and r["channel"]["ok"] for st, r in rows.items()}
    print(stage, {st: "%.3g / %.3g" % (r["l2"]["ratio"], r["channel"]["ratio"]) for st, r in rows.items()})
    assert ok == {st: st != stage for st in rows}, (ok, {st: (r["l2"]["ratio"], r["channel"]["ratio"]) for st, r in rows.items()})
