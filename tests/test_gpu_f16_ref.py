"""GPU (-m gpu): the fp16 and fp16-w2 engines against a float64 restatement WITH THEIR OWN ROUNDINGS (tests/f16_ref.py), stage by stage.

Every other f16 test judges these kernels against the fp32 engine at 0.08 on the logits (what half precision costs the network) or
against each other; an error shared by all forms of a stage, or one below what 11 mantissa bits cost, passes those.  Here every
case runs one engine per form and reads the engine's own taps:
  stage A   Engine.features()    against cnn(signal)                         pwl.hip, launch_lift, launch_stem_conv, stream16.hip, gemm.hip
  stage B   Engine.rnn_output()  against rnn(the engine's own features)      the projection GEMM's z, lstm16 / lstm16w / lstm16f / lstm16w2
  stage C   the logits           against head(the engine's own rnn_output)   fc_kernel
and, once per topology, the logits against the three reference stages composed from the signal.  The bar (tests/f16_cases.py):
err <= FACTOR * e_q + 1e-6 * scale for the tensor's L2 error and for the largest per-channel error, e_q = the same restatement
accumulated in float32, FACTOR from the CPU ensemble committed in profiles/f16_ref_accuracy.json before any HIP result (the measured
HIP ratios are recorded there under "hip" and do not enter it).  lasth and logits on the valid frames; past a row's seq_len lasth is
0 and the logits are the head's constant, exactly.  The engine's profile proves what it can tell apart: block 1 as the table or lifted,
and which layers ran a projection GEMM (fused or not).  It has one bucket for every recurrence kernel: that "wide-unfused" takes
lstm16w_kernel, "fused-pair" the two-group instantiation and fp16-w2 lstm16w2_kernel follows from launch_lstm's rules, which
tests/test_f16_ref_cpu.py reads out of the source and holds the engines' batch sizes to; "narrow" is lstm16_kernel, which the default
takes anyway at these batch sizes (bit-identical results: kept because the switch is a creation-time form of its own)."""
import numpy as np
import pytest

import f16_cases as fc
import f16_hip

pytestmark = pytest.mark.gpu

import functools

_RUNS = [(c, form) for c in fc.CASES for form in c[4]]


@functools.lru_cache(maxsize=None)
def _default_features(case_index):
    """the default form's features of a case, whichever tests ran before (the switches are cleared around the engine's creation)"""
    return f16_hip.run_form(fc.CASES[case_index], "default")["features"]


@pytest.fixture(scope="module")
def factor(built):
    return fc.committed()["factor"]


@pytest.mark.parametrize("c,form", _RUNS, ids=["%s-%s" % (fc.case_id(c), form) for c, form in _RUNS])
def test_f16_engine_stages_against_their_quantised_reference(factor, monkeypatch, c, form):
    spec = fc.specs()[c[0]]
    out = f16_hip.run_form(c, form, monkeypatch.setenv, monkeypatch.delenv)
    fc.expected_profile(spec, form, out["profile"])
    B, T = c[2], out["T"]
    assert out["features"].shape[:2] == (B, T) and out["lasth"].shape == (B, T, 2 * spec.hidden) and out["logits"].shape == (B, T, spec.classes)
    if form == "wide-unfused":
        import torch                      # lstm16w_kernel is taken when the 16-row workgroups fill the compute units (launch_lstm)
        assert torch.cuda.get_device_properties(0).multi_processor_count <= (fc.WIDE_BATCH // 16) * 2
    if form == "no-stream16" and T >= fc.STREAM3_MIN_T:
        # conv2b's streaming form sums the three taps' products in another order than the tiled GEMM: a switch that is silently
        # ignored gives the default's bits.  Below the 1 x 3 minimum only the 1 x 1 kernels stream, and they add each row's K
        # products in the tiled kernel's order: bit-identical features (measured at T = 1, 2 and 31), and no profile bucket names
        # the streaming kernels -- there nothing observable proves the switch; the case still holds both forms to the reference.
        assert not np.array_equal(out["features"], _default_features(fc.CASES.index(c)))
    rows, exact = f16_hip.judge_form(c, form, out, factor)
    for stage, r in rows.items():
        for m in ("l2", "channel"):
            print("%s %s %s %s: err %.3g (rel %.3g)  e_q %.3g  ratio %.3g  factor %.3g" % (fc.case_id(c), form, stage, m, r[m]["err"], r[m]["rel"],
                                                                                          r[m]["e_q"], r[m]["ratio"], factor[stage][m]))
    assert not exact, exact
    bad = {(stage, m): r[m] for stage, r in rows.items() for m in ("l2", "channel") if not r[m]["ok"]}
    assert not bad, bad
    assert ("e2e" in rows) == (c[5] and form == "default")
