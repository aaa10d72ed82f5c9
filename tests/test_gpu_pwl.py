"""GPU (-m gpu): block 1's table convolution (csrc/pwl.hip) against the float64 formula, at every row of the table, per position.

Every other GPU test feeds the kernel the integers of the synthetic signal with the synthetic weights: 52 of the table's 257 rows, all
but one with the reference point at the lower bound, judged by a norm over the tensor after three blocks (tests/test_pwl_cpu.py pins
that).  Here engines are built from a spec with block 1 ALONE (pwl_ref.one_block: engine creation accepts it), so that
Engine.features() is block 1's output -- the table's result through conv2c plus the signal branch -- and fed ragged windows holding
pwl_ref.samples_for: every breakpoint, its neighbours, the midpoints, +-0, non-integers, values far outside, the extremes next to the
padding (tests/pwl_hip.py CASES: the edges of the 32-position tile and of the (window, tile) block index, every left pad of the
stride-5 table, and every weight set of pwl_ref.WEIGHT_SETS -- zero-centred, planted(), equal breakpoints, no breakpoint at all).

Forms: fp32 (pwl_conv_kernel<0>), fp16 (<1>), fp32-split (<2>; Engine.features() returns hi + lo of its half pairs) and the lifted
form of CHIRON_NO_PWL=1 on fp32, which gets the same inputs and the same bar; the engine's profile proves which ran.  The half formats
get the capped sample set (no reference value above 3e4) and not planted(), whose constant channel of 1e9 no half can hold.

The bar, per position and never over the tensor: ||features[b, t] - ref64||_2 <= FACTOR * e32 + 1e-6 * ||ref64||_2, ref64 =
fp32_ref.cnn of the one-block spec in float64, e32 = the same in float32, FACTOR from the CPU (profiles/pwl_table_accuracy.json,
committed before any HIP result; the measured ratios go under "hip" there and into parity_pwl_<case>_<form>.json).  The fp16 engine
is judged against f16_ref.cnn's restatement with its roundings, per element and aware of rounding ties (pwl_ref.half_check: two
correct roundings to halves differ by a whole half-ulp at one position and by nothing at the next, so no ratio per position exists).
Exactly: everything finite; two runs give the same bytes; a window gives the same bits alone and in the batch; +0.0 and -0.0 give the
same bits."""
import numpy as np
import pytest

import pwl_hip
import pwl_ref as pr
from test_gpu_parity import _dump_report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def factor(built):
    return pr.committed()["factor"]


@pytest.mark.parametrize("c,form", pwl_hip.RUNS, ids=["%s-%s" % (pwl_hip.case_id(c), form) for c, form in pwl_hip.RUNS])
def test_block_1_meets_the_bar_at_every_position(factor, monkeypatch, c, form):
    out = pwl_hip.run_form(c, form, monkeypatch.setenv, monkeypatch.delenv)
    prof = out["profile"]
    assert prof.get("conv1_pwl", 0) == (0 if form == "fp32-lifted" else 1) and prof.get("conv_lift", 0) == (1 if form == "fp32-lifted" else 0), prof
    spec, w, x, sl, s, placed = pwl_hip.case_inputs(c, form in pwl_hip.HALF_FORMS)
    assert out["features"].shape == (x.shape[0], spec.output_len(c[1]), spec.blocks[0]["out"])
    row, exact = pwl_hip.judge_form(c, form, out, factor)
    _dump_report("pwl_%s_%s" % (pwl_hip.case_id(c), form), dict(row, exact_checks_failed=exact))
    print(pwl_hip.case_id(c), form, row)
    assert not exact, exact
    assert row["bad"] == 0, row


@pytest.mark.parametrize("form", list(pwl_hip.FORMS))
@pytest.mark.parametrize("name,L",[("synthetic-dna", 33), ("zero-centred", 33), ("synthetic-rna", 157)])
def test_plus_and_minus_zero_give_the_same_bits(built, monkeypatch, name, L, form):
    c = (name, L, 2, (form,), "")
    x = np.zeros((2, L), dtype=np.float32)
    x[1] = -0.0
    assert np.signbit(x[1]).all() and not np.signbit(x[0]).any()
    spec, w = pr.weight_set(name)
    T = spec.output_len(L)
    eng = pwl_hip.engine_of(c, form, 2, monkeypatch.setenv, monkeypatch.delenv)
    try:
        eng.infer(x, np.full(2, T, np.int32), want_prob=False)
        fea = eng.features()
    finally:
        eng.close()
    assert np.isfinite(fea).all() and np.array_equal(fea[0].view(np.uint32), fea[1].view(np.uint32))
