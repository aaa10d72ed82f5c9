"""GPU (-m gpu): the engine at every topology its descriptor accepts (tests/topology_cases.py), against the float64 oracle.

Per row: the engine's frame count, ratio and logits shape are the spec's; its CNN features and its logits lie within FACTOR x the
float32 oracle's own error of the float64 oracle, per window (topology_cases.judge: the features say which half is wrong when the
logits are); the greedy decode of the engine's own logits is the oracle's bit for bit, and where the row asks for it the beam search at
width 5; the engine's profile shows the conv2b forms the packer's rule predicts (Winograd launches, the table or the lifted form);
and a second identical call returns the same bits.

CHIRON_TOPOLOGY_RECORD=<file>: every row also appends its measured figures there (profiles/topology_accuracy.json is such a run)."""
import json
import os

import numpy as np
import pytest

import chiron_amd as ca
from chiron_amd import _lib

import topology_cases as tc
from test_gpu_parity import _check_beam, _check_decode

pytestmark = pytest.mark.gpu
_DEVICE_ERRORS = []        # rows in which the HIP runtime failed: the rows after them fail without touching the device

_SWITCHES = ("CHIRON_WINOGRAD_F2", "CHIRON_WINOGRAD_F4", "CHIRON_NO_WINOGRAD", "CHIRON_NO_PWL", "CHIRON_NO_STREAM32", "CHIRON_LSTM_WIDE",
             "CHIRON_LSTM_PAIR", "CHIRON_PROJ_FP32", "CHIRON_STATIC_TILES", "CHIRON_BEAM_SINGLE", "CHIRON_BEAM_GENERIC")


@pytest.fixture
def clean_env(monkeypatch):
    for v in _SWITCHES:
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


def _record(name, row):
    path = os.environ.get("CHIRON_TOPOLOGY_RECORD")
    if not path:
        return
    rows = {}
    if os.path.exists(path):
        with open(path) as f:
            rows = json.load(f)
    rows[name] = row
    with open(path, "w") as f:
        json.dump(rows, f, indent=1, sort_keys=True)


@pytest.mark.parametrize("name", [c.name for c in tc.CASES])
def test_topology_against_the_oracle(built, clean_env, name):
    if _DEVICE_ERRORS:
        pytest.fail("not run: the device reported an error in row %s, and nothing more is started on it" % _DEVICE_ERRORS[0])
    c = tc.BY_NAME[name]
    spec, w, x, sl, T = tc.inputs(name)
    f64, l64 = tc.reference(name)
    e32 = tc.yardstick(name)
    try:
        with ca.Engine(spec, w, max_batch=c.B, segment_len=c.L, dtype=c.dtype, max_beam=c.max_beam) as eng:
            assert eng.T == T and eng.ratio == c.L / T
            eng.profile(True)
            res = eng.infer(x, sl, want_prob=True, want_logits=True)
            prof = {k: v["launches"] for k, v in eng.profile_read().items()}
            eng.profile(False)
            fea = eng.features()
            again = eng.infer(x, sl, want_prob=True, want_logits=True)
            fea_again = eng.features()
            beam = eng.infer(x, sl, beam_width=5, want_prob=True, want_logits=True) if c.max_beam else None
    except _lib.ChironError as err:
        if err.status == _lib.ERR_DEVICE:
            _DEVICE_ERRORS.append(name)
        raise
    assert res.logits.shape == (c.B, T, spec.classes) and fea.shape == f64.shape
    ok_f, ratio_f, err_f, bound_f = tc.judge(fea, f64, e32["features"])
    ok_l, ratio_l, err_l, bound_l = tc.judge(res.logits, l64, e32["logits"], sl)
    row = {"why": c.why, "features": {"e32": e32["features"], "err": float(err_f.max()), "err_over_e32": ratio_f, "within_bar": ok_f},
           "logits": {"e32": e32["logits"], "err": float(err_l.max()), "err_over_e32": ratio_l, "within_bar": ok_l}}
    print("topology %s: features err / e32 = %.3f (e32 %.3g), logits err / e32 = %.3f (e32 %.3g); launches %s"
          % (name, ratio_f, e32["features"], ratio_l, e32["logits"], prof))
    _record(name, row)
    assert np.isfinite(fea).all() and np.isfinite(res.logits).all()
    want = tc.expected_profile(spec, c.L, c.dtype)
    assert {k: prof.get(k, 0) for k in want} == want, prof
    assert "ctc_beam" not in prof
    assert ok_f, ("features", ratio_f, err_f, bound_f)
    assert ok_l, ("logits", ratio_l, err_l, bound_l)
    _check_decode(res, res.logits, sl, c.B)
    assert np.array_equal(again.logits, res.logits) and np.array_equal(fea_again, fea)
    assert np.array_equal(again.decoded.values, res.decoded.values) and np.array_equal(again.decoded.indices, res.decoded.indices)
    if beam is not None:
        assert np.array_equal(beam.logits, res.logits)
        _check_beam(beam, beam.logits, sl, 5, c.B)
