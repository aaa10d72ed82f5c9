"""GPU: the fp32 LSTM x-projections as six-term bf16 products (gemm.hip gemm_proj_bf16x3_kernel), the fp32 engine's default
for K = 256 (layer 0) and K = 200 (the layers above), and its switch CHIRON_PROJ_FP32=1 (the fp32 MFMA kernels).

Engines are built on the DNA spec with rnn_layers 1, 2 and 3, so that each projection's output is the engine's output:
rnn_layers = 1 ends in the K = 256 kernel, 2 and 3 in the K = 200 kernel with its K tail."""
import json

import numpy as np
import pytest

import chiron_amd as ca
from test_gpu_parity import _dump_report

pytestmark = pytest.mark.gpu

TOL = 1e-4   # the project's bound of fp32 engine logits against the float64 oracle (test_gpu_parity.py)


def _layers(spec, n):
    return ca.ModelSpec(spec.blocks, spec.rnn_kind, n, spec.hidden, spec.classes, spec.bn_mode, spec.stem)


def _windows(B, L, seed):
    sig = ca.synthetic_signal(1, B * L, seed=seed)[0]
    return np.ascontiguousarray(sig[:B * L].reshape(B, L)).astype(np.float32)


@pytest.fixture(scope="module")
def dna(built):
    spec = ca.dna_default_spec()
    return spec, ca.synthetic_weights(spec, seed=21)


# name -> (B, segment_len, lengths or None for full windows)
CASES = {
    "B1": (1, 400, None),                                  # 15 padded rows
    "B17": (17, 400, None),                                # BP = 32, rows >= B
    "L61-B3": (3, 61, None),                               # M = T * BP = 976: not a multiple of 128
    "B48": (48, 400, None),                                # 750 tiles for 512 workgroups: later tiles come from the counter
    "ragged": (12, 400, [0, 1, 400, 399, 7, 400, 200, 3, 400, 0, 128, 129]),   # the reversed direction's placement
}

_oracle_cache = {}


def _oracle(spec, w, name):
    """float64 stages of a case, computed once: x, lengths, {n: logits of the n-layer network}"""
    if name not in _oracle_cache:
        from oracle import nn_oracle
        B, L, lens = CASES[name]
        x = _windows(B, L, seed=40 + len(name))
        ln = np.full(B, L, dtype=np.int64) if lens is None else np.array(lens, dtype=np.int64)
        for b in range(B):
            x[b, ln[b]:] = 0
        sd = spec.to_dict()
        w64 = {k: np.asarray(v, dtype=np.float64) for k, v in w.items()}
        sl = ca.seq_len_for_engine(ln, 1.0)
        prev = nn_oracle.cnn_forward(x.astype(np.float64), sd, w64)
        logits = {}
        for n in (1, 2, 3):
            prev = nn_oracle.rnn_layer_forward(prev, sl, sd, w64, n - 1)
            logits[n] = nn_oracle.fc_head(prev, w64)
        _oracle_cache[name] = (x, ln, logits)
    return _oracle_cache[name]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("n_layers", [1, 2, 3])
@pytest.mark.parametrize("name", list(CASES))
def test_shape_edges_against_the_oracle_and_across_schedules(dna, monkeypatch, name, n_layers):
    from oracle import ctc_oracle
    spec, w = dna
    B, L, _ = CASES[name]
    x, ln, ref = _oracle(spec, w, name)
    sp = _layers(spec, n_layers)
    for v in ("CHIRON_PROJ_FP32", "CHIRON_STATIC_TILES"):
        monkeypatch.delenv(v, raising=False)
    with ca.Engine(sp, w, max_batch=B, segment_len=L, n_slots=3) as eng:
        assert eng.ratio == 1.0
        sl = ca.seq_len_for_engine(ln, eng.ratio)
        res = [eng.infer(x, sl, want_prob=True, want_logits=True, slot=s) for s in range(3)]
        lasth = eng.rnn_output()
        got = res[0].logits
        mask = (np.arange(got.shape[1])[None, :] < sl[:, None])[..., None]
        err = float((np.abs(got - ref[n_layers]) * mask).max())
        print("%s layers %d: max |logit - float64| = %.3g" % (name, n_layers, err))
        assert np.isfinite(got).all() and err < TOL
        # greedy decode of the engine equals the oracle's decode of the engine's own logits
        rows, _ = ctc_oracle.greedy_decode(got, sl)
        idx, val, shape = ctc_oracle.rows_to_sparse(rows, B)
        assert np.array_equal(res[0].decoded.indices, idx) and np.array_equal(res[0].decoded.values, val)
        assert np.array_equal(res[0].decoded.dense_shape, shape)
        # same bits from every slot
        for r in res[1:]:
            assert np.array_equal(_bits(r.logits), _bits(got))
        # a row run alone has the bits it has in the batch
        for b in sorted({0, B // 2, B - 1}):
            alone = eng.infer(x[b:b + 1], sl[b:b + 1], want_logits=True, slot=1)
            assert np.array_equal(_bits(alone.logits[0]), _bits(got[b])), b
    monkeypatch.setenv("CHIRON_STATIC_TILES", "1")
    with ca.Engine(sp, w, max_batch=B, segment_len=L) as eng:
        st = eng.infer(x, sl, want_logits=True)
        assert np.array_equal(_bits(st.logits), _bits(got))
    monkeypatch.delenv("CHIRON_STATIC_TILES")
    # the switch: the fp32 MFMA projections are another kernel (other bits somewhere), inside the same bound, equal across slots
    monkeypatch.setenv("CHIRON_PROJ_FP32", "1")
    with ca.Engine(sp, w, max_batch=B, segment_len=L, n_slots=2) as eng:
        f = [eng.infer(x, sl, want_logits=True, slot=s) for s in range(2)]
        lasth32 = eng.rnn_output()
    assert np.array_equal(_bits(f[0].logits), _bits(f[1].logits))
    assert float((np.abs(f[0].logits - ref[n_layers]) * mask).max()) < TOL
    if sl.sum() >= 64:
        assert not np.array_equal(_bits(lasth32), _bits(lasth)), "CHIRON_PROJ_FP32 changed nothing: is the bf16 form running?"


@pytest.mark.parametrize("n_layers", [1, 2])
def test_error_born_in_the_layer_is_fp32_class_and_unbiased(built, monkeypatch, n_layers):
    """Trained-like weights (tests/regimes.py), 64 windows.  Local error of a layer = its output against the float64 layer applied to
    the engine's OWN input of that layer (the features, or the output of the engine with one layer less), as tools/parity_budget.py
    measures it.  The six-term form may not lose more than 1.5 x what the fp32 MFMA form loses (the margin BARS gives a typical float32
    realisation against the ensemble median; the fp32 form is the reference, never the new code), and the two forms' outputs may not
    differ by a bias: |mean signed difference| < rms difference / 10.  The figures are written next to the other parity reports
    (test_gpu_parity._dump_report) as parity_proj_bf16x3_layers<n>.json."""
    import regimes
    from oracle import nn_oracle
    spec = ca.dna_default_spec()
    B, L = 64, 400
    x = _windows(B, L, seed=67)
    ln = np.full(B, L, dtype=np.int64)
    ln[2], ln[5] = L // 3, 0
    w, _ = regimes.trained_like_weights(spec, x, seed=5)
    sd = spec.to_dict()
    w64 = {k: np.asarray(v, dtype=np.float64) for k, v in w.items()}
    out, local = {}, {}
    for form in ("bf16x3", "fp32"):
        monkeypatch.delenv("CHIRON_PROJ_FP32", raising=False)
        if form == "fp32":
            monkeypatch.setenv("CHIRON_PROJ_FP32", "1")
        stages = {}
        for n in range(1, n_layers + 1):
            with ca.Engine(_layers(spec, n), w, max_batch=B, segment_len=L) as eng:
                sl = ca.seq_len_for_engine(ln, eng.ratio)
                eng.infer(x, sl)
                stages[n] = eng.rnn_output()
                if n == 1:
                    stages[0] = eng.features()
        want = nn_oracle.rnn_layer_forward(stages[n_layers - 1].astype(np.float64), sl, sd, w64, n_layers - 1)
        mask = (np.arange(want.shape[1])[None, :] < sl[:, None])[..., None]
        d = (stages[n_layers] - want) * mask
        local[form] = float(np.sqrt((d ** 2).sum() / (mask.sum() * want.shape[2])))
        out[form] = stages[n_layers] * mask
    monkeypatch.delenv("CHIRON_PROJ_FP32", raising=False)
    diff = (out["bf16x3"].astype(np.float64) - out["fp32"].astype(np.float64))
    nval = float(mask.sum() * diff.shape[2])
    rms_diff = float(np.sqrt((diff ** 2).sum() / nval))
    mean_diff = float(diff.sum() / nval)
    report = {"local_rms_bf16x3": local["bf16x3"], "local_rms_fp32": local["fp32"], "ratio": local["bf16x3"] / local["fp32"],
              "rms_difference_of_forms": rms_diff, "mean_signed_difference_of_forms": mean_diff}
    print(json.dumps(report))
    _dump_report("proj_bf16x3_layers%d" % n_layers, report)
    assert local["bf16x3"] <= 1.5 * local["fp32"], report
    assert rms_diff > 0 and abs(mean_diff) < 0.1 * rms_diff, report
