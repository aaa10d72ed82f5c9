"""CPU tests of the CNN training seam: the float64 reference against the oracle, the host-only ABI queries, init_weights, the
batch-BN checkpoint writer and the `train` command line."""
import ctypes as C
import math

import numpy as np
import pytest

import chiron_amd as ca
from chiron_amd import _lib, entry, tf_bundle, train

import cnn_ref
import cnn_train_cases as cc


@pytest.mark.parametrize("kind", cc.SPECS)
def test_cnn_ref_float64_forward_equals_the_oracle_in_batch_mode(kind):
    """The yardstick is pinned to the existing oracle, not to the code under test."""
    from oracle import nn_oracle
    spec = cc.spec_of(kind, "batch")
    w = ca.synthetic_weights(spec, seed=7)
    x = ca.synthetic_signal(5, 230, seed=9).astype(np.float64)
    ref = nn_oracle.cnn_forward(x, spec.to_dict(), {k: np.asarray(v, dtype=np.float64) for k, v in w.items()})
    got, mom = cnn_ref.forward(x, spec, w)
    assert got.shape == ref.shape == (5, spec.output_len(230), 256)
    assert np.abs(got - ref).max() <= 1e-12
    assert len(mom) == sum(1 for _, _, has_bn in spec._sites() if has_bn)


@pytest.mark.parametrize("kind", cc.SPECS)
def test_cnn_params_range_and_the_recurrent_one_tile_the_blob(built, kind):
    spec = cc.spec_of(kind)
    layout = spec.blob_layout()
    names = list(layout)
    sizes = [int(np.prod(s)) for s in layout.values()]
    n_cnn = sum(sizes[:names.index(spec.lstm_scope(0, "fw") + "kernel")])
    assert train.cnn_params_range(spec) == (0, n_cnn)
    first, n = train.params_range(spec)
    assert first == n_cnn and first + n == sum(sizes)
    off = 0
    for name, (o, shape) in train.cnn_param_layout(spec).items():
        assert o == off and tuple(layout[name]) == shape
        off += int(np.prod(shape))
    assert off == n_cnn


def test_cnn_train_sizes_are_linear_in_the_batch(built):
    """Tape: per row.  Workspace: four activation buffers per row + partial sums whose slice counts are capped, so it is linear
    once the caps are reached."""
    spec = ca.dna_default_spec()
    t16, _ = train.cnn_train_sizes(spec, 16, 400)
    t32, _ = train.cnn_train_sizes(spec, 32, 400)
    t300, w300 = train.cnn_train_sizes(spec, 300, 400)
    stats = t16 - 16 * (t32 - t16) // 16                      # the per-site statistics do not grow
    assert (t32 - t16) * 300 // 16 + stats == t300 and 0 <= stats < 1 << 16
    _, w600 = train.cnn_train_sizes(spec, 600, 400)
    _, w900 = train.cnn_train_sizes(spec, 900, 400)
    _, w1200 = train.cnn_train_sizes(spec, 1200, 400)
    assert w900 - w600 == w1200 - w900 > 0
    assert t300 + w300 < 3 << 30                              # the issue's memory budget at the reference's batch


def _status(spec, batch, seg):
    desc = spec.to_c()
    a, b = C.c_size_t(), C.c_size_t()
    return _lib.load().chiron_cnn_train_sizes(C.byref(desc), batch, seg, C.byref(a), C.byref(b))


def test_cnn_train_sizes_refuse_bad_and_oversized_shapes(built):
    spec = ca.dna_default_spec()
    assert _status(spec, 16, 400) == _lib.OK
    assert _status(spec, 16, 0) == _lib.ERR_INVALID
    assert _status(spec, 0, 400) == _lib.ERR_INVALID
    assert _status(spec, -2, 400) == _lib.ERR_INVALID
    assert _status(spec, (1 << 20) + 1, 1) == _lib.ERR_OVERFLOW
    assert _status(spec, 1 << 19, 400) == _lib.ERR_OVERFLOW        # more than 2^24 rows
    assert _status(spec, 16, 8193) == _lib.ERR_OVERFLOW            # more than CHIRON_CTC_MAX_T frames
    assert b"frames" in _lib.load().chiron_last_error()
    assert _status(ca.rna_default_spec(), 16, 8193) == _lib.OK     # stride 5: 1639 frames
    bad = ca.dna_default_spec().to_c()
    bad.blocks[1].in_channels = 7
    a, b = C.c_size_t(), C.c_size_t()
    assert _lib.load().chiron_cnn_train_sizes(C.byref(bad), 16, 400, C.byref(a), C.byref(b)) == _lib.ERR_INVALID
    assert _lib.load().chiron_cnn_params_range(C.byref(bad), C.byref(a), C.byref(b)) == _lib.ERR_INVALID


@pytest.mark.parametrize("bn_mode", ["population", "batch"])
@pytest.mark.parametrize("kind", ["dna", "rna_model3"])
def test_init_weights_variable_set_and_distributions(kind, bn_mode):
    spec = cc.spec_of(kind, bn_mode)
    w = train.init_weights(spec, seed=3)
    assert list(w) == list(spec.blob_layout())
    for name, shape in spec.blob_layout().items():
        assert w[name].shape == tuple(shape) and w[name].dtype == np.float32, name
    # exactly the variable set of a checkpoint of this BN naming, through the writer's aliasing
    assert set(spec.variables()) <= set(w) | {n for s, _, bn in spec._sites() if bn for n in spec.bn_names(s) if n}
    H = spec.hidden
    checked = 0
    for name, a in w.items():
        if a.size < 25000:
            continue
        if name.endswith("/weights") and a.ndim == 4:
            _, k, ci, co = a.shape
            want = math.sqrt(2.0 / (k * ci + k * co))              # Xavier normal: fan-avg
        elif name.endswith("lstm_cell/kernel"):
            want = math.sqrt(6.0 / (a.shape[0] + 4 * H)) / math.sqrt(3.0)   # Glorot uniform: limit / sqrt(3)
        else:
            continue
        got = float(a.std(ddof=1))
        assert abs(got - want) <= 0.1 * want, (name, got, want)
        assert abs(float(a.mean())) <= 0.05 * want, name
        checked += 1
    assert checked >= 10
    for site, shape, has_bn in spec._sites():
        if has_bn:
            assert not w[site + "_bn/pop_mean"].any() and (w[site + "_bn/pop_var"] == 1).all()
            if bn_mode == "population":
                assert (w[site + "_bn/scale"] == np.float32(0.1)).all()
                assert np.abs(w[site + "_bn/offset"]).max() <= math.sqrt(3.0 / shape[-1])
    assert not w["rnn_fnn_layer/bias"].any() and not w[spec.lstm_scope(0, "fw") + "bias"].any()
    assert train.init_weights(spec, seed=3)["rnn_fnn_layer/weights"].tobytes() == w["rnn_fnn_layer/weights"].tobytes()
    assert train.init_weights(spec, seed=4)["rnn_fnn_layer/weights"].tobytes() != w["rnn_fnn_layer/weights"].tobytes()


@pytest.mark.parametrize("kind", ["dna", "rna_model2"])
def test_batch_bn_model_round_trips_through_save_and_load(built, tmp_path, kind):
    spec = cc.spec_of(kind, "batch")
    w = train.init_weights(spec, seed=5)
    out = str(tmp_path / "model")
    cfg = {"cnn": {"model": "dna_model1" if kind == "dna" else "rna_model2"}}
    train.save_model(out, spec, w, 17, train.config_for(spec, cfg, "Adam", 0.0))
    entries = tf_bundle.read_index(tf_bundle.latest_checkpoint(out) + ".index")
    assert set(k for k in entries if k) == set(spec.variables()) | {"global_step"}
    assert not any("pop_mean" in k or "pop_var" in k for k in entries)
    assert train._checkpoint_step(out) == 17
    spec2, w2, _ = ca.load_model(out)
    assert spec2.bn_mode == "batch" and spec2.to_dict() == spec.to_dict()
    for name in spec.blob_layout():
        assert np.asarray(w2[name]).tobytes() == np.asarray(w[name]).tobytes(), name


def test_train_command_line_defaults_equal_the_reference():
    a = entry.build_parser().parse_args(["train", "-i", "in", "-o", "out"])
    assert a.func is entry.train
    assert (a.sequence_len, a.batch_size, a.step_rate, a.max_steps, a.segments_num) == (400, 300, 4e-3, 10000, None)   # chiron_rcnn_train.py:192-203
    assert (a.model, a.validation, a.configure, a.gradient_clip, a.retrain, a.bn) == (None, None, None, None, False, "batch")
    assert (a.fl_gamma, a.opt_method, a.sig_norm, a.device, a.synthetic_weights) == (0.0, "Adam", "none", 0, False)
    b = entry.build_parser().parse_args(["train", "-i", "in", "-o", "out", "-m", "mod", "-v", "val", "-s", "300", "-b", "16", "-t", "1e-3",
                                         "-x", "40", "-n", "500", "--configure", "c.json", "--gradient_clip", "5", "--retrain",
                                         "--bn", "population", "--report-every", "2", "--seed", "3"])
    assert (b.model, b.validation, b.sequence_len, b.batch_size, b.step_rate, b.max_steps, b.segments_num) == ("mod", "val", 300, 16, 1e-3, 40, 500)
    assert (b.configure, b.gradient_clip, b.retrain, b.bn, b.report_every, b.seed) == ("c.json", 5.0, True, "population", 2, 3)
