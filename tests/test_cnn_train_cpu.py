"""CPU tests of the CNN training seam: the float64 reference against the oracle, the host-only ABI queries, init_weights, the
batch-BN checkpoint writer and the `train` command line."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import chiron_amd as ca
from chiron_amd import _lib, entry, tf_bundle, train

import cnn_ref
import cnn_train_cases as cc
import train_cases as tc


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


# ---------------------------------------------------------------------------------------------
# the cases past the reduction caps against the kernels' own constants
# ---------------------------------------------------------------------------------------------
class _CgGeometry:
    """csrc/cnn_grad.hip's slicing of a site's rows, restated: cg_slices with its unrounded chunk (cg_sum_kernel,
    cg_bn_bwd_sum_kernel, cg_rank1_dw_kernel) and cg_nsplit with cg_dw_kernel's chunk, rounded up to the k-tile."""
    def __init__(self):
        k = tc.kernel_constants("cnn_grad.hip", ["CG_SLICE_ROWS", "CG_MAX_SLICES", "CG_DW_SPLIT_ROWS", "CG_DW_MAX_SPLIT", "CK"])
        self.slice_rows, self.max_slices, self.split_rows, self.max_split, self.ck = (
            k["CG_SLICE_ROWS"], k["CG_MAX_SLICES"], k["CG_DW_SPLIT_ROWS"], k["CG_DW_MAX_SPLIT"], k["CK"])

    def slice_chunk(self, rows):
        return -(-rows // min(max(-(-rows // self.slice_rows), 1), self.max_slices))

    def nslices(self, rows):
        return -(-rows // self.slice_chunk(rows))

    def nsplit(self, rows):
        return min(max(-(-rows // self.split_rows), 1), self.max_split)

    def dw_chunk(self, rows):
        return -(-(-(-rows // self.nsplit(rows))) // self.ck) * self.ck


def _ragged_last(rows, n, chunk):
    tc.assert_slices_tile(rows, n, chunk)
    last = tc.slices(rows, n, chunk)[-1]
    assert 0 < last[1] - last[0] < chunk
    return last[1] - last[0]


def test_cap_cases_lie_past_the_caps_of_the_kernels_constants():
    """CAP_GRAD_CASES exist to run the row reductions of csrc/cnn_grad.hip where their slice counts are capped; a change of a constant
    there must not put them back below the caps unnoticed."""
    g = _CgGeometry()
    sites = {(kind, B, L): cc.site_rows(cc.spec_of(kind), B, L) for kind, B, L in cc.CAP_GRAD_CASES}
    for case, rows_of in sites.items():
        assert rows_of[-1][3] == case[1] * cc.spec_of(case[0]).output_len(case[2])      # the walk ends at the features' frames
        for _, _, _, rows in rows_of:
            tc.assert_slices_tile(rows, g.nslices(rows), g.slice_chunk(rows))
            tc.assert_slices_tile(rows, g.nsplit(rows), g.dw_chunk(rows))
    # rna at the trainer's default batch: the site that reads the signal at full length is past the slice cap, the rest below both
    rna = sites[("rna", 300, 500)]
    past = [(site, ci, k, rows) for site, ci, k, rows in rna if rows > g.slice_rows * g.max_slices]
    assert [(ci, rows) for _, ci, _, rows in past] == [(1, 150000)]
    assert g.nslices(150000) == g.max_slices < -(-150000 // g.slice_rows)
    assert (g.slice_chunk(150000), _ragged_last(150000, g.max_slices, g.slice_chunk(150000))) == (293, 277)
    assert all(rows == 30000 for _, _, _, rows in rna if rows != 150000)
    # dna: every site is past both caps
    dna = sites[("dna", 330, 400)]
    assert all(rows == 132000 for _, _, _, rows in dna) and any(ci == 1 for _, ci, _, _ in dna) and any(k > 1 for _, _, k, _ in dna)
    assert g.nslices(132000) == g.max_slices < -(-132000 // g.slice_rows)
    assert g.nsplit(132000) == g.max_split < -(-132000 // g.split_rows)
    assert (g.slice_chunk(132000), _ragged_last(132000, g.max_slices, g.slice_chunk(132000))) == (258, 162)
    assert (g.dw_chunk(132000), _ragged_last(132000, g.max_split, g.dw_chunk(132000))) == (2064, 1968)


def test_row_slices_tile_every_row_count():
    """No slice of a row reduction or of cg_dw_kernel's split is empty, and the slices tile [0, rows).  (Just past the cap, as at
    131 073 rows, CG_MAX_SLICES slices of the rounded-up chunk would leave the last ones empty: cg_slices launches only those that
    hold a row.)"""
    g = _CgGeometry()
    rng = np.random.default_rng(6)
    cap = g.slice_rows * g.max_slices
    edge = [1, 2, g.slice_rows, g.slice_rows + 1, g.split_rows, g.split_rows + 1, cap - 1, cap, cap + 1, g.split_rows * g.max_split + 1,
            (1 << 24) - 1, 1 << 24]
    some = np.concatenate([rng.integers(1, 1 << 12, 1000), rng.integers(1, 1 << 18, 2000), rng.integers(1, (1 << 24) + 1, 2000)])
    for rows in edge + [int(v) for v in some]:
        tc.assert_slices_tile(rows, g.nslices(rows), g.slice_chunk(rows))
        tc.assert_slices_tile(rows, g.nsplit(rows), g.dw_chunk(rows))


def test_cap_factors_are_the_ensemble_tools():
    """The factors the GPU test holds the cap cases to are what tools/cnn_grad_accuracy.py derived on the CPU: max(4, 1.5 x the
    largest max / median of the float32 ensemble over exactly these cases)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prof = json.load(open(os.path.join(root, "profiles", "cnn_grad_accuracy.json")))
    assert sorted(prof["cap"]["cases"]) == sorted("%s B%d L%d" % c for c in cc.CAP_GRAD_CASES)
    for part, factor in (("forward", cc.CAP_FWD_FACTOR), ("gradients", cc.CAP_GRAD_FACTOR)):
        largest = max(r["max_over_median"] for case in prof["cap"]["cases"].values() for r in case[part].values())
        assert prof["cap"]["largest_max_over_median"][part] == largest
        assert prof["factor_cap"][part] == max(4.0, 1.5 * largest)
        assert abs(factor - prof["factor_cap"][part]) <= 5e-5 and factor >= 4.0, (part, factor, prof["factor_cap"][part])


# ---------------------------------------------------------------------------------------------
# the window-geometry cases: what they reach, their factors, and that the bar can tell a wrong pad
# ---------------------------------------------------------------------------------------------
def test_geometry_cases_reach_every_left_pad_of_every_strided_site():
    """GEOMETRY_GRAD_CASES with GRAD_CASES run every L mod stride, hence every left pad TF 'SAME' can give, at every strided site
    with a kernel wider than 1 of every topology.  A new topology without such cases fails here."""
    reached = {}
    for kind, _, L in cc.GRAD_CASES + cc.GEOMETRY_GRAD_CASES:
        for site, k, stride, tin in cc.site_windows(cc.spec_of(kind), L):
            if stride > 1:
                reached.setdefault((kind, site, k, stride), set()).add(tin % stride)
    strided = {kind: [(site, k, stride) for site, k, stride in cc.site_strides(cc.spec_of(kind)) if stride > 1] for kind in cc.SPECS}
    assert {kind: len(v) for kind, v in strided.items()} == {"dna": 0, "rna": 2, "rna_model2": 1, "rna_model3": 1}
    for kind, sites in strided.items():
        for site, k, stride in sites:
            assert reached[(kind, site, k, stride)] == set(range(stride)), (kind, site, sorted(reached[(kind, site, k, stride)]))
    # the left pads themselves, from same_padding at a length of each residue that is no shorter than the kernel
    lefts = {(kind, k, stride): [cnn_ref.same_padding(10 * stride + r, k, stride)[1] for r in range(stride)]
             for kind, sites in strided.items() for _, k, stride in sites if k > 1}
    assert lefts == {("rna", 13, 5): [4, 6, 5, 5, 4], ("rna_model2", 9, 5): [2, 4, 3, 3, 2], ("rna_model3", 14, 7): [3, 6, 6, 5, 5, 4, 4]}
    # and what GRAD_CASES alone reach: one pad at rna and rna_model2, two of seven residues at rna_model3
    alone = {}
    for kind, _, L in cc.GRAD_CASES:
        for site, k, stride, tin in cc.site_windows(cc.spec_of(kind), L):
            if stride > 1 and k > 1:
                alone.setdefault(kind, set()).add(tin % stride)
    assert alone == {"rna": {0}, "rna_model2": {0}, "rna_model3": {1, 3}}


def test_geometry_cases_reach_tiny_windows():
    """Windows of 1, 2 and 3 frames occur, at T = 1 with a k = 3 convolution whose outer taps both lie in the padding, and every strided
    kernel wider than 1 runs on a window shorter than itself."""
    frames = {cc.spec_of(kind).output_len(L) for kind, _, L in cc.GEOMETRY_GRAD_CASES}
    assert {1, 2, 3} <= frames
    short, one_frame_k3, all_wide = set(), set(), set()
    for kind in cc.SPECS:
        all_wide |= {(kind, k) for _, k, stride in cc.site_strides(cc.spec_of(kind)) if stride > 1 and k > 1}
    for kind, B, L in cc.GEOMETRY_GRAD_CASES:
        for site, k, stride, tin in cc.site_windows(cc.spec_of(kind), L):
            if stride > 1 and 1 < k and tin < k:
                short.add((kind, k))
            if k == 3 and tin == 1:
                one_frame_k3.add(kind)
    assert short == all_wide == {("rna", 13), ("rna_model2", 9), ("rna_model3", 14)}
    assert {"dna", "rna", "rna_model2"} <= one_frame_k3
    # about a hundred rows or more at every site (40 windows of 2 frames are the fewest)
    for kind, B, L in cc.GEOMETRY_GRAD_CASES:
        assert min(rows for _, _, _, rows in cc.site_rows(cc.spec_of(kind), B, L)) >= 80, (kind, B, L)
    assert len(cc.GEOMETRY_GRAD_CASES) == len(set(cc.GEOMETRY_GRAD_CASES)) == 21 and not set(cc.GEOMETRY_GRAD_CASES) & set(cc.GRAD_CASES)


def test_geometry_factors_are_the_ensemble_tools():
    """As test_cap_factors_are_the_ensemble_tools, for "factor_geometry" over exactly GEOMETRY_GRAD_CASES; the JSON keeps one row per
    case and part, the tensor with the largest ratio."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prof = json.load(open(os.path.join(root, "profiles", "cnn_grad_accuracy.json")))
    assert sorted(prof["geometry"]["cases"]) == sorted("%s B%d L%d" % c for c in cc.GEOMETRY_GRAD_CASES)
    for part, factor in (("forward", cc.GEOMETRY_FWD_FACTOR), ("gradients", cc.GEOMETRY_GRAD_FACTOR)):
        largest = max(case[part]["max_over_median"] for case in prof["geometry"]["cases"].values())
        assert prof["geometry"]["largest_max_over_median"][part] == largest
        assert prof["factor_geometry"][part] == max(4.0, 1.5 * largest)
        assert abs(factor - prof["factor_geometry"][part]) <= 5e-5 and factor >= 4.0, (part, factor, prof["factor_geometry"][part])


_GEOMETRY_REF = {}


def _geometry_ref(case):
    """The float64 and float32 restatements of one geometry case, computed once and shared (read only): forward, and gradients under
    the signs of the float64 pre-activations; the float32 run's own free-ReLU pre-activations besides."""
    if case not in _GEOMETRY_REF:
        import torch
        spec, w, x, g = cc.grad_case(*case)
        pre64, pre32 = {}, {}
        cnn_ref.gradients(x, spec, w, g, torch.float64, pre=pre64)
        cnn_ref.gradients(x, spec, w, g, torch.float32, pre=pre32)
        masks = {k: v > 0 for k, v in pre64.items()}
        _, g64 = cnn_ref.gradients(x, spec, w, g, torch.float64, masks=masks)
        _, g32 = cnn_ref.gradients(x, spec, w, g, torch.float32, masks=masks)
        _GEOMETRY_REF[case] = {"fwd64": cnn_ref.forward(x, spec, w, torch.float64), "fwd32": cnn_ref.forward(x, spec, w, torch.float32),
                               "pre64": pre64, "pre32": pre32, "masks": masks, "g64": g64, "g32": g32}
    return _GEOMETRY_REF[case]


@pytest.mark.parametrize("case", cc.GEOMETRY_GRAD_CASES, ids=lambda c: "%s-B%d-L%d" % c)
def test_geometry_float32_masks_stay_within_the_mask_cap(case):
    """The float32 restatement's own ReLU masks differ from the float64 signs within FLIP_TOL and FLIP_SHARE on these inputs (far
    within: shares of the order of 1e-5, |pre| / rms of 1e-7), so a HIP failure of assert_masks_legitimate here is a finding."""
    ref = _geometry_ref(case)
    cc.assert_masks_legitimate({k: v > 0 for k, v in ref["pre32"].items()}, ref["pre64"], "%s B=%d L=%d float32" % case)


@pytest.mark.parametrize("case", cc.GEOMETRY_GRAD_CASES, ids=lambda c: "%s-B%d-L%d" % c)
def test_geometry_bar_rejects_a_pad_moved_by_one(case, monkeypatch):
    """Power of the bar at these shapes: the float64 restatement with every site's padding moved one to the left (left + 1,
    right - 1, wherever right >= 1) is NOT within GEOMETRY_*_FACTOR x e32 + FLOOR of the true one: not in the features, and in
    the gradients (under the same fixed masks) in all tensors but at most one.  (The last block's conv2c_bn/offset gradient is the sum
    of the masked dfeatures, whatever the convolutions do.)"""
    import torch
    ref = _geometry_ref(case)
    spec, w, x, g = cc.grad_case(*case)
    true_padding = cnn_ref.same_padding

    def moved(width, k, stride):
        out, left, right = true_padding(width, k, stride)
        return (out, left + 1, right - 1) if right >= 1 else (out, left, right)
    monkeypatch.setattr(cnn_ref, "same_padding", moved)
    f_mut, m_mut = cnn_ref.forward(x, spec, w, torch.float64)
    _, g_mut = cnn_ref.gradients(x, spec, w, g, torch.float64, masks=ref["masks"])
    monkeypatch.undo()
    (f64, m64), (f32, m32) = ref["fwd64"], ref["fwd32"]
    assert f_mut.shape == f64.shape
    fwd = cc.row(f_mut, f64, f32, cc.GEOMETRY_FWD_FACTOR)
    assert not fwd["ok"], ("features", fwd)
    # the first wide site's own moments see it too (sites before it are untouched: k = 1 has no padding)
    first = next(site for site, k, _ in cc.site_strides(spec) if k > 1)
    seen = [cc.row(m_mut[first][i], m64[first][i], m32[first][i], cc.GEOMETRY_FWD_FACTOR)["ok"] for i in (0, 1)]
    assert not all(seen), (first, seen)
    rows = {name: cc.row(g_mut[name], ref["g64"][name], ref["g32"][name], cc.GEOMETRY_GRAD_FACTOR) for name in ref["g64"]}
    passed = [name for name, r in rows.items() if r["ok"]]
    print("%s B=%d L=%d:" % case, "%d of %d gradient tensors reject the moved pad; not: %s" % (len(rows) - len(passed), len(rows), passed))
    assert len(passed) <= 1, passed


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
