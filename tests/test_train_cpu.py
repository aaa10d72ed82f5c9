"""CPU tests of the training seam: the float64 reference against the oracle, the host-only ABI queries, the checkpoint writer and the
`finetune` command line."""
import ctypes as C
import os

import numpy as np
import pytest

import chiron_amd as ca
from chiron_amd import _lib, entry, tf_bundle, train

import rnn_ref
import train_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind", ["dna", "rna"])
def test_rnn_ref_float64_forward_equals_the_oracle(kind):
    from oracle import nn_oracle
    spec = ca.dna_default_spec() if kind == "dna" else ca.rna_default_spec()
    w = ca.synthetic_weights(spec, seed=7)
    rng = np.random.default_rng(3)
    B, T = 6, 17
    fea = rng.normal(size=(B, T, 256))
    sl = np.array([0, 1, T, 9, 4, 16])
    ref = nn_oracle.fc_head(nn_oracle.rnn_forward(fea, sl, spec.to_dict(), w), w)
    got, _, _ = rnn_ref.forward(fea, sl, spec, w)
    assert np.abs(got.numpy() - ref).max() <= 1e-12


@pytest.mark.parametrize("spec", [ca.dna_default_spec(), ca.rna_default_spec()], ids=["DNA_default", "RNA_default"])
def test_params_range_equals_the_offsets_of_the_variables(built, spec):
    names = list(spec.variables())
    sizes = [int(np.prod(s)) for s in spec.variables().values()]
    first_name = spec.lstm_scope(0, "fw") + "kernel"
    first = sum(sizes[:names.index(first_name)])
    assert names[-1] == "rnn_fnn_layer/bias_class"
    assert train.params_range(spec) == (first, sum(sizes) - first)
    off = 0
    for name, (o, shape) in train.param_layout(spec).items():
        assert o == off and tuple(spec.variables()[name]) == shape
        off += int(np.prod(shape))
    assert off == sum(sizes) - first


def test_train_sizes_grow_linearly_in_the_batch(built):
    spec = ca.dna_default_spec()
    t16, w16 = train.train_sizes(spec, 16, 400)
    t32, w32 = train.train_sizes(spec, 32, 400)
    t48, w48 = train.train_sizes(spec, 48, 400)
    assert t32 == 2 * t16 and t48 == 3 * t16        # the tape is per row
    assert t32 - t16 == t48 - t32 > 0
    assert train.train_sizes(spec, 17, 400) == (t32, w32)     # rows padded to 16
    # the workspace: per-row buffers + split-K partials that depend on the row count only through a capped slice count
    t3200, w3200 = train.train_sizes(spec, 3200, 400)
    t6400, w6400 = train.train_sizes(spec, 6400, 400)
    t9600, w9600 = train.train_sizes(spec, 9600, 400)
    assert w6400 - w3200 == w9600 - w6400 > 0 and w32 > w16


def _sizes_status(spec, batch, T):
    desc = spec.to_c()
    a, b = C.c_size_t(), C.c_size_t()
    return _lib.load().chiron_rnn_train_sizes(C.byref(desc), batch, T, C.byref(a), C.byref(b))


def test_train_sizes_refuse_bad_shapes(built):
    spec = ca.dna_default_spec()
    assert _sizes_status(spec, 16, 0) == _lib.ERR_INVALID
    assert _sizes_status(spec, 16, -3) == _lib.ERR_INVALID
    assert _sizes_status(spec, 0, 400) == _lib.ERR_INVALID
    assert _sizes_status(spec, 16, 8193) == _lib.ERR_OVERFLOW          # T > CHIRON_CTC_MAX_T
    assert _sizes_status(spec, 1 << 19, 400) == _lib.ERR_OVERFLOW      # T * batch > 2^24 rows
    assert _sizes_status(spec, (1 << 20) + 1, 1) == _lib.ERR_OVERFLOW
    # the GEMMs over the T * BP rows put their 128-row tiles on a grid's y extent: at most 65535 of them
    assert 255 * 32896 == 128 * 65535 and 32896 % 16 == 0
    assert _sizes_status(spec, 32896, 255) == _lib.OK
    assert _sizes_status(spec, 32897, 255) == _lib.ERR_OVERFLOW        # 255 * 32912 rows, still below 2^24
    assert b"row tiles" in _lib.load().chiron_last_error()
    small = ca.dna_default_spec()
    small.hidden = 64
    assert _sizes_status(small, 16, 400) == _lib.ERR_INVALID           # the kernels are built for hidden 100
    desc = small.to_c()
    a, b = C.c_size_t(), C.c_size_t()
    assert _lib.load().chiron_rnn_params_range(C.byref(desc), C.byref(a), C.byref(b)) == _lib.ERR_INVALID


# ---------------------------------------------------------------------------------------------
# the cases past the reduction caps against the kernels' own constants
# ---------------------------------------------------------------------------------------------
class _RgGeometry:
    """csrc/rnn_grad.hip's slicing of a reduction over rows, restated: rg_nsplit, rg_gemm's chunk (rounded up to the k-tile),
    the column sum's chunk (not rounded), and rg_layout's head_rows / head_wg."""
    def __init__(self):
        k = tc.kernel_constants("rnn_grad.hip", ["RG_SPLIT_ROWS", "RG_MAX_SPLIT", "RG_HEAD_WG", "RG_HEAD_ROWS", "GK"])
        self.split_rows, self.max_split, self.head_wg_max, self.head_rows_min, self.gk = (
            k["RG_SPLIT_ROWS"], k["RG_MAX_SPLIT"], k["RG_HEAD_WG"], k["RG_HEAD_ROWS"], k["GK"])

    def nsplit(self, R):
        return min(max(-(-R // self.split_rows), 1), self.max_split)

    def gemm_chunk(self, R):
        return -(-(-(-R // self.nsplit(R))) // self.gk) * self.gk

    def colsum_chunk(self, M):
        return -(-M // self.nsplit(M))

    def head(self, M):
        rows = max(-(-M // self.head_wg_max), self.head_rows_min)
        return rows, -(-M // rows)


def test_cap_cases_lie_past_the_caps_of_the_kernels_constants():
    """CAP_CASES exist to run the reductions of csrc/rnn_grad.hip where their slice counts are capped; a change of a constant there
    must not put them back below the caps unnoticed."""
    g = _RgGeometry()
    whats = set()
    for kind, B, T, what in tc.CAP_CASES:
        whats.add(what)
        BP = -(-B // 16) * 16
        M = T * BP
        head_rows, head_wg = g.head(M)
        tc.assert_slices_tile(M, head_wg, head_rows)
        # the head cap binds: more rows per workgroup than the least, no multiple of the 16-row tiles or of a frame, padding rows present
        assert M > g.head_wg_max * g.head_rows_min and head_rows > g.head_rows_min and head_wg == g.head_wg_max
        assert B < BP and head_rows % BP != 0
        if what == "head":
            assert head_rows % 16 != 0
            assert g.nsplit(M) < g.max_split            # the split-K cap is the other cases' business
            assert (M, head_rows) == (33024, 129)
        for R in (M, M - BP):                           # dWx and db reduce over M rows, dWh over M - BP
            tc.assert_slices_tile(R, g.nsplit(R), g.gemm_chunk(R))
            tc.assert_slices_tile(R, g.nsplit(R), g.colsum_chunk(R))
        if what == "split":
            n = g.nsplit(M)
            assert n == g.max_split and -(-M // g.split_rows) > g.max_split and g.nsplit(M - BP) == g.max_split
            assert g.gemm_chunk(M) > g.split_rows and g.colsum_chunk(M) > g.split_rows      # the slices grow instead of their count
            gemm, colsum = tc.slices(M, n, g.gemm_chunk(M)), tc.slices(M, n, g.colsum_chunk(M))
            assert g.gemm_chunk(M) != g.colsum_chunk(M)                 # the two disagree about the slice borders
            for sl, chunk in ((gemm, g.gemm_chunk(M)), (colsum, g.colsum_chunk(M)), (tc.slices(M, head_wg, head_rows), head_rows)):
                assert 0 < sl[-1][1] - sl[-1][0] < chunk                # a ragged last slice
            assert (M, g.gemm_chunk(M), gemm[-1][1] - gemm[-1][0], g.colsum_chunk(M), head_rows) == (133472, 2096, 1424, 2086, 522)
            assert (M - BP, g.gemm_chunk(M - BP)) == (132096, 2064) and 64 * 2064 == M - BP     # dWh: the slices fit exactly
    assert whats == {"head", "split"}


def test_row_slices_tile_every_row_count():
    """For row counts up to 2^24, more than the sizes call admits: no slice of the split-K GEMMs, the column sum or the head backward is
    empty, and the slices tile [0, rows)."""
    g = _RgGeometry()
    rng = np.random.default_rng(5)
    edge = [1, 2, 15, 16, 17, g.split_rows, g.split_rows + 1, g.split_rows * g.max_split - 1, g.split_rows * g.max_split,
            g.split_rows * g.max_split + 1, g.head_wg_max * g.head_rows_min, g.head_wg_max * g.head_rows_min + 1, (1 << 24) - 1, 1 << 24]
    some = np.concatenate([rng.integers(1, 1 << 12, 1000), rng.integers(1, 1 << 18, 2000), rng.integers(1, (1 << 24) + 1, 2000)])
    for rows in edge + [int(v) for v in some]:
        tc.assert_slices_tile(rows, g.nsplit(rows), g.gemm_chunk(rows))
        tc.assert_slices_tile(rows, g.nsplit(rows), g.colsum_chunk(rows))
        head_rows, head_wg = g.head(rows)
        tc.assert_slices_tile(rows, head_wg, head_rows)
        assert head_wg <= g.head_wg_max


# ---------------------------------------------------------------------------------------------
# the tiny and odd frame counts
# ---------------------------------------------------------------------------------------------
def test_geometry_cases_reach_tiny_and_odd_frame_counts():
    """GEOMETRY_CASES run both recurrent wirings at T = 1, 2 and 3 and at frame counts that are multiples of nothing in the kernels;
    their lengths cover 0, 1 and T in every case, which ragged_seq_len cannot draw at T = 1."""
    g = _RgGeometry()
    for kind in ("dna-stack", "rna-multi"):
        frames = sorted(T for k, _, T in tc.GEOMETRY_CASES if k == kind)
        assert frames == [1, 2, 3, 17, 33]
        assert sum(1 for T in frames if T > 3 and T % 2 and T % g.gk) >= 2
    assert len(tc.GEOMETRY_CASES) == len(set(tc.GEOMETRY_CASES)) == 10
    for kind, B, T in tc.GEOMETRY_CASES:
        spec, w, fea, sl, dl = tc.geometry_case(kind, B, T)
        assert fea.shape == (B, T, 256) and dl.shape == (B, T, 5) and sl.shape == (B,) and sl.dtype == np.int32
        assert (fea >= 0).all() and 0.3 < (fea == 0).mean() < 0.7          # post-ReLU-like
        assert tuple(sl[:3]) == (0, 1, T) and sl.min() >= 0 and sl.max() <= T
        assert B * T >= 96                                                  # about a hundred rows or more
        spec2, _, fea2, sl2, dl2 = tc.geometry_case(kind, B, T)           # seeded by the case alone
        assert fea2.tobytes() == fea.tobytes() and sl2.tobytes() == sl.tobytes() and dl2.tobytes() == dl.tobytes()
    with pytest.raises(ValueError):
        tc.ragged_seq_len(5, 1, np.random.default_rng(0))
    sl = tc.geometry_seq_len(2000, 3, np.random.default_rng(0))
    assert set(sl.tolist()) == {0, 1, 2, 3}


@pytest.mark.parametrize("kind", ["dna-stack", "rna-multi"])
def test_reference_at_one_frame_has_no_recurrent_gradient(kind):
    """What the GPU test asserts of the kernels at T = 1 holds of the float64 reference: no step has a predecessor, so the recurrent
    rows of every lstm kernel's gradient are exactly 0 and the input rows are not."""
    import torch
    spec, w, fea, sl, dl = tc.geometry_case(kind, 101, 1)
    _, g64, dx64 = rnn_ref.gradients(fea, sl, spec, w, dl, torch.float64)
    kernels = [name for name in g64 if name.endswith("lstm_cell/kernel")]
    assert len(kernels) == 2 * spec.rnn_layers
    for name in kernels:
        in_w = g64[name].shape[0] - spec.hidden
        assert g64[name][:in_w].any() and not g64[name][in_w:].any(), name
    assert not dx64[sl == 0].any() and dx64[sl == 1].any()


def test_write_bundle_round_trip_and_crc(built, tmp_path):
    rng = np.random.default_rng(2)
    tensors = {"a/%03d/w" % i: rng.normal(size=(3, i + 1)).astype(np.float32) for i in range(90)}
    tensors["global_step"] = np.asarray(77, dtype=np.int64)
    tensors["flags"] = np.arange(5, dtype=np.int32)
    prefix = str(tmp_path / "x.ckpt-77")
    tf_bundle.write_bundle(prefix, tensors)
    entries = tf_bundle.read_index(prefix + ".index")
    assert sorted(entries) == sorted(tensors)
    got = tf_bundle.read_tensors(prefix, entries, list(tensors))
    for k, v in tensors.items():
        assert got[k].dtype == v.dtype and got[k].shape == v.shape and got[k].tobytes() == v.tobytes(), k
    data = prefix + ".data-00000-of-00001"
    raw = bytearray(open(data, "rb").read())
    raw[len(raw) // 2] ^= 0x10
    open(data, "wb").write(bytes(raw))
    with pytest.raises(IOError, match="checksum mismatch"):
        tf_bundle.read_tensors(prefix, entries, list(tensors))


@pytest.mark.parametrize("spec", [ca.dna_default_spec(), ca.rna_default_spec()], ids=["DNA_default", "RNA_default"])
def test_saved_model_loads_through_load_model(built, tmp_path, spec):
    w = ca.synthetic_weights(spec, seed=11)
    out = str(tmp_path / "model")
    train.save_model(out, spec, w, 123, train.config_for(spec, None, "Adam", 2.0))
    assert tf_bundle.latest_checkpoint(out).endswith("final.ckpt-123")
    spec2, w2, config = ca.load_model(out)
    assert spec2.to_dict() == spec.to_dict() and config["opt_method"] == "Adam"
    canon = spec.canonical_weights(w)
    assert list(w2) == list(canon)
    for k in canon:
        assert np.asarray(w2[k]).tobytes() == np.asarray(canon[k], dtype=np.float32).tobytes(), k


def test_finetune_command_line_defaults():
    a = entry.build_parser().parse_args(["finetune", "-i", "in", "-o", "out"])
    assert a.func is entry.finetune
    assert (a.sequence_len, a.batch_size, a.step_rate, a.max_steps, a.segments_num) == (400, 300, 4e-3, 10000, None)
    assert (a.gradient_clip, a.fl_gamma, a.opt_method, a.sig_norm, a.device, a.validation) == (None, 0.0, "Adam", "none", 0, None)
    assert a.synthetic_weights is False and isinstance(a.seed, int)
    assert a.model.endswith(os.path.join("model", "DNA_default"))
    b = entry.build_parser().parse_args(["finetune", "-i", "in", "-o", "out", "-v", "val", "-s", "300", "-b", "16", "-t", "1e-3", "-x", "40",
                                         "-n", "500", "--gradient_clip", "5", "--fl_gamma", "2", "--opt_method", "Momentum",
                                         "--sig_norm", "median", "--device", "1", "--seed", "3", "--synthetic-weights"])
    assert (b.validation, b.sequence_len, b.batch_size, b.step_rate, b.max_steps, b.segments_num) == ("val", 300, 16, 1e-3, 40, 500)
    assert (b.gradient_clip, b.fl_gamma, b.opt_method, b.sig_norm, b.device, b.seed, b.synthetic_weights) == \
        (5.0, 2.0, "Momentum", "median", 1, 3, True)
