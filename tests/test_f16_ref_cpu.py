"""CPU: the quantised restatement of the f16 engines (tests/f16_ref.py), its committed bar (profiles/f16_ref_accuracy.json) and the
cases of tests/test_gpu_f16_ref.py -- everything about that test that can be wrong without a GPU.

  * with identity roundings the three stages composed ARE the oracle (1e-12, all four topologies, ragged rows);
  * hi + lo halves reproduce a weight to 2^-22;
  * the committed factors are what the tool computes, and the committed case list is the test's;
  * the bar rejects a deliberately wrong reference at the shapes the GPU test runs (f16_cases.REQUIRED: a lost shift at the first
    and at the last block and of a whole middle site, (b), (c), (d)), and what it cannot resolve (one channel's lost shift in the
    middle of the network on the short RNA cases, (e) .. (g)) is on record;
  * every case sits on the kernel edge it claims, read from the kernels' own constants."""
import numpy as np
import pytest

import chiron_amd as ca
from oracle import nn_oracle

import f16_cases as fc
import f16_ref
from train_cases import kernel_constants


@pytest.mark.parametrize("topology,L", [("dna", 37), ("rna", 158), ("rna_model2", 66), ("rna_model3", 71)])
def test_identity_roundings_are_the_oracle(topology, L):
    spec = fc.specs()[topology]
    sd = spec.to_dict()
    w = ca.synthetic_weights(spec, seed=fc.WEIGHT_SEED)
    x, sl, T = fc.ragged(spec, L, 6, seed=11)
    assert {0, 1, T} <= set(sl.tolist()) and ((sl > 1) & (sl < T)).any()
    ref, _, fea, lasth = nn_oracle.inference(x.astype(np.float64), sl, sd, w, return_all=True)
    f = f16_ref.cnn(x, sd, w, mode=None, aq=f16_ref.ident, fold=np.float64)
    h = f16_ref.rnn(f, sl, sd, w, mode=None, z16=False, hq=f16_ref.ident, oq=f16_ref.ident, fold=np.float64)
    for got, want in ((f, fea), (h, lasth), (f16_ref.head(h, w), ref)):
        assert got.dtype == np.float64 and got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    # the lifted form of block 1 with identity roundings is the same network
    f2 = f16_ref.cnn(x, sd, w, mode=None, table=False, aq=f16_ref.ident, fold=np.float64)
    assert np.abs(f2 - fea).max() <= 1e-12 * np.abs(fea).max()


def test_the_roundings_are_where_the_docstring_says():
    """each rounding moves the result, halves come out where halves are stored, and the wide last layer is not halves"""
    spec = fc.specs()["dna"]
    sd, w = spec.to_dict(), ca.synthetic_weights(spec, seed=fc.WEIGHT_SEED)
    x, sl, T = fc.ragged(spec, 24, 5, seed=12)
    fea = f16_ref.cnn(x, sd, w)
    assert np.array_equal(fea, f16_ref.f16(fea))
    assert not np.array_equal(fea, f16_ref.cnn(x, sd, w, table=False))            # conv2a stored, conv2b's filter rounded
    assert not np.array_equal(fea, f16_ref.cnn(x, sd, w, mode="fp16-w2"))
    h = f16_ref.rnn(fea, sl, sd, w)
    assert not np.array_equal(h, f16_ref.f16(h))                                   # the last layer leaves as fp32
    h16 = f16_ref.rnn(fea, sl, sd, w, lasth16=True)
    assert np.array_equal(h16, f16_ref.f16(h)) and np.array_equal(h16, f16_ref.f16(h16))
    assert not np.array_equal(h, f16_ref.rnn(fea, sl, sd, w, z16=False))
    assert not np.array_equal(h, f16_ref.rnn(fea, sl, sd, w, z16=[True, False, True]))
    mask = fc.valid_mask(sl, T)
    assert np.all(h[~mask] == 0) and np.abs(f16_ref.head(h, w)[~mask] - f16_ref.head_constant(w, spec.hidden)).max() < 1e-14


def test_hi_plus_lo_halves_reproduce_a_weight_to_2_to_the_minus_22():
    """hi + lo is W to 2^-22 relative wherever halves can hold it: from |W| = 2^-3 on.  Below, lo = f16(W - hi) is a SUBNORMAL half
    (|W - hi| <= 2^-15 < 2^-14) with the fixed quantum 2^-24, so the error is 2^-25 absolute -- WeightPacker::gemm's fp16-w2 branch has no
    row scaling (the fp32-split branch has) -- which is what the reference reproduces."""
    rng = np.random.default_rng(3)
    spec = fc.specs()["dna"]
    w = ca.synthetic_weights(spec, seed=fc.WEIGHT_SEED)
    folded = f16_ref.folded(w, "res_layer2/branch2/conv2b", True)[0]
    kern = np.asarray(w["BDLSTM_rnn/cell_1/bidirectional_rnn/fw/lstm_cell/kernel"], dtype=np.float32)
    wide = (rng.normal(size=4096) * np.exp2(rng.integers(-10, 11, size=4096))).astype(np.float32)
    for v in (folded, kern, wide):
        hi, lo = f16_ref.hilo(v)
        assert hi.dtype == lo.dtype == np.float16
        got = f16_ref.weight_rounding("fp16-w2")(v)
        assert np.array_equal(got, hi.astype(np.float64) + lo.astype(np.float64))
        err, mag = np.abs(got - v), np.abs(v.astype(np.float64))
        big = mag >= 2.0 ** -3
        assert big.any() and (~big).any()
        assert (err[big] <= 2.0 ** -22 * mag[big]).all()
        assert (err[~big] <= 2.0 ** -25).all()
        one = f16_ref.weight_rounding("fp16")(v)
        normal = mag >= 2.0 ** -14
        assert (np.abs(one - v)[normal] <= 2.0 ** -11 * mag[normal]).all() and np.abs(one - v).max() > 100 * err.max()


def test_committed_factors_are_what_the_tool_computes():
    d = fc.committed()
    assert d["case_list"] == [fc.case_id(c) for c in fc.CASES] == list(d["cases"])
    assert d["floor"] == fc.FLOOR and d["draws"] == 8
    largest, factor = fc.factors_from(d["cases"])
    assert factor == d["factor"] and largest == d["largest_max_over_median"]
    assert d["factor"]["head"] == {"l2": fc.HEAD_FACTOR, "channel": fc.HEAD_FACTOR}
    for stage in ("cnn", "rnn", "e2e"):
        for m in ("l2", "channel"):
            assert d["factor"][stage][m] == max(4.0, 1.5 * d["largest_max_over_median"][stage][m])
    for c in fc.CASES:
        assert set(d["cases"][fc.case_id(c)]) == set(fc.case_arithmetics(c)), fc.case_id(c)
    c = fc.CASES[2]                                            # one small case recomputed
    again = fc.ensemble(c, d["draws"])
    for key, row in again.items():
        for m in ("l2", "channel"):
            for leaf, v in row[m].items():
                assert v == pytest.approx(d["cases"][fc.case_id(c)][key][m][leaf], rel=1e-6, abs=1e-12), (key, m, leaf)


@pytest.mark.parametrize("c", fc.CASES, ids=[fc.case_id(c) for c in fc.CASES])
def test_the_bar_rejects_a_wrong_reference(c):
    """every required row of f16_cases.MUTATIONS at this case's shapes under the committed factors; the others as recorded"""
    d = fc.committed()
    got = fc.sensitivity(c, d["factor"], sorted(fc.MUTATIONS))
    for name in fc.REQUIRED:
        if name in got:
            assert got[name]["rejected"], (name, fc.MUTATIONS[name][1], got[name])
    assert {k: v["rejected"] for k, v in got.items()} == {k: v["rejected"] for k, v in d["sensitivity"][fc.case_id(c)].items()}


def test_every_required_mutation_is_exercised():
    d = fc.committed()
    for name in fc.REQUIRED:
        n = sum(1 for rows in d["sensitivity"].values() if name in rows)
        assert n >= len(fc.CASES) - 1, (name, n)               # (c) and (d) need a second step / a ragged row: not at T = 1
    assert set(fc.REQUIRED) >= {"a", "a-last", "a-all", "b", "c", "d"}


def test_cases_sit_on_the_edges_they_claim():
    k = kernel_constants("stream16.hip", ["S_ROWS", "S_C"])
    s3_valid = k["S_ROWS"] - 2                                 # S3_VALID: output rows per tile of the 1 x 3 kernel
    assert "constexpr int S3_VALID = S_ROWS - 2;" in open(fc.ROOT + "/chiron_amd/csrc/stream16.hip").read()
    assert k["S_C"] == 256 and fc.STREAM3_MIN_T == k["S_ROWS"]
    specs = fc.specs()
    by = {}
    for c in fc.CASES:
        by.setdefault(c[0], []).append(c)
    dna_T = [c[1] for c in by["dna"]]
    assert dna_T == [1, 2, 31, 32, 33, 48, 100]
    # below / at / above stream16's 1 x 3 minimum (launch_stream16: taps && T_out < S_ROWS -> the tiled GEMM)
    assert {k["S_ROWS"] - 1, k["S_ROWS"], k["S_ROWS"] + 1} <= set(dna_T) and min(dna_T) < 3
    for c in by["dna"]:
        rows = c[1] * c[2]
        assert rows % s3_valid, c                              # partial last 30-row tile of the 1 x 3 kernel
        assert rows % k["S_ROWS"] or c[1] % k["S_ROWS"] == 0, c    # partial last 32-row tile (T = 32 cannot have one)
    assert sum(1 for c in by["dna"] if c[3] > c[2]) >= 2       # inert rows
    # every left pad of the strided table conv and of the lifted form, at T = 32
    rna = specs["rna"]
    stride, kk = rna.blocks[0]["stride"], rna.blocks[0]["k"]
    short = [c for c in by["rna"] if rna.output_len(c[1]) == k["S_ROWS"]]
    assert {c[1] % stride for c in short} == set(range(stride))
    assert len({nn_oracle.same_padding(c[1], kk, stride)[1:] for c in short}) == stride
    assert all("no-pwl" in c[4] for c in short) and any("no-pwl" in c[4] for c in by["dna"])
    assert {c[1] for c in by["rna_model3"]} == {694, 700} and {c[1] for c in by["rna_model2"]} == {486}
    # the recurrence forms: the 16-row group sizes of launch_lstm
    forms = [c for c in fc.CASES if "wide-unfused" in c[4]]
    assert {c[:3] for c in forms} == {("dna", 48, 37), ("rna", 500, 20)}
    r = fc.launch_rules()                                      # the numbers of launch_lstm / engine.hip, read from the source
    assert r["wide_rows"] == r["fused_rows"] == r["pair_rows"] == r["pad"]
    for c in forms:
        assert set(fc._RNN_FORMS[1:] + fc._W2_FORMS) <= set(c[4]) and "default" in c[4]
        pair = fc.engine_batch(c, "fused-pair")
        assert pair % (r["pair_rows"] * r["pair_groups"]) == 0 and 0 <= pair - c[2] < r["pair_rows"] * r["pair_groups"]
        pad = lambda n: -(-n // r["pad"]) * r["pad"]
        bp = pad(fc.engine_batch(c, "wide-unfused"))
        assert (bp // r["wide_rows"]) * 2 >= fc.CUS > ((bp - r["pad"]) // r["wide_rows"]) * 2    # the smallest batch that fills the compute units
        for form in ("default", "narrow", "lasth16", "fused"):
            small = pad(fc.engine_batch(c, form))
            assert (small // r["wide_rows"]) * 2 < fc.CUS      # lstm16_kernel, not lstm16w_kernel
            assert (small // r["fused_rows"]) * 2 < r["fused_min"]     # fused only where CHIRON_LSTM16_FUSED_MIN asks for it
        assert pad(c[2]) > r["pad"]                            # more than one 16-row group
    spec, w, x, sl, T = fc.case_inputs(forms[0])
    assert (sl[:16] < T / 4).all() and sl[16] == T             # a whole 16-row group finishes early
    for c in fc.CASES:
        spec, w, x, sl, T = fc.case_inputs(c)
        assert list(sl[:3]) == [T, 1, 0][:len(sl)] or c is forms[0]
        assert {0, 1, T} <= set(sl.tolist())
        assert x.shape == (c[2], c[1]) and T == spec.output_len(c[1])
    assert [c[0] for c in fc.CASES if c[5]] == ["dna", "rna", "rna_model3", "rna_model2"]     # one end-to-end row per topology


def test_arithmetic_of_every_form():
    dna, rna = fc.specs()["dna"], fc.specs()["rna"]
    assert fc.arithmetic(dna, "default") == {"mode": "fp16", "table": True, "z16": [True] * 3, "lasth16": False}
    assert fc.arithmetic(dna, "fused")["z16"] == [False] * 3 and fc.arithmetic(rna, "fused-pair")["z16"] == [False, True, True]
    assert fc.arithmetic(dna, "w2")["z16"] == [False] * 3 and fc.arithmetic(rna, "w2-zf16")["z16"] == [True] * 3
    assert fc.arithmetic(rna, "no-pwl")["table"] is False and fc.arithmetic(dna, "lasth16")["lasth16"] is True
    assert fc.arithmetic(dna, "wide-unfused") == fc.arithmetic(dna, "narrow") == fc.arithmetic(dna, "no-stream16") == fc.arithmetic(dna, "default")
    assert fc.arithmetic(fc.specs()["rna_model2"], "default")["table"] is False        # a stem: no one-channel block
