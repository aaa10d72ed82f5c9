"""CPU: the float32 yardstick of the fp32 engine's stages (tests/fp32_ref.py), its committed bar (profiles/fp32_stage_accuracy.json)
and the cases of tests/test_gpu_fp32_ref.py -- everything about that test that can be wrong without a GPU.

  * in float64 the stages composed ARE the oracle, the gate formula of lstm.hip is sigmoid / tanh, and with exact transformed
    filters both Winograd restatements ARE the direct convolution (1e-12, all four topologies, ragged rows);
  * the transformed filters are rounded to float32 once, and that is visible;
  * the committed factors are what the tool computes, the committed case list is the test's, one case is recomputed;
  * the bar rejects every required defect (fp32_cases.REQUIRED: an operand at 16 significant bits at one conv site, in one
    projection, in one W_hh, in 32 output channels; the f16 suite's structural mutations) at every case it applies to, what it is not
    required to resolve is on record, and so is what the same defects move the logits by (below the suite's older 1e-4 bar);
  * every case keeps about a hundred distinct valid (frame, row) pairs at every stage and sits on the kernel edge it claims, read
    from the kernels' own constants and launch rules."""
import numpy as np
import pytest

import chiron_amd as ca
from oracle import nn_oracle

import f16_cases as fc
import fp32_cases as pc
import fp32_ref
from train_cases import kernel_constants

_IDS = [pc.case_id(c) for c in pc.CASES]


@pytest.mark.parametrize("topology,L", [("dna", 36), ("rna", 158), ("rna_model2", 60), ("rna_model3", 84)])
def test_float64_restatement_is_the_oracle_in_every_conv2b_form(topology, L):
    spec = pc.specs()[topology]
    sd = spec.to_dict()
    w = ca.synthetic_weights(spec, seed=pc.WEIGHT_SEED)
    x, sl, T = pc.ragged(spec, L, 6, seed=11)
    assert T % 4 == 0 and {0, 1, T} <= set(sl.tolist()) and ((sl > 1) & (sl < T)).any()
    ref, _, fea, lasth = nn_oracle.inference(x.astype(np.float64), sl, sd, w, return_all=True)
    close = lambda got, want: got.dtype == np.float64 and got.shape == want.shape and np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    for form in fp32_ref.CONV2B_FORMS:                         # exact U: the transforms re-associate the sum over taps, nothing else
        assert close(fp32_ref.cnn(x, sd, w, conv2b=form, fold=np.float64, exact_u=True), fea), form
    w64 = {k: np.asarray(v, dtype=np.float64) for k, v in w.items()}
    h = fea
    for layer in range(spec.rnn_layers):
        want = nn_oracle.rnn_layer_forward(h, sl, sd, w64, layer)
        for gates in ("libm", "engine"):                       # lstm.hip's exp2 / rcp formula IS sigmoid / tanh in float64
            assert close(fp32_ref.rnn_layer(h, sl, sd, w, layer, gates=gates, fold=np.float64), want), (layer, gates)
        h = want
    assert close(h, lasth) and close(fp32_ref.head(h, w), ref)
    # the engine's operands: BN folded in float32, U rounded to float32 once -- close to the oracle, and not the oracle
    for form in ("f2", "f4"):
        exact = fp32_ref.cnn(x, sd, w, conv2b=form, exact_u=True)
        rounded = fp32_ref.cnn(x, sd, w, conv2b=form)
        d = np.abs(rounded - exact).max() / np.abs(exact).max()
        assert 0 < d < 1e-5, (form, d)
    fea32, layers32, logits32 = fp32_ref.compose(x, sl, sd, w, np.float32, "f2")
    assert fea32.dtype == logits32.dtype == np.float32 and all(v.dtype == np.float32 for v in layers32)
    mask = pc.valid_mask(sl, T)
    assert all(np.all(v[~mask] == 0) for v in layers32)
    assert 0 < np.abs(logits32 - ref)[mask].max() < 1e-4


def test_sixteen_significant_bits():
    rng = np.random.default_rng(5)
    v = (rng.normal(size=4096) * np.exp2(rng.integers(-20, 21, size=4096))).astype(np.float32)
    r = fp32_ref.round_bits(v)
    assert r.dtype == np.float32 and np.array_equal(fp32_ref.round_bits(r), r)
    # 16 significant bits as bf16 has 8: half a unit of the 16th bit is at most 2^-16 of the value
    assert (np.abs(r.astype(np.float64) - v) <= 2.0 ** -16 * np.abs(v)).all() and np.abs(r.astype(np.float64) / v - 1).max() > 2.0 ** -18
    m, _ = np.frexp(r.astype(np.float64))
    assert np.array_equal(m * 2.0 ** 16, np.round(m * 2.0 ** 16))


def test_committed_factors_are_what_the_tool_computes():
    d = pc.committed()
    assert d["case_list"] == _IDS == list(d["cases"]) and len(set(_IDS)) == len(_IDS)
    assert d["floor"] == pc.FLOOR and d["draws"] == pc.DRAWS >= 8 and d["gates"] == pc.GATES and d["weight_seed"] == pc.WEIGHT_SEED
    largest, factor = pc.factors_from(d["cases"])
    assert factor == d["factor"] and largest == d["largest_max_over_median"]
    assert d["factor"]["head"] == {"l2": pc.HEAD_FACTOR, "channel": pc.HEAD_FACTOR}
    for stage in ("cnn", "rnn"):
        for m in ("l2", "channel"):
            assert d["factor"][stage][m] == max(4.0, 1.5 * d["largest_max_over_median"][stage][m])
    for c in pc.CASES:
        assert list(d["cases"][pc.case_id(c)]) == pc.stages(pc.specs()[c[0]])[:-1], pc.case_id(c)
        assert d["conv2b_form"][pc.case_id(c)] == pc.conv2b_form(c)
    c = pc.CASES[_IDS.index("dna-L12-B17-f4")]                 # one small case recomputed, in its own (forced F(4,3)) form
    again = pc.ensemble(c, d["draws"])
    for stage, row in again.items():
        assert row["rows"] == d["cases"][pc.case_id(c)][stage]["rows"]
        for m in ("l2", "channel"):
            for leaf, v in row[m].items():
                assert v == pytest.approx(d["cases"][pc.case_id(c)][stage][m][leaf], rel=1e-6, abs=1e-12), (stage, m, leaf)


@pytest.mark.parametrize("c", pc.CASES, ids=_IDS)
def test_the_bar_rejects_every_required_defect(c):
    """every required row of fp32_cases.DEFECTS at this case's shapes under the committed factors; the others as recorded"""
    d = pc.committed()
    got = pc.sensitivity(c, d["factor"], sorted(pc.DEFECTS))
    want = d["sensitivity"][pc.case_id(c)]
    for name in pc.REQUIRED:
        if name in got:
            assert got[name]["rejected"], (name, pc.DEFECTS[name][1], got[name])
    assert {k: v["rejected"] for k, v in got.items()} == {k: v["rejected"] for k, v in want.items()}
    for name, v in got.items():
        if name in pc.LOGIT_RECORD:
            assert v["max_logit_deviation"] == pytest.approx(want[name]["max_logit_deviation"], rel=1e-6, abs=1e-15), name
    # p4 is the row the channel metric is there for: the tensor's L2 error alone would let it pass the factor
    if "p4" in got:
        assert got["p4"]["channel_over_e32"] > d["factor"]["cnn"]["channel"] and got["p4"]["channel_over_e32"] > got["p4"]["l2_over_e32"]


def test_every_required_defect_is_exercised_and_the_reason_stays_on_file():
    d = pc.committed()
    assert list(d["required"]) == list(pc.REQUIRED) and set(pc.REQUIRED) >= {"p1-mid", "p1-last", "p2-l0", "p2-l1", "p3", "p4", "a", "a-last", "b", "c", "d"}
    assert set(pc.LOGIT_RECORD) == {n for n in pc.REQUIRED if n.startswith("p")}
    for name in pc.REQUIRED:
        n = sum(1 for rows in d["sensitivity"].values() if name in rows)
        # everywhere, but: p3 / (c) / (d) not at T = 1, p3 not at T = 2 (fp32_cases.P3_NOTE), (b) / (d) not on the one-window case
        assert n >= len(pc.CASES) - 2, (name, n)
        assert all(rows[name]["rejected"] for rows in d["sensitivity"].values() if name in rows), name
    for name in ("k-tail", "wx-tail"):                         # report only: recorded wherever they apply
        assert sum(1 for rows in d["sensitivity"].values() if name in rows) >= 8
    # why this suite exists: the operand defects the stage bar rejects move the logits by less than the 1e-4 bar of the older tests
    dev = d["largest_logit_deviation"]
    assert set(dev) == set(pc.LOGIT_RECORD)
    below = [n for n in pc.LOGIT_RECORD if dev[n] < 1e-4]
    assert set(below) >= {"p1-mid", "p1-last", "p2-l1", "p3", "p4"}, dev
    per_case = [rows[n]["max_logit_deviation"] for rows in d["sensitivity"].values() for n in pc.LOGIT_RECORD if n in rows]
    assert sum(1 for v in per_case if v < 1e-4) >= len(per_case) - 2 and min(per_case) > 0


def test_cases_keep_about_a_hundred_distinct_valid_pairs_at_every_stage():
    d = pc.committed()
    for c in pc.CASES:
        spec, w, x, sl, T = pc.case_inputs(c)
        assert x.shape == (c[2], c[1]) and T == spec.output_len(c[1])
        assert int(pc.valid_mask(sl, T).sum()) >= pc.MIN_ROWS, pc.case_id(c)
        for stage, row in d["cases"][pc.case_id(c)].items():
            assert row["rows"] >= pc.MIN_ROWS, (pc.case_id(c), stage, row["rows"])
        assert {0, T} <= set(sl.tolist()) or c[2] == 1
        assert c[2] == 1 or 1 in sl.tolist()


def test_the_case_table_reaches_every_form():
    specs = pc.specs()
    assert pc.wino_rule()["f4_min_t"] == pc.F4_MIN_T
    wino = kernel_constants("wino.hip", ["WP", "Q4"])
    by = {cid: c for cid, c in zip(_IDS, pc.CASES)}
    T = lambda c: specs[c[0]].output_len(c[1])
    form = {cid: pc.conv2b_form(c) for cid, c in by.items()}
    # conv2b: direct at an odd length, F(2,3) with T % 4 == 2 and a tile boundary inside a window, F(4,3) at its threshold with a
    # partial tile, every forced form
    assert form["dna-L33-B7"] == "direct" and T(by["dna-L33-B7"]) % 2 == 1
    for cid in ("dna-L30-B13", "dna-L130-B3"):
        c = by[cid]
        assert form[cid] == "f2" and T(c) % 4 == 2 and wino["WP"] < c[2] * T(c) // 2 < 2 * wino["WP"] and wino["WP"] % (T(c) // 2)
    c = by["dna-L256-B3"]
    assert form["dna-L256-B3"] == "f4" and T(c) == pc.F4_MIN_T and 2 * c[2] * T(c) // 4 == 3 * wino["Q4"]
    c = by["dna-L12-B17-f4"]
    assert form["dna-L12-B17-f4"] == "f4" and c[3] == "CHIRON_WINOGRAD_F4" and T(c) // 4 == 3 and T(c) < pc.F4_MIN_T
    assert form["dna-L256-B3-f2"] == "f2" and form["dna-L256-B3-nowino"] == "direct" and T(by["dna-L256-B3-nowino"]) % 2 == 0
    assert form["dna-L1-B300"] == "direct" and T(by["dna-L1-B300"]) == 1 and form["dna-L2-B110"] == "f2" and T(by["dna-L2-B110"]) == 2
    # every left pad of the strided first block at T = 32, as the table and lifted; RNA_default's own window; both stems
    rna = specs["rna"]
    stride, kk = rna.blocks[0]["stride"], rna.blocks[0]["k"]
    for switch in (None, "CHIRON_NO_PWL"):
        short = [c for c in pc.CASES if c[0] == "rna" and c[3] == switch and T(c) == 32]
        assert {c[1] % stride for c in short} == set(range(stride)) and all(5 <= c[2] <= 9 for c in short)
        assert len({nn_oracle.same_padding(c[1], kk, stride)[1:] for c in short}) == stride
    assert by["rna-L500-B16"][3] is None and T(by["rna-L500-B16"]) == 100
    assert {c[1] % 7 for c in pc.CASES if c[0] == "rna_model3"} == {694 % 7, 0} and [c[1] for c in pc.CASES if c[0] == "rna_model2"] == [486]
    assert all(3 <= c[2] <= 4 for c in pc.CASES if c[0].startswith("rna_model"))
    # every CNN row under the streaming 1 x 1 kernels and on the tiled GEMM
    cnn_rows = [c for c in pc.CASES if c[4] == pc._CNN]
    assert len(cnn_rows) == 23 and all(set(pc.form_env(c, "no-stream32")) == {"CHIRON_NO_STREAM32"} | ({c[3]} if c[3] else set()) for c in cnn_rows)
    # the recurrence forms and the projections: launch_lstm's rules, read from the source
    r = pc.launch_rules()
    assert r["default_form"] == 2 and r["wide_needs_unpaired"] and r["pairs"] == "std::min(groups / 2, n_cu / p.ndir)"
    assert pc.FORMS["wide0"] == {"CHIRON_LSTM_WIDE": "0"} and pc.FORMS["wide1"] == {"CHIRON_LSTM_WIDE": "1"}
    assert pc.FORMS["pair"]["CHIRON_LSTM_PAIR"] == "1" and pc.FORMS["pair"]["CHIRON_LSTM_WIDE"] == "0"       # the 4-row form, paired
    rec = [c for c in pc.CASES if "pair" in c[4]]
    assert [c[:3] for c in rec] == [("dna", 48, 37), ("rna", 500, 20)] and all(set(c[4]) == set(pc._RNN) for c in rec)
    pad = lambda n: -(-n // r["pad"]) * r["pad"]
    for c in rec:
        groups = pad(c[2]) // 4                                # 4-row groups of the padded batch: all of them pair up within one round
        assert pad(c[2]) > r["pad"] and groups % 2 == 0 and groups // 2 <= fc.CUS // 2
    spec, w, x, sl, TT = pc.case_inputs(rec[0])
    assert (sl[:16] < TT / 4).all() and sl[16] == TT             # a whole 16-row group finishes early
    assert specs["rna"].rnn_kind == "multi" and specs["dna"].rnn_kind == "stack"
    # the projections' edges of tests/test_gpu_proj_bf16x3.py; engines of 1, 2, 3 layers end in the K = 256 / K = 200 kernels
    c = by["dna-L61-B4"]
    assert set(c[4]) == {"default", "proj-fp32"} and (T(c) * pad(c[2])) % 128 and pad(c[2]) == pad(3)
    c = by["dna-L400-B1"]
    assert set(c[4]) == {"default", "proj-fp32"} and pad(c[2]) - c[2] == 15 and form["dna-L400-B1"] == "f4"
    assert specs["dna"].rnn_layers == 3 and specs["dna"].blocks[-1]["out"] == 256 and 2 * specs["dna"].hidden == 200
    assert len(pc.RUNS) == sum(len(c[4]) for c in pc.CASES) == 60
