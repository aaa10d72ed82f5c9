"""CPU: block 1's table (csrc/weight_pack.h), read back by tests/native/pwl_table_dump.cpp and evaluated in the arithmetic of
csrc/pwl.hip (tests/pwl_ref.py table_eval), against the formula it tabulates -- at every row of the table.

Accuracy     every weight set of pwl_ref.WEIGHT_SETS, every sample of pwl_ref.samples_for in ragged windows: per sample and tap, and per
             position of conv2b's output, ||table - formula64||_2 over the channels <= FACTOR * e32 + 1e-6 * scale (e32: the formula in
             float32; FACTOR: profiles/pwl_table_accuracy.json, recomputed here); per element |table - formula64| <= FACTOR * e32 +
             1e-6 * sum_c |W| relu(.); everything finite; +0.0 and -0.0 give the same bits.
Coverage     a condition: the samples select every row that holds a float32 value, and miss exactly the rows bounded by a breakpoint
             at +-inf or by two equal breakpoints; the zero-centred set has reference points at 0, at lower and at upper bounds.  What
             the synthetic signal selects with the synthetic weights -- all the GPU suite read before -- is pinned beside it.
Sensitivity  five ways of reading the table wrongly each miss the bar on every weight set they apply to.
Harmless     `<=` instead of `<` at an exact breakpoint still meets the bar: the function is continuous there, both rows give f(bp) up to
             rounding, which is why no test asserts the tie rule.
Halves       the capped sample set of the half formats drops values of the two outermost rows only and still selects every row; the
             per-element, tie-aware judgement of the fp16 engine (pwl_ref.half_check) accepts the table evaluated in float32 and
             rounded where the engine rounds, and rejects the same with a wrong row."""
import numpy as np
import pytest

import chiron_amd as ca

import f16_ref
import pwl_hip
import pwl_ref as pr

SETS = list(pr.WEIGHT_SETS)
# rows no finite sample can select: planted() has breakpoints at -inf and +inf; the equal pairs bound an empty interval each
UNREACHABLE = {"planted": 2, "equal-breakpoints": 2}


@pytest.fixture(scope="module")
def factor():
    return pr.committed()["factor"]


@pytest.fixture(scope="module")
def refs():
    """per weight set, once: (spec, weights, dump, x, y2b in float64, y2b in float32)"""
    cache = {}

    def get(name):
        if name not in cache:
            spec, w, d, x = pr.cpu_case(name)
            cache[name] = (spec, w, d, x, pr.y2b_formula(x, w, spec), pr.y2b_formula(x, w, spec, np.float32))
        return cache[name]
    return get


def test_the_committed_factor_is_what_the_cpu_ensemble_gives(factor):
    rec = pr.committed()
    assert rec["weight_sets"] == SETS and rec["floor"] == pr.FLOOR
    largest = {lv: max(pr.cpu_ratios(name, rec["draws"])[lv] for name in SETS) for lv in ("taps", "y2b", "features")}
    for lv, v in largest.items():
        assert np.isfinite(v) and abs(v - rec["largest_err_over_e32"][lv]) <= 1e-9 * max(1.0, v), (lv, v, rec["largest_err_over_e32"][lv])
        assert factor[lv] == pr.factor_of(v), (lv, factor[lv], v)


@pytest.mark.parametrize("name", SETS)
def test_the_table_meets_the_bar_at_every_sample_tap_and_channel(refs, factor, name):
    spec, w, d, x, y64, y32 = refs(name)
    s = pr._bits_unique(x.reshape(-1))
    assert set(pr.samples_for(d).view(np.uint32).tolist()) <= set(s.view(np.uint32).tolist())      # the windows hold every sample
    t, t64, t32, tsc = pr.table_taps(s, d), pr.formula(s, w, spec), pr.formula(s, w, spec, np.float32), pr.formula(s, w, spec, scale=True)
    assert np.isfinite(t).all()
    err, e32 = np.abs(t - t64), np.abs(t32 - t64)
    bad = err > factor["taps"] * e32 + pr.FLOOR * tsc
    print(name, "per element: largest err / sum|W|relu %.3g (float32 formula %.3g)" % (np.max(err / np.maximum(tsc, 1e-300)), np.max(e32 / np.maximum(tsc, 1e-300))))
    assert not bad.any(), (int(bad.sum()), s[np.argwhere(bad)[0][0]])
    j = pr.per_position(t, t64, t32, factor["taps"])
    assert j["ok"].all(), (name, "taps", int((~j["ok"]).sum()), j["ratio"])
    y = pr.table_eval(x, d)
    assert np.isfinite(y).all()
    j = pr.per_position(y, y64, y32, factor["y2b"])
    print(name, "y2b per position: largest err / e32 %.3g, err / scale %.3g" % (j["raw"], np.max(j["err"] / np.maximum(j["scale"], 1e-300))))
    assert j["ok"].all(), (name, "y2b", int((~j["ok"]).sum()), j["ratio"])
    zero = np.zeros((2, x.shape[1]), dtype=np.float32)
    zero[1] = -0.0
    assert np.signbit(zero[1]).all() and not np.signbit(zero[0]).any()
    yz = pr.table_eval(zero, d)
    assert np.array_equal(yz[0].view(np.uint32), yz[1].view(np.uint32))


@pytest.mark.parametrize("name", SETS)
def test_the_samples_select_every_row_a_float_can_reach(name):
    spec, w, d, x = pr.cpu_case(name)
    rows = set(pr.intervals(pr.samples_for(d), d).tolist())
    every = set(range(d["nbp"] + 1))
    reach = set(pr.reachable_rows(d))
    assert rows == reach, (sorted(reach - rows), sorted(rows - reach))
    missed = sorted(every - rows)
    assert len(missed) == UNREACHABLE.get(name, 0), missed
    bp = d["bp"]
    for iv in missed:          # ... and exactly those: bounded by a breakpoint at +-inf, or between two equal breakpoints
        assert (iv == 0 and bp[0] == -np.inf) or (iv == d["nbp"] and bp[iv - 1] == np.inf) or (0 < iv < d["nbp"] and bp[iv - 1] == bp[iv]), iv
    if name == "planted":
        assert missed == [0, d["nbp"]] and np.isfinite(bp[1:-1]).all() and bp[1] < -1e29
    if name == "no-breakpoints":
        assert d["nbp"] == 0 and rows == {0}
    if name == "zero-centred":
        kinds = pr.ref_kinds(d, sorted(rows))
        assert kinds["zero"] == 1 and kinds["lower"] > 50 and kinds["upper"] > 50 and sum(kinds.values()) == len(rows), kinds


def test_what_the_synthetic_signal_selects_with_the_synthetic_weights():
    """the gap this file closes, as a fact: the integers of ca.synthetic_signal between the extreme breakpoints select 50 inner rows and
    the two tails, 52 of 257; more than half of the samples land in the two outermost rows; every selected row but row 0 has its
    reference point at its lower bound.  A change of the synthetic model fails this."""
    d = pr.set_dump("synthetic-dna", 130)
    assert d["nbp"] == 256 and 463.8 < d["bp"][0] < 463.9 and 525.3 < d["bp"][-1] < 525.4
    sig = np.concatenate([ca.synthetic_signal(1, 200000, seed=3)[0], np.zeros(1, np.float32)])
    assert (sig == np.rint(sig)).all() and sig.min() == 0 and 150 < np.sort(np.unique(sig))[1] and sig.max() < 1100
    iv = pr.intervals(sig, d)
    rows = sorted(set(iv.tolist()))
    assert len(rows) == 52 and rows[0] == 0 and rows[-1] == 256, (len(rows), rows[:3], rows[-3:])
    assert np.mean((iv == 0) | (iv == 256)) > 0.5
    kinds = pr.ref_kinds(d, rows)
    assert kinds == {"zero": 1, "lower": 51, "upper": 0}, kinds
    assert len(set(pr.intervals(pr.samples_for(d), d).tolist())) == 257


@pytest.mark.parametrize("mutation", list(pr.MUTATIONS))
@pytest.mark.parametrize("name", SETS)
def test_a_table_read_wrongly_misses_the_bar(refs, factor, name, mutation):
    spec, w, d, x, y64, y32 = refs(name)
    if not pr.applies(mutation, d, x):
        # not a skip: the mutation changes nothing here (no row above the only one; every selected row's reference point IS its lower bound)
        assert np.array_equal(pr.table_eval(x, d, mutation).view(np.uint32), pr.table_eval(x, d).view(np.uint32))
        return
    with np.errstate(over="ignore", invalid="ignore"):
        y = pr.table_eval(x, d, mutation)
    j = pr.per_position(np.nan_to_num(y.astype(np.float64), nan=np.inf), y64, y32, factor["y2b"])
    print(name, mutation, "positions over the bar: %d of %d" % (int((~j["ok"]).sum()), j["ok"].size))
    assert not j["ok"].all()


def test_every_mutation_applies_somewhere():
    seen = {m: [name for name in SETS if pr.applies(m, *pr.cpu_case(name)[2:])] for m in pr.MUTATIONS}
    assert all(len(v) >= 2 for v in seen.values()), seen
    assert set(seen["ref-lower"]) == {"zero-centred", "planted"}, seen["ref-lower"]


@pytest.mark.parametrize("name", SETS)
def test_the_other_tie_rule_at_a_breakpoint_is_harmless(refs, factor, name):
    spec, w, d, x, y64, y32 = refs(name)
    on_bp = np.isin(x.reshape(-1), d["bp"][:d["nbp"]])
    assert on_bp.any() or d["nbp"] == 0
    if d["nbp"]:
        assert (pr.intervals(x.reshape(-1), d, "<=") != pr.intervals(x.reshape(-1), d))[on_bp].all()
    j = pr.per_position(pr.table_eval(x, d, tie="<="), y64, y32, factor["y2b"])
    assert j["ok"].all(), (name, int((~j["ok"]).sum()))


@pytest.mark.parametrize("name", SETS)
def test_the_half_formats_cap_drops_tail_values_only(name):
    spec, w = pr.weight_set(name)
    d = pr.set_dump(name, pr.CPU_L[pr.WEIGHT_SETS[name][0]])
    kept, dropped = pr.samples_capped(d, w, spec)
    if name == "planted":      # a constant channel of 1e9: no value survives, the set runs in the wide formats only
        assert len(kept) == 0 and all(name != c[0] or not set(c[3]) & set(pwl_hip.HALF_FORMS) for c in pwl_hip.CASES)
        return
    iv = pr.intervals(dropped, d)
    assert np.isin(iv, [0, d["nbp"]]).all(), dropped
    assert set(pr.intervals(kept, d).tolist()) == set(pr.reachable_rows(d))


@pytest.mark.parametrize("c", pwl_hip.CASES, ids=[pwl_hip.case_id(c) for c in pwl_hip.CASES])
def test_the_gpu_cases_inputs(c):
    """what tests/test_gpu_pwl.py feeds: the long cases hold every sample, whole windows begin and end in the extreme values, the half
    formats' reference stays far from a half's largest value"""
    for capped in sorted({f in pwl_hip.HALF_FORMS for f in c[3]}):
        spec, w, x, sl, s, placed = pwl_hip.case_inputs(c, capped)
        k, L = spec.blocks[0]["k"], c[1]
        assert x.shape[1] == L and np.isfinite(x).all() and (c[2] is None or x.shape[0] == c[2])
        if c[2] is None:
            assert placed == len(s) and set(s.view(np.uint32).tolist()) <= set(x.view(np.uint32).reshape(-1).tolist())
        extremes = np.concatenate([np.sort(s[s > 0])[-2:], np.sort(s[s < 0])[:2]])       # the two largest and the two most negative
        edge = np.concatenate([x[0, :k], x[0, -k:]])
        assert extremes.size == 4 and np.isin(edge, extremes).all() and (L < 2 * k or set(edge.tolist()) == set(extremes.tolist())), edge
        if capped:
            y = pr.y2b_formula(x, w, spec)
            fea = np.maximum(pr.block_tail(y, x, w, spec, np.float64), 0)
            assert max(y.max(), fea.max()) < 5e4, (y.max(), fea.max())


def test_one_channel_wrong_by_a_thousandth_misses_both_judgements(factor):
    """the judgements of tests/test_gpu_pwl.py on a small defect of the whole table: the table of weights with ONE conv2a offset off by
    1e-3 (pwl_hip.one_channel_wrong), against the true weights' formula"""
    spec, w, d, x = pr.cpu_case("synthetic-dna", capped=True)
    wrong = pr.dump(spec, pwl_hip.one_channel_wrong(w), x.shape[1])
    y = pr.table_eval(x, wrong)
    j = pr.per_position(y, pr.y2b_formula(x, w, spec), pr.y2b_formula(x, w, spec, np.float32), factor["y2b"])
    print("positions over the bar: %d of %d; largest err / scale %.3g" % (int((~j["ok"]).sum()), j["ok"].size, np.max(j["err"] / j["scale"])))
    assert (~j["ok"]).mean() > 0.25
    fea = f16_ref.f16(np.maximum(pr.block_tail(f16_ref.f16(y), x, w, spec, np.float32, "fp16"), np.float32(0)))
    h = pr.half_check(fea, x, w, spec, factor["features"])
    print("elements over the bar: %d of %d" % (int((~h["ok"]).sum()), h["elements"]))
    assert not h["ok"].all()


@pytest.mark.parametrize("name", ["synthetic-dna", "zero-centred", "synthetic-rna"])
def test_the_half_judgement_accepts_a_correct_engine_and_rejects_a_wrong_row(factor, name):
    spec, w, d, x = pr.cpu_case(name, capped=True)

    def engine(mutate):        # the fp16 engine's arithmetic on the CPU: the table in float32, halves where the engine stores them
        b = f16_ref.f16(pr.table_eval(x, d, mutate))
        return f16_ref.f16(np.maximum(pr.block_tail(b, x, w, spec, np.float32, "fp16"), np.float32(0)))
    good = pr.half_check(engine(None), x, w, spec, factor["features"])
    print(name, {k: v for k, v in good.items() if k != "ok"})
    assert good["ok"].all(), int((~good["ok"]).sum())
    # (1e-6 of the terms' magnitudes is 13 .. 23 % of a half-ulp's width around the ties here: that share of conv2b's live outputs may
    # round either way; the rest is held to the nearest half -- enough for every mutation below)
    for mutation in pr.MUTATIONS:
        if pr.applies(mutation, d, x):
            bad = pr.half_check(engine(mutation), x, w, spec, factor["features"])
            print(name, mutation, "elements over the bar: %d" % int((~bad["ok"]).sum()))
            assert not bad["ok"].all(), mutation
