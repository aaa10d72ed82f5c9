"""GPU: chiron_ctc_align (csrc/ctc_align.hip) through chiron_amd.label against the numpy float64 restatement of
tests/ctc_align_ref.py.  Every comparison is exact: start, the float64 bits of score, band and status, no tolerance.  Scores are
integer-valued floats where ties are the point and float32 N(0,1) with the planted path's class raised by 6 elsewhere.  band0
is an argument, so the band logic is exercised at small shapes."""
import json
import os

import numpy as np
import pytest

from chiron_amd import label, labelled

import ctc_align_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(xs, labs, band0, max_band=0, want=None):
    got = label.align(xs, labs, band0=band0, max_band=max_band)
    want = want or ref.align(xs, labs, band0, max_band)
    for k in range(len(xs)):
        where = (k, xs[k].shape[0], len(labs[k]), band0, max_band)
        assert int(got["status"][k]) == int(want["status"][k]), where
        assert int(got["band"][k]) == int(want["band"][k]), where
        assert got["score"][k].tobytes() == want["score"][k].tobytes(), where + (got["score"][k], want["score"][k])
        assert got["start"][k].dtype == np.int32 and np.array_equal(got["start"][k], want["start"][k]), where
    return got, want


def _planted_exact(rng, L, F, dwell_weight=None, repeats=True):
    """A planted path of exactly F frames over L random bases: every base at least one frame, a blank between equal neighbours,
    the other frames dealt to the bases by dwell_weight (uniform by default).  repeats=False: no two neighbours equal."""
    lab = rng.integers(0, 4, size=L).astype(np.uint8)
    if not repeats:
        lab = (np.cumsum(rng.integers(1, 4, size=L)) % 4).astype(np.uint8)
    rep = int(np.count_nonzero(lab[1:] == lab[:-1]))
    extra = F - L - rep
    assert extra >= 0
    p = np.ones(L) if dwell_weight is None else np.asarray(dwell_weight, dtype=np.float64)
    dwell = 1 + rng.multinomial(extra, p / p.sum())
    classes = []
    for j in range(L):
        if j and lab[j] == lab[j - 1]:
            classes.append(ref.BLANK)
        classes += [int(lab[j])] * int(dwell[j])
    x = rng.standard_normal((F, 5)).astype(np.float32)
    x[np.arange(F), classes] += np.float32(6)
    return x, lab


def _ints(rng, F):
    return rng.integers(-3, 4, size=(F, 5)).astype(np.float32)


def _codes(s):
    return np.array(["ACGT".index(c) for c in s], dtype=np.uint8)


@pytest.mark.parametrize("band0", [0, 1, 3])
def test_edge_cases_in_one_launch(built, band0):
    rng = np.random.default_rng(21)
    single = np.array([2, 0, 3, 1, 2, 0, 1], np.uint8)                  # no repeats: F = L has a single path
    cases = [
        (_ints(rng, 1), _codes("")),                                    # L = 0, F = 1
        (_ints(rng, 5), _codes("")),                                    # L = 0, F = 5
        (_ints(rng, 1), _codes("G")),                                   # L = 1, F = 1
        (_ints(rng, 7), single),                                        # F = L, no repeats
        (_ints(rng, 4), _codes("AAC")),                                 # F = L + repeats exactly
        (_ints(rng, 7), _codes("AAAA")),
        (_ints(rng, 3), _codes("AAC")),                                 # one short: status 1
        (_ints(rng, 6), _codes("AAAA")),
        (_ints(rng, 0), _codes("ACG")),                                 # F = 0 with L > 0: status 1
        (np.zeros((12, 5), np.float32), _codes("ACGT")),                # all-zero scores: the tie order alone decides
        (np.zeros((40, 5), np.float32), _codes("AACCA")),
        (_ints(rng, 60), _codes("T" * 17)),                             # one repeated base
        (_ints(rng, 33), _codes("T" * 17)),                             # ... at F = L + repeats exactly
        (_ints(rng, 25), _codes("ACGTTGCA")),
    ]
    xs, labs = [c[0] for c in cases], [c[1] for c in cases]
    got, want = _check(xs, labs, band0)
    assert got["status"].tolist() == [0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0]
    assert got["score"][0] == float(xs[0][0, 4]) and got["score"][1] == float(xs[1][:, 4].astype(np.float64).sum())
    assert got["start"][3].tolist() == list(range(7))
    assert got["start"][4].tolist() == [0, 2, 3] and got["start"][5].tolist() == [0, 2, 4, 6]
    for k in (6, 7, 8):
        assert np.all(got["start"][k] == -1) and got["score"][k] == -np.inf
    if band0 == 0:
        assert np.all(got["band"] == 0)
    # the empty call is a no-op
    none = label.align([], [], band0=band0)
    assert none["start"] == [] and none["score"].shape == (0,)


@pytest.mark.parametrize("mult", [3, 9])
@pytest.mark.parametrize("band0", [0, 8])
def test_boundaries_of_wave_and_workgroup(built, band0, mult):
    """S = 2L+1 around a wave's and the workgroup's share of states (a thread owns four): L in 31 .. 257, F = 3L and 9L."""
    rng = np.random.default_rng(22 + mult)
    xs, labs = [], []
    for L in (31, 32, 127, 128, 129, 255, 256, 257):
        x, lab = _planted_exact(rng, L, mult * L)
        xs.append(x)
        labs.append(lab)
    got, _ = _check(xs, labs, band0)
    assert np.all(got["status"] == 0)


def test_band_doubling_and_exhaustion(built):
    """Uneven dwell: the first bases take one or two frames each and the last ones twenty, so the path runs far off the band's
    centre line and band0 = 4 needs several doublings.  The band each read stops at is the reference's.  With max_band below
    what such a read needs it ends with status 2."""
    rng = np.random.default_rng(23)
    xs, labs = [], []
    for L, F in ((120, 1300), (90, 700), (60, 900)):
        weight = np.where(np.arange(L) < L // 2, 0.02, 1.0)
        for wgt in (weight, weight[::-1], None):
            x, lab = _planted_exact(rng, L, F, wgt)
            xs.append(x)
            labs.append(lab)
    got, want = _check(xs, labs, 4)
    assert np.all(got["status"] == 0)
    assert max(want["band"]) >= 64 and min(want["band"]) <= 32, want["band"]
    got, want = _check(xs, labs, 4, 16)
    assert set(got["status"].tolist()) == {0, 2}, got["status"]
    for k in np.flatnonzero(got["status"] == 2):
        assert np.all(got["start"][k] == -1) and got["score"][k] == -np.inf and got["band"][k] <= 16
    _check(xs, labs, 4, 4)
    _check(xs, labs, 5, 40)


def test_lds_to_workspace_rows(built):
    """The recursion rows leave LDS when the band has more than LDS_SLOTS states.  A band has min(2w + 1, S) states, an odd
    number, so LDS_SLOTS = 4096 itself cannot occur: the last width LDS holds is LDS_SLOTS - 1 (w = 2047, or L = 2047 in full)
    and the first in the workspace rows is LDS_SLOTS + 1 (w = 2048, or L = 2048 in full).  And a full table well past LDS,
    L = 2050 with F = 2300."""
    rng = np.random.default_rng(24)
    S_LDS = label.LDS_SLOTS
    assert S_LDS == 4096
    x, lab = _planted_exact(rng, 2100, 2400, repeats=False)
    for w in (S_LDS // 2 - 1, S_LDS // 2):                               # 4095 and 4097 states of S = 4201
        got, _ = _check([x], [lab], w)
        assert int(got["band"][0]) == w and int(got["status"][0]) == 0
    xs, labs = [], []
    for L, F in ((S_LDS // 2 - 1, 2700), (S_LDS // 2, 2700), (2050, 2300)):
        a, b = _planted_exact(rng, L, F, repeats=L != 2050)
        xs.append(a)
        labs.append(b)
    _check(xs, labs, 0)


def test_doubling_across_the_lds_threshold(built):
    """One read whose band doubles from 1024 (2049 states, in LDS) to 2048 (4097 states, workspace rows) inside the launch: its
    first 1500 bases take one frame each, which puts the path 1500 states off the centre line."""
    rng = np.random.default_rng(27)
    L = 2300
    x, lab = _planted_exact(rng, L, 2 * L, np.where(np.arange(L) < 1500, 1e-5, 1.0), repeats=False)
    got, want = _check([x], [lab], 1024)
    assert int(want["band"][0]) == 2048 and int(want["status"][0]) == 0, want["band"]


def test_batch_of_256_is_deterministic_and_order_independent(built):
    rng = np.random.default_rng(25)
    xs, labs = [], []
    for k in range(256):
        L = int(rng.integers(0, 31))
        lab = rng.integers(0, 4, size=L).astype(np.uint8)
        rep = int(np.count_nonzero(lab[1:] == lab[:-1]))
        if k % 9 == 0 and L > 1:                                        # infeasible
            xs.append(_ints(rng, int(rng.integers(0, L + rep))))
            labs.append(lab)
        elif k % 4 == 0 and L > 12:                                     # far off the centre line: max_band 8 is not enough
            x, lab = _planted_exact(rng, L, 6 * L, np.where(np.arange(L) < L // 2, 0.01, 1.0))
            xs.append(x)
            labs.append(lab)
        elif k % 3 == 0:
            xs.append(_ints(rng, L + rep + int(rng.integers(0, 40))))
            labs.append(lab)
        else:
            x, lab = _planted_exact(rng, max(L, 1), int(rng.integers(2, 5)) * max(L, 1))
            xs.append(x)
            labs.append(lab)
    first, want = _check(xs, labs, 2, 8)
    assert {0, 1, 2} == set(first["status"].tolist())
    second = label.align(xs, labs, band0=2, max_band=8)
    for key in ("score", "band", "status"):
        assert first[key].tobytes() == second[key].tobytes()
    assert all(np.array_equal(a, b) for a, b in zip(first["start"], second["start"]))
    for k in reversed(range(256)):
        one = label.align([xs[k]], [labs[k]], band0=2, max_band=8)
        assert one["score"].tobytes() == first["score"][k:k + 1].tobytes() and one["band"][0] == first["band"][k], k
        assert one["status"][0] == first["status"][k] and np.array_equal(one["start"][0], first["start"][k]), k


def _fasta(path, name, codes):
    with open(path, "w") as f:
        f.write(">%s\n%s\n" % (name, "".join("ACGT"[c] for c in codes)))


@pytest.mark.parametrize("model", ["DNA_default", "RNA_default"])
def test_label_command_end_to_end(built, tmp_path, model):
    """`label` on a few synthetic reads with --synthetic-weights (the logits are meaningless; the alignment is defined for any
    scores): every .label written equals what this test derives from the same engine's logits through the numpy reference and
    the label.py helpers, and the output folder is one the labelled reader takes.  RNA_default: five samples per frame."""
    import chiron_amd as ca
    from chiron_amd import assess, entry, fast5, model as model_mod
    from chiron_amd.engine import Engine
    rng = np.random.default_rng(26)
    model_dir = os.path.join(ROOT, "chiron_amd", "model", model)
    inp, out = tmp_path / "in", tmp_path / "out"
    (inp / "raw").mkdir(parents=True)
    (inp / "reference").mkdir()
    n_bases = {"DNA_default": 300, "RNA_default": 120}[model]
    sigs, refs = {}, {}
    for k, n in enumerate((3000, 2900, 3100, 3000, 3050)):
        name = "read%d" % k
        sigs[name] = ca.synthetic_signal(1, n, seed=40 + k)[0]
        fast5.write_signal_text(str(inp / "raw" / (name + ".signal")), sigs[name])
        if k == 1:
            continue                                                    # no reference
        refs[name] = rng.integers(0, 4, size=n + 50 if k == 3 else n_bases + 7 * k).astype(np.uint8)    # read3: more bases than frames
        _fasta(str(inp / "reference" / (name + ".fasta")), name, refs[name])
    argv = ["label", "-i", str(inp), "-o", str(out), "-m", model_dir, "-l", "400", "-b", "16", "--synthetic-weights"]
    report = entry.main(argv)
    on_disk = json.loads((out / "label_report.json").read_text())
    assert on_disk["totals"] == report["totals"] and on_disk["no_reference"] == ["read1"] and on_disk["no_reference_count"] == 1
    by = {r["name"]: r for r in on_disk["reads"]}
    assert by["read3"]["status"] == "infeasible" and on_disk["totals"]["infeasible"] == 1
    assert not (out / "read3.label").exists() and not (out / "read1.label").exists()
    spec, weights, _ = model_mod.load_model(model_dir, allow_synthetic=True)
    written = 0
    with Engine(spec, weights, max_batch=16, segment_len=400) as eng:
        assert eng.ratio == {"DNA_default": 1.0, "RNA_default": 5.0}[model]
        for name in ("read0", "read2", "read4"):
            sig, codes = sigs[name], refs[name]
            logits, sl = label.read_frames(eng, sig, 16)
            start, score, band, status = ref.align_one(logits, codes, 256, 8192)
            rec = by[name]
            assert (rec["frames"], rec["bases"], rec["band"], rec["status"]) == (logits.shape[0], len(codes), band, "aligned") and status == 0
            assert rec["score"] == score
            x = logits.astype(np.float64)
            lse = np.log(np.exp(x - x.max(axis=1)[:, None]).sum(axis=1)) + x.max(axis=1)
            assert rec["mean_log_prob"] == pytest.approx((score - lse.sum()) / len(x), rel=1e-12)
            want = label.spans(label.frames_to_samples(start, sl, 400, eng.ratio, len(sig)), len(sig))
            lab = labelled.read_label(str(out / (name + ".label")), skip_start=0)
            assert len(lab.base) == len(codes) and lab.base == codes.tolist()
            assert lab.start == [a for a, _ in want] and lab.length == [b - a for a, b in want]
            ends = [s + n for s, n in zip(lab.start, lab.length)]
            assert all(n > 0 for n in lab.length) and lab.start[1:] == ends[:-1] and lab.start[0] >= 0 and ends[-1] <= len(sig)
            assert np.array_equal(assess.encode("".join("ACGT"[c] for c in lab.base)), codes)
            assert np.array_equal(np.loadtxt(str(out / (name + ".signal")), dtype=np.float32), sig)
            written += 1
    assert on_disk["totals"]["written"] == written == 3 and on_disk["totals"]["aligned"] == 3
    ds = labelled.read_raw_data_sets(str(out), 400)
    assert ds.event.shape[0] >= 1 and ds.event.shape[1] == 400
