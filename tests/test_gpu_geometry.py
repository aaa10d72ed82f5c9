"""GPU (-m gpu): every kernel form across window geometry, against the oracles.

The engine derives its kernel forms from the window's frame count T at creation (engine.hip, conv2b plan):
  odd T                      conv2b of blocks 2 and 3 on the direct DMA GEMM (gemm.hip);
  even T < 256, or T % 4     Winograd F(2,3) (wino.hip wino_conv3_kernel), 128-pair tiles across window boundaries;
  T % 4 == 0 and T >= 256    Winograd F(4,3) (wino_conv3_f4_kernel), 128-quad tiles.
Both Winograd forms swap in the SAME padding zero at the first and last pair / quad of each window.  The strided first block and
the HEAD stems pad by L mod stride (same_pad), which the table conv (pwl.hip), the lifted GEMM segments and the stem conv read.
Each row below names the branch or edge it hits; every row runs ragged windows (seq_len 0, 1 and T among them, the signal zeroed
past each window's samples), checks fp32 and fp32-split against the oracle at 1e-4 and the decode bit for bit, and proves with the
engine's own profile which conv2b form ran."""
import numpy as np
import pytest

import chiron_amd as ca
from test_gpu_parity import TOL, _check_beam, _check_decode, _windows

pytestmark = pytest.mark.gpu

F16_TOL = 0.08            # the f16 bar of the randomized-shapes test: valid frames against the fp32 engine
_SWITCHES = ("CHIRON_WINOGRAD_F2", "CHIRON_WINOGRAD_F4", "CHIRON_NO_WINOGRAD", "CHIRON_NO_PWL", "CHIRON_BEAM_SINGLE", "CHIRON_BEAM_GENERIC",
             "CHIRON_LSTM_WIDE", "CHIRON_LSTM_PAIR", "CHIRON_NO_STREAM16", "CHIRON_STATIC_TILES")


@pytest.fixture(scope="module")
def models(built):
    specs = {"dna": ca.dna_default_spec(), "rna": ca.rna_default_spec(),
             "rna_model2": ca.rna_head_spec("rna_model2"), "rna_model3": ca.rna_head_spec("rna_model3")}
    return {k: (s, ca.synthetic_weights(s, seed=61 + i)) for i, (k, s) in enumerate(sorted(specs.items()))}


@pytest.fixture
def clean_env(monkeypatch):
    for v in _SWITCHES:
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


# (topology, segment_len L, batch B, max_batch, beam): the comment names the conv2b form the rule picks and the edge.  Pairs = B*T/2,
# quads = B*T/4 against the 128-pair / 128-quad tile.
_DNA = [
    ("dna", 1, 3, 3, True),         # T = 1: direct; no pair fits; recurrence prefetch clamped to frame 0
    ("dna", 2, 3, 16, True),        # F(2,3): one pair per window, first AND last; 3 pairs, far below one tile
    ("dna", 3, 5, 7, True),         # odd: direct, T below the conv width
    ("dna", 4, 7, 16, False),       # F(2,3): two pairs per window (first, last); 14 pairs
    ("dna", 5, 2, 2, False),        # odd: direct
    ("dna", 7, 9, 32, False),       # odd: direct
    ("dna", 8, 5, 21, False),       # F(2,3) though T % 4 == 0 (below 256); 20 pairs
    ("dna", 30, 13, 13, False),     # F(2,3), T % 4 == 2; 195 pairs: a tile boundary mid-window; f16: stream16 fallback region
    ("dna", 32, 9, 48, False),      # F(2,3); 144 pairs
    ("dna", 33, 6, 6, True),        # odd: direct
    ("dna", 64, 5, 16, False),      # F(2,3); 160 pairs
    ("dna", 127, 3, 5, False),      # odd: direct
    ("dna", 130, 3, 33, False),     # F(2,3), T % 4 == 2; 195 pairs
    ("dna", 252, 3, 3, False),      # F(2,3) just below the F(4,3) threshold; 378 pairs
    ("dna", 254, 5, 17, False),     # F(2,3), T % 4 == 2; 635 pairs
    ("dna", 255, 2, 2, False),      # odd: direct
    ("dna", 256, 3, 16, False),     # F(4,3) threshold; 192 quads = 1.5 tiles
    ("dna", 257, 5, 5, True),       # odd: direct, first length above the threshold
    ("dna", 258, 3, 64, False),     # F(2,3) above 256 (T % 4 == 2); 387 pairs
    ("dna", 260, 7, 7, False),      # F(4,3); 455 quads
    ("dna", 398, 3, 19, False),     # F(2,3) (T % 4 == 2); 597 pairs
    ("dna", 399, 2, 2, False),      # odd: direct
    ("dna", 401, 3, 3, False),      # odd: direct, the headline length + 1
    ("dna", 500, 3, 32, False),     # F(4,3); 375 quads (no-preset DNA call window)
    ("dna", 1024, 3, 8, False),     # F(4,3); 768 quads: tiles end exactly at the batch end
    ("dna", 4000, 3, 4, False),     # F(4,3); 3000 quads; 4000-step recurrence
]
# RNA_default: k 13 / stride 5 first block, T = ceil(L / 5); every L mod 5 (every left pad of the table conv) around each T
_RNA = [
    ("rna", 1, 3, 3, False),        # T = 1 (left pad 6), L far below the k = 13 window: direct
    ("rna", 3, 2, 16, False),       # T = 1, left pad 5
    ("rna", 5, 4, 4, False),        # T = 1, left pad 4
    ("rna", 6, 5, 17, False),       # T = 2: F(2,3), one pair first and last
    ("rna", 12, 3, 3, False),       # T = 3: direct, left pad 5
    ("rna", 13, 3, 8, True),        # T = 3: L == k, direct
    ("rna", 14, 2, 2, False),       # T = 3: direct
    ("rna", 156, 5, 5, False),      # T = 32: F(2,3), every L mod 5 ...
    ("rna", 157, 3, 16, False),
    ("rna", 158, 7, 9, False),
    ("rna", 159, 2, 2, False),
    ("rna", 160, 4, 32, False),     # ... L mod 5 == 0
    ("rna", 496, 3, 3, False),      # T = 100: F(2,3) (RNA_default's own window is 500)
    ("rna", 497, 2, 16, False),
    ("rna", 498, 5, 5, False),
    ("rna", 499, 3, 7, False),
    ("rna", 500, 4, 4, False),
    ("rna", 501, 3, 3, True),       # T = 101: odd, direct
    ("rna", 1276, 2, 2, False),     # T = 256: F(4,3) on the RNA topology ...
    ("rna", 1277, 3, 16, False),
    ("rna", 1278, 2, 5, False),
    ("rna", 1279, 3, 3, False),
    ("rna", 1280, 2, 2, False),
    ("rna", 1281, 3, 3, False),     # T = 257: direct
    ("rna", 1996, 2, 2, False),     # T = 400: F(4,3) (the rna-pre window 2000) ...
    ("rna", 1997, 3, 3, False),
    ("rna", 1998, 2, 16, False),
    ("rna", 1999, 2, 2, False),
    ("rna", 2000, 3, 3, False),
    ("rna", 2001, 2, 2, False),     # T = 401: direct
    ("rna", 2500, 2, 2, False),     # T = 500: F(4,3)
]
# HEAD stems: strided stem conv (rna_model3 k 14 / s 7, rna_model2 k 9 / s 5) then three 256-channel stride-1 blocks (all three
# on the conv2b rule); every L mod stride around one T below 256 and one above
_STEM = ([("rna_model3", L, 2, 4, False) for L in range(694, 701)]           # T = 100: F(2,3)
         + [("rna_model3", L, 2, 2, False) for L in range(1793, 1800)]       # T = 257: direct
         + [("rna_model2", L, 2, 3, False) for L in range(486, 491)]         # T = 98: F(2,3), T % 4 == 2
         + [("rna_model2", L, 2, 2, False) for L in range(1496, 1501)])      # T = 300: F(4,3)
_ROWS = _DNA + _RNA + _STEM


def _row_id(r):
    return "%s-L%d-B%d-mb%d%s" % (r[0], r[1], r[2], r[3], "-beam" if r[4] else "")


def _wino_blocks(spec):
    """blocks whose conv2b the Winograd rule applies to: 1 x 3, stride 1, 256 -> 256 channels (not the lifted first block)"""
    return sum(1 for b in spec.blocks if b["k"] == 3 and b["stride"] == 1 and b["in"] == b["out"] and b["in"] > 1)


def _lifted(spec):
    return spec.blocks[0]["in"] == 1


def _ragged(spec, L, B, seed):
    """B windows of L samples: seq_len T, 1 and 0 in the first rows, random lengths after; signal zeroed past each window's samples"""
    T = spec.output_len(L)
    ratio = L / T
    x, _ = _windows(L * B, L, L, seed=seed)
    rng = np.random.RandomState(seed)
    ln = rng.randint(0, L + 1, size=B)
    head = [L, min(L, int(np.ceil(ratio))), 0][:B]
    ln[:len(head)] = head
    for b in range(B):
        x[b, ln[b]:] = 0
    sl = np.minimum(ca.seq_len_for_engine(ln, ratio), T).astype(np.int32)
    sl[:len(head)] = [T, 1, 0][:B]
    return x, sl, T


def _profile_launches(eng):
    return {k: v["launches"] for k, v in eng.profile_read().items()}


def _expect_forms(spec, prof, T, dtype="fp32", env=()):
    """the kernel forms the rule says ran for one batch, read from the engine's profile"""
    wino = (dtype == "fp32" and spec.bn_mode == "population" and T % 2 == 0 and "CHIRON_NO_WINOGRAD" not in env)
    assert prof.get("conv_wino", 0) == (_wino_blocks(spec) if wino else 0), (T, dtype, prof)
    pwl = _lifted(spec) and spec.bn_mode == "population" and "CHIRON_NO_PWL" not in env
    assert prof.get("conv1_pwl", 0) == (1 if pwl else 0), (T, dtype, prof)
    if _lifted(spec) and not pwl and spec.bn_mode == "population":
        assert prof.get("conv_lift", 0) == 1, prof             # conv2a materialised, conv2b on the GEMM
    assert "ctc_beam" not in prof


def _reference(spec, w, x, sl, T, stem_or_short):
    from oracle import c_oracle, nn_oracle
    if spec.stem:                                              # the C oracle covers the shipped topologies only
        return nn_oracle.inference(x, sl, spec.to_dict(), w, dtype=np.float64)[0], None
    cref = c_oracle.forward(x, sl, spec.to_dict(), spec.pack(w), T)
    ref64 = nn_oracle.inference(x, sl, spec.to_dict(), w, dtype=np.float64)[0] if stem_or_short else None
    return cref, ref64


def _run(spec, w, x, sl, L, max_batch, dtype="fp32", max_beam=0, profile=True):
    eng = ca.Engine(spec, w, max_batch=max_batch, segment_len=L, dtype=dtype, max_beam=max_beam)
    if profile:
        eng.profile(True)
    res = eng.infer(x, sl, want_prob=True, want_logits=True)
    prof = _profile_launches(eng) if profile else None
    return eng, res, prof


@pytest.mark.parametrize("row", _ROWS, ids=[_row_id(r) for r in _ROWS])
def test_geometry_sweep_against_the_oracle(models, clean_env, row):
    topology, L, B, max_batch, beam = row
    spec, w = models[topology]
    x, sl, T = _ragged(spec, L, B, seed=1000 + L + 7 * B)
    ref, ref64 = _reference(spec, w, x, sl, T, T <= 64)
    outs = {}
    for dtype in ("fp32", "fp32-split"):
        eng, res, prof = _run(spec, w, x, sl, L, max_batch, dtype=dtype, max_beam=50 if beam and dtype == "fp32" else 0)
        try:
            assert eng.T == T and eng.ratio == L / T
            assert res.logits.shape == (B, T, spec.classes)
            _expect_forms(spec, prof, T, dtype)
            err = np.abs(res.logits.astype(np.float64) - ref).max()
            assert err < TOL, (dtype, err)
            if ref64 is not None:
                assert np.abs(res.logits.astype(np.float64) - ref64).max() < TOL, dtype
            _check_decode(res, res.logits, sl, B)
            outs[dtype] = res.logits.copy()
            if beam and dtype == "fp32":
                for bw in (5, 50):
                    eng.profile(True)
                    r = eng.infer(x, sl, beam_width=bw, want_prob=True, want_logits=True)
                    assert _profile_launches(eng).get("ctc_beam", 0) == 1
                    assert np.array_equal(r.logits, res.logits)
                    _check_beam(r, r.logits, sl, bw, B)
        finally:
            eng.close()
    if T < 32 or _ROWS.index(row) % 3 == 0:
        mask = (np.arange(T)[None, :] < sl[:, None])[..., None]
        for dtype in ("fp16", "fp16-w2"):
            eng, res, _ = _run(spec, w, x, sl, L, max_batch, dtype=dtype, profile=False)
            eng.close()
            assert np.isfinite(res.logits).all(), dtype
            assert (np.abs(res.logits - outs["fp32"]) * mask).max() < F16_TOL, dtype


def test_every_conv2b_form_is_in_the_sweep():
    """the table above reaches the direct form, F(2,3) and F(4,3) on every topology with a Winograd-eligible block, every left pad
    of the strided first block and of both stems, and beam rows on short and odd windows"""
    forms = {}
    for topology, L, B, mb, beam in _ROWS:
        spec = ca.dna_default_spec() if topology == "dna" else ca.rna_default_spec() if topology == "rna" else ca.rna_head_spec(topology)
        T = spec.output_len(L)
        f = "direct" if T % 2 else "f4" if T % 4 == 0 and T >= 256 else "f2"
        forms.setdefault(topology, set()).add(f)
    assert forms["dna"] == forms["rna"] == {"direct", "f2", "f4"}
    assert forms["rna_model2"] >= {"f2", "f4"} and forms["rna_model3"] >= {"f2", "direct"}
    for topology, stride in (("rna", 5), ("rna_model2", 5), ("rna_model3", 7)):
        assert {L % stride for t, L, _, _, _ in _ROWS if t == topology} == set(range(stride)), topology
    assert {(t, L) for t, L, _, _, beam in _ROWS if beam} >= {("dna", 1), ("dna", 2), ("dna", 3), ("rna", 501)}


# forced forms: (topology, L, B, switch) -- the default hides the form, the switch forces it; each result goes to the oracle
_FORCED = [
    ("dna", 4, 5, "CHIRON_WINOGRAD_F4"),     # one quad per window: first AND last quad
    ("dna", 8, 3, "CHIRON_WINOGRAD_F4"),     # two quads per window
    ("dna", 12, 7, "CHIRON_WINOGRAD_F4"),    # 21 quads
    ("dna", 64, 3, "CHIRON_WINOGRAD_F4"),
    ("dna", 252, 2, "CHIRON_WINOGRAD_F4"),   # just below the default threshold
    ("dna", 256, 3, "CHIRON_WINOGRAD_F2"),   # F(2,3) where the default takes F(4,3)
    ("dna", 400, 3, "CHIRON_WINOGRAD_F2"),
    ("dna", 130, 3, "CHIRON_NO_WINOGRAD"),   # direct GEMM at an even length
    ("dna", 256, 2, "CHIRON_NO_WINOGRAD"),
    ("rna", 1, 3, "CHIRON_NO_PWL"),          # lifted conv2a + strided GEMM conv2b, every left pad
    ("rna", 12, 3, "CHIRON_NO_PWL"),
    ("rna", 13, 2, "CHIRON_NO_PWL"),
    ("rna", 14, 3, "CHIRON_NO_PWL"),
    ("rna", 156, 3, "CHIRON_NO_PWL"),
    ("rna", 157, 2, "CHIRON_NO_PWL"),
    ("rna", 158, 3, "CHIRON_NO_PWL"),
    ("rna", 159, 2, "CHIRON_NO_PWL"),
    ("rna", 160, 3, "CHIRON_NO_PWL"),
    ("rna", 2000, 2, "CHIRON_NO_PWL"),       # the rna-pre window
]


@pytest.mark.parametrize("row", _FORCED, ids=["%s-L%d-%s" % (r[0], r[1], r[3][7:].lower()) for r in _FORCED])
def test_forced_forms_against_the_oracle(models, clean_env, row):
    """each forced form within 1e-4 of the C oracle, its profile showing the form, and its bits different from the default's
    (a switch that is silently ignored fails here)"""
    topology, L, B, switch = row
    spec, w = models[topology]
    x, sl, T = _ragged(spec, L, B, seed=2000 + L)
    ref, ref64 = _reference(spec, w, x, sl, T, T <= 64)
    eng, base, _ = _run(spec, w, x, sl, L, B)
    eng.close()
    clean_env.setenv(switch, "1")
    eng, res, prof = _run(spec, w, x, sl, L, B)
    eng.close()
    clean_env.delenv(switch)
    _expect_forms(spec, prof, T, env=(switch,))
    for out in (base, res):
        assert np.abs(out.logits.astype(np.float64) - ref).max() < TOL, switch
        if ref64 is not None:
            assert np.abs(out.logits.astype(np.float64) - ref64).max() < TOL, switch
    _check_decode(res, res.logits, sl, B)
    assert not np.array_equal(res.logits, base.logits), "%s at T = %d gave the default form's bits" % (switch, T)


@pytest.mark.parametrize("T,B", [(1, 1), (1, 5), (3, 1), (3, 5), (33, 1), (33, 5), (258, 1), (258, 5)])
def test_batch_statistics_bn_at_odd_and_short_lengths(built, clean_env, T, B):
    """batch-statistics BN (HEAD's simple_global_bn) on the DNA topology at odd and one-frame windows: the moments of this batch
    only, against the float64 oracle on the same batch; B = 1, T = 1 is the zero-variance edge (one position per channel)"""
    from oracle import nn_oracle
    spec = ca.dna_default_spec(bn_mode="batch")
    w = ca.synthetic_weights(spec, seed=71)
    x, sl, _ = _ragged(spec, T, B, seed=3000 + T + B)
    eng, res, prof = _run(spec, w, x, sl, T, B + 3)
    eng.close()
    _expect_forms(spec, prof, T)
    ref, _ = nn_oracle.inference(x, sl, spec.to_dict(), w, dtype=np.float64)
    assert np.abs(res.logits.astype(np.float64) - ref).max() < TOL
    _check_decode(res, res.logits, sl, B)


@pytest.mark.parametrize("T", [8191, 8192])
def test_beam_kernel_switch_at_8192_frames(built, clean_env, T):
    """beam.hip picks its register kernels (beam32x2_kernel, beam64_kernel) only below 8192 frames (the depth field of their
    packed entries) and the generic walk from there on: both sides, widths 30, 64 and 100, bit-exact against the C oracle; width
    30 again with two windows per wave (CHIRON_BEAM_SINGLE=0: beam32x2_kernel, which a batch below 512 does not take by default)"""
    spec = ca.dna_default_spec()
    w = ca.synthetic_weights(spec, seed=72)
    rng = np.random.RandomState(T)
    B = 4
    lg = (rng.randn(B, T, 5) * 2.0).astype(np.float32)
    lg[..., 4] += 1.0                                     # blank-leaning, long emissions
    sl = np.asarray([T, T - 1, 1, rng.randint(2, T)], np.int32)
    with ca.Engine(spec, w, max_batch=B, segment_len=T, max_beam=100) as eng:
        assert eng.T == T
        for bw, single in ((30, None), (64, None), (100, None), (30, "0")):
            if single is not None:
                clean_env.setenv("CHIRON_BEAM_SINGLE", single)
            eng.profile(True)
            r = eng.decode(lg, sl, beam_width=bw)
            assert _profile_launches(eng).get("ctc_beam", 0) == 1
            clean_env.delenv("CHIRON_BEAM_SINGLE", raising=False)
            _check_beam(r, lg, sl, bw, B)
