"""GPU: chiron_demux_windows (csrc/demux.hip) through chiron_amd.demux against the numpy column DP of tests/demux_ref.py, and `demux`
end to end.  Everything is an integer: every comparison is exact."""
import filecmp
import os
import subprocess
import sys

import numpy as np
import pytest

from chiron_amd import assess, demux, map as cmap

import demux_cases as cases
import demux_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW_KEYS = ("best", "dist", "end", "second")


def _check(windows, patterns, groups, want_matrix=True, want=None):
    """One call against the reference, every window and (with the matrix) every pair.  -> the GPU's result."""
    got = demux.match_call(windows, patterns, groups, want_matrix=want_matrix)
    want = want or ref.match(windows, patterns, groups, want_matrix=want_matrix)
    for k in WINDOW_KEYS + (("pair_dist", "pair_end") if want_matrix else ()):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, (k, len(patterns), bad[:5].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])
    return got


def test_edge_cases_in_one_launch(built):
    windows, patterns, groups = cases.edge_case()
    assert sorted({len(p) for p in patterns}) == [1, 2, 31, 32, 33, 63, 64]
    assert sorted({len(w) for w in windows}) == [0, 1, 2, 63, 64, 65, 79, 150, 4096]
    got = _check(windows, patterns, groups)
    full = 6                                                   # the 64-base pattern: its own copy, and the copy with one base gone
    assert (got["pair_dist"][-3, full], got["pair_end"][-3, full]) == (0, 64)
    assert (got["pair_dist"][-2, full], got["pair_end"][-2, full]) == (1, 63)
    assert got["pair_dist"][-1, full] <= 1
    # planted exact copies: at the window's start the end is n (or earlier, when a prefix of the window happens to do as well),
    # at the window's end it is m unless the pattern already occurs before
    assert (got["pair_dist"] >= 0).all() and (got["pair_end"] <= np.array([len(w) for w in windows])[:, None]).all()


@pytest.mark.parametrize("patterns", [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 128, 129, 130])
def test_every_lane_map(built, patterns):
    """37 windows -- no multiple of any slot count -- of 0 to 40 bases mixed within a wave, patterns of 1 to 24 bases in
    several groups, some of them spellings of one barcode."""
    rng = np.random.default_rng(700 + patterns)
    pats = [cases.random_codes(int(rng.integers(1, 25)), rng, with_n=q % 7 == 3) for q in range(patterns)]
    groups = rng.integers(0, max(patterns // 2, 1) + 1, patterns).astype(np.int32)
    windows = [cases.random_codes(int(rng.integers(0, 41)), rng, with_n=w % 5 == 2) for w in range(37)]
    for w in range(0, 37, 3):                                  # plant a mutated pattern so that the best is not noise
        p = pats[int(rng.integers(0, patterns))]
        if len(windows[w]) >= len(p):
            at = int(rng.integers(0, len(windows[w]) - len(p) + 1))
            windows[w][at:at + len(p)] = p
    got = _check(windows, pats, groups)
    if len(set(groups.tolist())) == 1:
        assert (got["second"] == demux.NONE).all()


@pytest.mark.parametrize("patterns", [1, 70])
def test_more_windows_than_the_launch_has_wave_slots(built, patterns):
    """One launch holds MAX_GROUPS workgroups of THREADS / 64 waves of 64 / P2 window slots; 1000 windows more than that make some
    waves take a second slot group."""
    rng = np.random.default_rng(800 + patterns)
    p2 = 1
    while p2 < min(patterns, 64):
        p2 *= 2
    count = demux.MAX_GROUPS * (demux.THREADS // 64) * (64 // p2) + 1000
    pats = [cases.random_codes(int(rng.integers(1, 9)), rng) for _ in range(patterns)]
    groups = (np.arange(patterns) % 3).astype(np.int32)
    lens = rng.integers(0, 13, count)
    flat = cases.random_codes(int(lens.sum()), rng, with_n=True)
    windows = np.split(flat, np.cumsum(lens)[:-1])
    _check(windows, pats, groups, want_matrix=patterns == 70)


def test_a_window_depends_on_itself_alone(built):
    rng = np.random.default_rng(900)
    pats = [cases.random_codes(24, rng) for _ in range(12)]
    groups = np.arange(12, dtype=np.int32)
    windows = [cases.random_codes(int(rng.integers(0, 151)), rng) for _ in range(50)]
    batch = demux.match_call(windows, pats, groups, want_matrix=True)
    plain = demux.match_call(windows, pats, groups)
    back = demux.match_call(windows[::-1], pats, groups, want_matrix=True)
    planned = demux.match_windows(windows, pats, groups, workspace_mb=demux.workspace_size(25, 25 * 150, 12) / (1 << 20))
    assert planned["calls"] >= 2
    for k in WINDOW_KEYS:
        assert np.array_equal(batch[k], plain[k]) and np.array_equal(batch[k], back[k][::-1]) and np.array_equal(batch[k], planned[k]), k
    assert np.array_equal(batch["pair_dist"], back["pair_dist"][::-1]) and np.array_equal(batch["pair_end"], back["pair_end"][::-1])
    for w in (0, 17, 49):
        alone = demux.match_call([windows[w]], pats, groups, want_matrix=True)
        for k in WINDOW_KEYS + ("pair_dist", "pair_end"):
            assert np.array_equal(alone[k][0], batch[k][w]), (k, w)


def test_distance_equals_the_infix_kernels(built):
    rng = np.random.default_rng(950)
    pats = [cases.random_codes(n, rng) for n in (1, 24, 33, 64)]
    windows = [cases.random_codes(m, rng) for m in (0, 30, 150, 150, 400)]
    windows[2][40:64] = pats[1]
    windows[3][100:164 - 14] = pats[3][:50]
    got = demux.match_call(windows, pats, np.arange(4, dtype=np.int32), want_matrix=True)
    pairs = [(q, w) for q in range(4) for w in range(5)]
    infix = cmap.align_infix([pats[q] for q, _ in pairs], [windows[w] for _, w in pairs])
    assert [int(got["pair_dist"][w, q]) for q, w in pairs] == infix["edit"].tolist()


def _tree(folder):
    return sorted(os.path.relpath(os.path.join(d, f), folder) for d, _, fs in os.walk(folder) for f in fs)


def test_demux_command_end_to_end(built, tmp_path):
    """The planted run through `chiron demux` in a process of its own: the output tree is byte for byte the one the command writes
    with the numpy reference in the kernel's place, and a bin file is a valid input of assess."""
    case = cases.planted()
    reads, barcodes = cases.write_planted(case, str(tmp_path))
    want_dir, got_dir = str(tmp_path / "want"), str(tmp_path / "got")
    want = demux.demux_command(reads, barcodes, want_dir, matcher=lambda w, p, g: ref.match(w, p, g))
    run = subprocess.run([sys.executable, "-m", "chiron_amd.entry", "demux", "-i", reads, "--barcodes", barcodes, "-o", got_dir],
                         cwd=ROOT, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert "demux: 300 reads against 12 patterns; %d classified" % want["status"]["classified"] in run.stdout
    assert _tree(got_dir) == _tree(want_dir) and "demux.tsv" in _tree(got_dir) and len(_tree(got_dir)) >= 12
    match, mismatch, errors = filecmp.cmpfiles(want_dir, got_dir, _tree(want_dir), shallow=False)
    assert not mismatch and not errors, (mismatch, errors)
    name = max(want["bins"], key=want["bins"].get)
    loaded = assess.load_reads(os.path.join(got_dir, name + ".fastq"))
    assert len(loaded) == want["bins"][name] >= 2 and all(set(s) <= set("ACGT") for s in loaded.values())
