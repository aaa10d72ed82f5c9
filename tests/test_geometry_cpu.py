"""CPU pins of the window geometry (no GPU): the frame count the engine plans for every segment length, and the C oracle
against the float64 numpy oracle at the geometries tests/test_gpu_geometry.py compares the device with (the C oracle covers
the shipped topologies; the sweep holds the HEAD stem models to the numpy oracle directly).

The GPU geometry sweep holds the device to c_oracle.forward; these tests pin the C oracle itself there first -- at every
residue of L mod 5 (every SAME left pad of the strided first block), at L below the kernel
width and at a single frame."""
import numpy as np
import pytest

import chiron_amd as ca
from oracle import nn_oracle as no

_TOPOLOGIES = {"dna": ca.dna_default_spec, "rna": ca.rna_default_spec,
               "rna_model2": lambda: ca.rna_head_spec("rna_model2"), "rna_model3": lambda: ca.rna_head_spec("rna_model3")}


def _same_padding_chain(spec, L):
    t = L
    if spec.stem:
        t = no.same_padding(t, spec.stem["k"], spec.stem["stride"])[0]
    for b in spec.blocks:
        t = no.same_padding(t, b["k"], b["stride"])[0]
    return t


@pytest.mark.parametrize("topology", sorted(_TOPOLOGIES))
def test_planned_frames_follow_same_padding_for_every_length(built, topology):
    """chiron_engine_plan's T and ratio for every segment length 1 .. 6000: equal to ModelSpec.output_len and to the chain
    of TF SAME paddings over the stem and the blocks (what the oracle's convolutions produce)."""
    from chiron_amd.engine import plan_sizes
    spec = _TOPOLOGIES[topology]()
    for L in range(1, 6001):
        p = plan_sizes(spec, 1, L)
        T = spec.output_len(L)
        assert p["T"] == T == _same_padding_chain(spec, L), (topology, L, p["T"], T)
        assert p["ratio"] == L / T, (topology, L, p["ratio"])


# (topology, segment lengths): every residue of L mod stride around one frame count below 256 and one above it, L below the
# first kernel's width, and the short lengths of the DNA sweep
_ORACLE_GEOMETRIES = [
    ("dna", [1, 2, 3, 5, 33]),
    ("rna", [1, 3, 5, 6, 12, 13, 14] + list(range(156, 161)) + list(range(496, 502))),
    ("rna", list(range(1276, 1282)) + list(range(1996, 2002)) + [2500]),
]


@pytest.mark.parametrize("topology,lengths", _ORACLE_GEOMETRIES, ids=["%s-%d" % (g[0], i) for i, g in enumerate(_ORACLE_GEOMETRIES)])
def test_c_oracle_matches_numpy_oracle_at_every_left_pad(built, topology, lengths):
    """c_oracle.forward against nn_oracle.inference in float64 within 5e-5 (the bar of test_c_oracle_matches_numpy_oracle at
    400 / 500), ragged rows including seq_len 0, 1 and T, signal zeroed past each row's samples."""
    from oracle import c_oracle
    spec = _TOPOLOGIES[topology]()
    w = ca.synthetic_weights(spec, seed=41)
    for L in lengths:
        T = spec.output_len(L)
        sl = np.asarray([T, min(1, T), 0, T // 2], np.int32)
        B = sl.size
        x = ca.synthetic_signal(1, B * L, seed=L)[0].reshape(B, L).copy()
        for b in range(B):
            x[b, int(np.ceil(sl[b] * L / T)):] = 0
        ref, ratio = no.inference(x, sl, spec.to_dict(), w, dtype=np.float64)
        assert ref.shape == (B, T, spec.classes) and ratio == L / T
        got = c_oracle.forward(x, sl, spec.to_dict(), spec.pack(w), T)
        err = np.abs(got - ref).max()
        assert err < 5e-5, (topology, L, err)
