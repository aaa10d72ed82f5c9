"""GPU: chiron_consensus_device (csrc/consensus.hip: displacements, start scan, vote) on the reads of tests/consensus_cases.py --
overlaps of up to 39 bases, the clamp by a short segment, ties of the glue score, empty segments, segment counts around the scan's
1024-segment chunks, a longest segment owned by a later chunk -- against the plain restatement tests/consensus_ref.py, exactly: the
raw consensus, n1, n2, q_top (bit for bit) and the length, through the library's own entry point.  Then once more against the host
path, and as strings through assembly.consensus_device."""
import ctypes as C

import numpy as np
import pytest

from chiron_amd import _lib, assembly, eval as ce

import consensus_cases
import consensus_host

pytestmark = pytest.mark.gpu


def device_consensus(segments, qs, kernal):
    """-> (consensus uint8, n1 int32, n2 int32, q_top float64, out_len), the arrays cut to out_len"""
    bases, off = assembly.encode(segments)
    qs = np.ascontiguousarray(qs, dtype=np.float64)
    cap = int(bases.shape[0]) + 1
    cons = np.full(cap, 255, dtype=np.uint8)
    n1, n2, q_top = np.full(cap, -7, dtype=np.int32), np.full(cap, -7, dtype=np.int32), np.full(cap, np.nan)
    n = C.c_int64(-1)
    _lib.check(_lib.load().chiron_consensus_device(0, bases.ctypes.data, off.ctypes.data, len(segments), qs.ctypes.data, assembly.KERNALS[kernal],
                                                   cons.ctypes.data, n1.ctypes.data, n2.ctypes.data, q_top.ctypes.data, cap, C.byref(n)))
    k = n.value
    assert 0 <= k <= cap and (cons[k:] == 255).all() and (n1[k:] == -7).all() and (n2[k:] == -7).all() and np.isnan(q_top[k:]).all()
    return cons[:k], n1[:k], n2[:k], q_top[:k], k


@pytest.fixture(scope="module")
def device(built):
    return {(name, kernal): device_consensus(segs, qs, kernal) for name, segs, qs, kernal in consensus_cases.cases()}


@pytest.fixture(scope="module")
def ref():
    return consensus_host.reference()


def test_device_consensus_equals_the_restatement(built, device, ref):
    assert len(device) == 2 * len(consensus_cases.names()) - len(consensus_cases.GLUE_ONLY)
    for name, segs, qs, kernal in consensus_cases.cases():
        want = ref[name, kernal]
        cons, n1, n2, q_top, length = device[name, kernal]
        assert length == want["length"], (name, kernal)
        assert np.array_equal(cons, want["base"]), (name, kernal, np.flatnonzero(cons != want["base"])[:5])
        assert np.array_equal(n1, want["n1"]) and np.array_equal(n2, want["n2"]), (name, kernal)
        assert q_top.tobytes() == want["q_top"].tobytes(), (name, kernal)


def test_device_consensus_equals_the_host_path(built, device):
    for name, segs, qs, kernal in consensus_cases.cases():
        base, h1, h2, hq, _, _ = consensus_host.host_consensus(segs, qs, kernal)
        cons, n1, n2, q_top, length = device[name, kernal]
        assert length == base.shape[0], (name, kernal)
        assert np.array_equal(cons, base) and np.array_equal(n1, h1) and np.array_equal(n2, h2), (name, kernal)
        assert q_top.tobytes() == np.asarray(hq, dtype=np.float64).tobytes(), (name, kernal)


def test_device_consensus_strings_without_qualities(built, ref):
    for name, segs, qs, kernal in consensus_cases.cases():
        want = ce.index2base(ref[name, kernal]["base"])
        assert assembly.consensus_device(segs, None, kernal) == (want, None), (name, kernal)
