"""CPU: the guard and poison helper of tests/ws_guard.py does what tests/test_gpu_workspace.py relies on, and the allocation seam
of chiron_amd._lib is today's torch.empty while no hook is set."""
import re

import pytest
import torch

from chiron_amd import _lib

import ws_guard
from ws_guard import FILLS, GUARD, Recorder

CPU = torch.device("cpu")


def _whole(rec, i=0):
    return rec.blocks[i][0]


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("n", [0, 1, 7, 512, 1000])
def test_a_buffer_is_exact_filled_and_guarded(fill, n):
    rec = Recorder(fill)
    buf = rec.byte_buffer(n, CPU)
    whole = _whole(rec)
    assert buf.dtype == torch.uint8 and buf.numel() == n and whole.numel() == GUARD + n + GUARD
    assert buf.data_ptr() == whole.data_ptr() + GUARD and buf.data_ptr() != 0          # n = 0 included: a pointer into the block
    assert bool((whole == fill).all())                                                  # the interior and both guards
    assert rec.sizes == [n]
    rec.check()


@pytest.mark.parametrize("fill", FILLS)
def test_a_write_next_to_the_region_is_reported_with_its_offset(fill):
    n = 1000
    other = fill ^ 0x55
    for at, said in ((GUARD - 1, "start-1"), (GUARD + n, r"end\+0"), (GUARD - 700, "start-700"), (GUARD + n + 123, r"end\+123"), (0, "start-%d" % GUARD),
                     (2 * GUARD + n - 1, r"end\+%d" % (GUARD - 1))):
        rec = Recorder(fill)
        rec.byte_buffer(n, CPU)
        _whole(rec)[at] = other
        with pytest.raises(AssertionError, match=r"buffer 0 of 1000 bytes: %s was written" % said):
            rec.check()
    rec = Recorder(fill)                   # of several changed bytes the one nearest the region is named
    rec.byte_buffer(n, CPU)
    _whole(rec)[GUARD - 9:GUARD - 3] = other
    with pytest.raises(AssertionError, match=re.escape("start-4 was written (6 guard bytes")):
        rec.check()
    _whole(rec)[GUARD - 9:GUARD - 3] = fill
    _whole(rec)[GUARD + n + 5:GUARD + n + 8] = other
    with pytest.raises(AssertionError, match=re.escape("end+5 was written (3 guard bytes")):
        rec.check()


@pytest.mark.parametrize("fill", FILLS)
def test_a_write_inside_the_region_is_not_reported(fill):
    rec = Recorder(fill)
    buf = rec.byte_buffer(1000, CPU)
    buf[0] = fill ^ 0xFF
    buf[999] = fill ^ 0xFF
    buf[1:999] = 0x33
    rec.check()
    assert rec.interior(0).data_ptr() == buf.data_ptr() and int(rec.interior(0)[0]) == fill ^ 0xFF


@pytest.mark.parametrize("fill", FILLS)
def test_every_allocation_is_checked(fill):
    rec = Recorder(fill)
    bufs = [rec.byte_buffer(n, CPU) for n in (64, 0, 4096)]
    assert rec.sizes == [64, 0, 4096] and len({b.data_ptr() for b in bufs}) == 3
    rec.check()
    for i in range(3):
        _whole(rec, i)[GUARD + rec.sizes[i]] = fill ^ 1
        with pytest.raises(AssertionError, match=r"buffer %d of %d bytes: end\+0" % (i, rec.sizes[i])):
            rec.check()
        _whole(rec, i)[GUARD + rec.sizes[i]] = fill
    rec.check()


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.int32, torch.uint8])
def test_a_typed_output_is_the_fill_in_every_byte(fill, dtype):
    rec = Recorder(fill)
    out = rec.output((3, 5, 2), dtype, CPU)
    assert out.shape == (3, 5, 2) and out.dtype == dtype and out.is_contiguous() and rec.outputs[0] is out
    assert bool((out.view(-1).view(torch.uint8) == fill).all())
    assert ws_guard.still_filled(out, fill) == 30
    if dtype.is_floating_point:
        assert bool(torch.isnan(out).all()) == (fill == 0xFF)
        assert bool(torch.isfinite(out).all()) == (fill != 0xFF)
        if fill == 0x7F:
            assert float(out.min()) > (3e38 if dtype == torch.float32 else 1e306)
    else:
        want = {0x00: 0, 0xFF: 255 if dtype == torch.uint8 else -1, 0x7F: 0x7F if dtype == torch.uint8 else 0x7F7F7F7F}[fill]
        assert bool((out == want).all())
    out.view(-1)[7] = 1
    assert ws_guard.still_filled(out, fill) == 29
    empty = rec.output((0, 5), dtype, CPU)
    assert empty.shape == (0, 5) and ws_guard.still_filled(empty, fill) == 0


def test_f16_reads_0xff_as_nan():
    raw = torch.full((8,), 0xFF, dtype=torch.uint8)
    assert bool(torch.isnan(raw.view(torch.float16)).all())


def test_without_a_hook_the_seam_is_torch_empty():
    assert _lib.alloc_hook is None
    for n, floor, want in ((0, 256, 256), (10, 256, 256), (256, 256, 256), (1000, 256, 1000), (0, 4, 4), (3, 0, 3), (0, 0, 0)):
        buf = _lib.device_bytes(n, CPU, at_least=floor)
        assert buf.dtype == torch.uint8 and buf.shape == (want,) and buf.device == CPU
    assert _lib.device_bytes(77, CPU).shape == (77,)
    out = _lib.device_output((4, 3, 5), torch.float32, CPU)
    assert out.shape == (4, 3, 5) and out.dtype == torch.float32 and out.is_contiguous()
    assert _lib.device_output(torch.Size([6]), torch.int32, CPU).shape == (6,)


def test_with_a_hook_the_seam_passes_the_exact_request(monkeypatch):
    rec = Recorder(0x7F)
    monkeypatch.setattr(_lib, "alloc_hook", rec)
    buf = _lib.device_bytes(10, CPU, at_least=256)                # the minimum is not applied: the hook sees what the call needs
    assert buf.shape == (10,) and rec.sizes == [10] and bool((buf == 0x7F).all())
    assert _lib.device_bytes(0, CPU, at_least=4).shape == (0,) and rec.sizes == [10, 0]
    out = _lib.device_output((2, 5), torch.float64, CPU)
    assert out is rec.outputs[0] and out.shape == (2, 5) and out.dtype == torch.float64 and float(out.min()) > 1e306
    rec.check()
    monkeypatch.undo()
    assert _lib.alloc_hook is None
