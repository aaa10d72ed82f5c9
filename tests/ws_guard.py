"""Poisoned, exactly sized, guarded memory for the calls that compute in memory their caller hands them.

A Recorder is what chiron_amd._lib.alloc_hook takes (set it with monkeypatch, never globally).  For a byte buffer of n bytes it
allocates GUARD + n + GUARD bytes, fills all of them with one byte value and hands out the interior [GUARD : GUARD + n]; for a
typed output it hands out a tensor whose every byte is the fill.  check() then asserts that both guards of every buffer still
hold the fill: a call that writes past the bytes its size function names is seen, and never leaves the allocation.  Call
check() only after the stream is synchronised.

GUARD is 1 MiB: a multiple of 512, so the interior keeps the allocator's alignment, and more than any single workspace row or
LDS-spill row the kernels address, so an overrun by a whole row still lands inside the block.

The fills: 0x00; 0xFF, a NaN as f16 / f32 / f64, -1 as any integer, all ones as a bit-vector word; 0x7F, a huge finite float or
double (3.4e38 / 1.4e306) and a huge positive integer.  A min, a max, a sum or a bit automaton that touches a word nobody wrote
changes its answer under at least two of the three.

Plain torch, no GPU needed: tests/test_ws_guard_cpu.py runs it on CPU tensors.
"""
import torch

GUARD = 1 << 20
FILLS = (0x00, 0xFF, 0x7F)


class _NoBytes(object):
    """The interior of a block of zero bytes.  torch gives an empty view a null data_ptr(); the library is owed a valid pointer
    (between the two guards), so this stands in for the view with what the wrappers use of it."""
    dtype, shape = torch.uint8, torch.Size([0])

    def __init__(self, block):
        self.block = block
        self.device = block.device

    def data_ptr(self):
        return self.block.data_ptr() + GUARD

    def numel(self):
        return 0

    def record_stream(self, stream):
        self.block.record_stream(stream)


class Recorder(object):
    def __init__(self, fill):
        assert 0 <= fill <= 0xFF and GUARD % 512 == 0
        self.fill = fill
        self.blocks = []            # (whole block, n) of every byte buffer handed out, in order
        self.outputs = []           # every typed output handed out, in order

    def byte_buffer(self, nbytes, device):
        assert nbytes >= 0
        block = torch.full((GUARD + nbytes + GUARD,), self.fill, dtype=torch.uint8, device=device)
        self.blocks.append((block, nbytes))
        return block[GUARD:GUARD + nbytes] if nbytes else _NoBytes(block)

    def output(self, shape, dtype, device):
        n = 1
        for s in shape:
            n *= int(s)
        raw = torch.full((n * torch.empty((), dtype=dtype).element_size(),), self.fill, dtype=torch.uint8, device=device)
        out = raw.view(dtype).view(*shape) if n else torch.empty(shape, dtype=dtype, device=device)
        self.outputs.append(out)
        return out

    @property
    def sizes(self):
        """The byte counts asked for, in order."""
        return [n for _, n in self.blocks]

    def interior(self, i):
        block, n = self.blocks[i]
        return block[GUARD:GUARD + n]

    def check(self):
        """Every guard byte of every buffer still holds the fill; else AssertionError naming the changed byte nearest the region:
        `start-k` is k bytes before its first byte, `end+k` is k bytes past its last one's successor (end+0 is the first byte past)."""
        for i, (block, n) in enumerate(self.blocks):
            before = torch.nonzero(block[:GUARD] != self.fill)
            assert before.numel() == 0, "buffer %d of %d bytes: start-%d was written (%d guard bytes changed before the region)" % (
                i, n, GUARD - int(before[-1]), before.numel())
            after = torch.nonzero(block[GUARD + n:] != self.fill)
            assert after.numel() == 0, "buffer %d of %d bytes: end+%d was written (%d guard bytes changed after the region)" % (
                i, n, int(after[0]), after.numel())


def still_filled(t, fill):
    """Elements of `t` whose every byte is still the fill byte (0 for an empty tensor)."""
    if t.numel() == 0:
        return 0
    raw = t.contiguous().view(-1).view(torch.uint8).view(t.numel(), -1)
    return int((raw == fill).all(dim=1).sum())
