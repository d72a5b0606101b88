"""Buffers at chosen device addresses, for tests/test_address_range_gpu.py (a helper module, not a conftest).

One torch.uint8 arena of 8 GiB always contains an address B that is 0 mod 2^32 with at least 1 GiB on either side
(boundary_in).  A Placer hands out 16-byte aligned, contiguous, typed views of the arena:

  bit31     the whole buffer lies below B inside [B - 2 GiB, B): bit 31 of every one of its addresses is set
            (bump allocation, 256-byte aligned);
  straddle  B falls on a chosen element of the buffer (rounded down to 16 bytes), so a carry into bit 32 happens
            inside the touched data.  One role of a launch at a time; the others stay at bit31.

Every view has a guard band of 64 KiB on both sides, filled with a byte pattern when the view is made and compared by
check_guards().  Plain is the control: ordinary torch allocations behind the same two calls, which is also what the
launch helpers of the three route files do when no allocator is passed.

The address arithmetic (boundary_in, straddle_start) is plain integer code: tests/test_address_range_cpu.py runs it
without a GPU."""
from __future__ import annotations

import torch

GIB = 1 << 30
LINE = 1 << 32
ARENA_BYTES = 8 * GIB
GUARD = 64 * 1024
PATTERN = 0xA5


def boundary_in(base: int, nbytes: int = ARENA_BYTES) -> int:
    """The multiple of 2^32 inside [base, base + nbytes) with at least 1 GiB of the arena on either side."""
    b = -(-base // LINE) * LINE
    if b - base < GIB:
        b += LINE
    assert b - base >= GIB and base + nbytes - b >= GIB, (hex(base), nbytes)
    return b


def straddle_start(boundary: int, elem_off: int, itemsize: int, nbytes: int) -> int:
    """Start address of a buffer of nbytes such that `boundary` falls on its element elem_off, rounded down to 16
    bytes (at least 16 bytes of the buffer lie below the boundary if it has that many)."""
    off = (elem_off * itemsize) // 16 * 16
    if off == 0 and nbytes > 16:
        off = 16
    return boundary - off


def mid(row_lo: int, nrows: int, ld: int, col_lo: int, ncols: int) -> int:
    """Flat element index of the middle column of the middle row of a [row_lo, row_lo + nrows) x [col_lo, col_lo + ncols)
    block of a row-major buffer with row stride ld: where a straddling placement puts the boundary."""
    return (row_lo + nrows // 2) * ld + col_lo + ncols // 2


class Plain:
    """Ordinary torch allocations (the control, and the launch helpers' default)."""
    straddle = None

    def __init__(self, dev="cuda"):
        self.dev = dev

    def to(self, t, roles=None):
        return t.to(self.dev)

    def full(self, shape, fill, dtype, roles=None):
        return torch.full(tuple(shape), fill, device=self.dev, dtype=dtype)

    def check_guards(self):
        pass


class Arena:
    def __init__(self, dev="cuda", nbytes: int = ARENA_BYTES):
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.nbytes = nbytes
        self.base = self.buf.data_ptr()
        self.B = boundary_in(self.base, nbytes)
        self.lo = max(self.base, self.B - 2 * GIB)      # bit 31 is set in [lo, B)

    def placer(self, straddle=None):
        return Placer(self, straddle)

    def window(self, start: int, nbytes: int):
        """uint8 view of the absolute addresses [start, start + nbytes)."""
        o = start - self.base
        assert 0 <= o and o + nbytes <= self.nbytes, (hex(start), nbytes)
        return self.buf[o:o + nbytes]


class Placer:
    """One launch's buffers.  `straddle` names the role whose buffer is put across the boundary; every other buffer
    (all of them with straddle=None) lies in the bit-31 region.  roles = {role: flat element index where the boundary
    goes if that role straddles (None: the middle of the buffer's middle row)}."""

    def __init__(self, arena: Arena, straddle=None):
        self.arena = arena
        self.straddle = straddle
        self.next = arena.lo
        self.guards = []          # absolute start addresses of the guard bands
        self.placed = {}          # role -> (start address, nbytes)
        self.floor = arena.B      # lowest address used by a straddling buffer (with its guard)

    def _carve(self, shape, dtype, roles):
        a = self.arena
        shape = tuple(shape)
        n = 1
        for s in shape:
            n *= s
        item = torch.empty((), dtype=dtype).element_size()
        nbytes = n * item
        if nbytes == 0:
            return torch.empty(shape, dtype=dtype, device=a.buf.device)
        roles = roles or {}
        if self.straddle is not None and self.straddle in roles:
            e = roles[self.straddle]
            if e is None:      # mid-row of the middle row (1-D: the middle element)
                inner = n // shape[0] if len(shape) > 1 else 1
                e = (shape[0] // 2) * inner + inner // 2 if len(shape) > 1 else n // 2
            assert 0 <= e < n, (self.straddle, e, n)
            start = straddle_start(a.B, e, item, nbytes)
            assert start < a.B < start + nbytes or nbytes <= 16, (self.straddle, hex(start), nbytes)
            assert self.floor == a.B, "one straddling buffer per launch"
            self.floor = start - GUARD
            assert self.next <= self.floor, "bit-31 buffers reach into the straddling buffer"
        else:
            start = (self.next + GUARD + 255) // 256 * 256
            self.next = start + nbytes + GUARD
            assert self.next <= self.floor, "bit-31 region full"
            assert start >> 31 & 1 and (start + nbytes - 1) >> 31 & 1 and (start >> 32) == ((start + nbytes - 1) >> 32)
        assert start % 16 == 0
        for g in (start - GUARD, start + nbytes):
            a.window(g, GUARD).fill_(PATTERN)
            self.guards.append(g)
        for r in roles:
            self.placed[r] = (start, nbytes)
        return a.window(start, nbytes).view(dtype).view(shape)

    def to(self, t, roles=None):
        assert t.is_contiguous(), "the launch helpers place contiguous buffers and slice them afterwards"
        v = self._carve(t.shape, t.dtype, roles)
        v.copy_(t)
        return v

    def full(self, shape, fill, dtype, roles=None):
        v = self._carve(shape, dtype, roles)
        v.fill_(fill)
        return v

    def check_guards(self):
        for g in self.guards:
            w = self.arena.window(g, GUARD)
            assert bool((w == PATTERN).all()), f"guard band at {hex(g)} written"
