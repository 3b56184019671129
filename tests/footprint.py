"""Footprint checks for the device-pointer entry points (include/fsgm.h): does a call write only its outputs, and does its
result depend only on its inputs?

An Arena is one uint8 device tensor from a single allocation.  Every input and output of one call is carved from it as a
contiguous view, with a guard band before the first, between any two and after the last.  A guard is at least as large as the
largest tensor of the case and never below 64 KiB: a kernel wrong by a vector, a row or a whole frame still lands inside the
arena, and the bug is seen by reading bytes back, never by a fault.  Nothing here places a buffer at the end of an allocation.

Two placements:
  aligned   every start a multiple of 256
  minimal   every start aligned to exactly what the entry's check table demands (the `align` of its DevicePtr row, which is the
            element size in every table of fsgm_amd/csrc/capi_*.hip: 1 for u8, 4 for u32 / i32, 8 for f64) and not to twice
            that -- u8 tensors start at an odd address -- and the end not 16-byte aligned wherever size and dtype allow

Guards hold a pattern byte, outputs the poison byte 0xCD (0xCDCDCDCD is above any cost sum, as a double about -6.2e66: no entry
produces either), inputs their data.

The plumbing of a call is not restated here: record() runs the ordinary call -- the package's own wrappers and binders -- with
the C entry replaced by a recorder, and replay() makes the same ctypes call with every device pointer swapped for the arena's
carved tensor, pointers inside fsgm_epi_in / fsgm_epi_out included.  Only arguments passed as ctypes.c_void_p (or as such a field
of a struct passed by reference) are recognised as pointers: a wrapper that handed a bare int would not be replayed, and the
caller's check that every tensor it names was among the call's pointers then fails.

Stray-write detection relies on both guard patterns: a stray store of zeros cannot be seen against 0x00 guards nor one of 0xFF
bytes against 0xFF guards, so check() is made in both arenas; a store that writes an input's own value back is invisible.
"""
import ctypes as C

import torch

POISON = 0xCD
MIN_GUARD = 64 * 1024
PLACEMENTS = ("aligned", "minimal")


def _up(x, a):
    return -(-x // a) * a


def place(cursor, nbytes, esize, placement):
    """the first start >= cursor (an offset from a 256-aligned base) that the placement allows"""
    if placement == "aligned":
        return _up(cursor, 256)
    assert placement == "minimal"
    first = None
    for s in range(_up(cursor, esize), cursor + 64 + 2 * esize, esize):
        if s % (2 * esize) != esize % (2 * esize) or (esize == 1 and s % 2 == 0):
            continue
        if first is None:
            first = s
        if (s + nbytes) % 16 != 0:
            return s
    return first                                  # f64 with an odd element count: start = 8 mod 16 ends on a multiple of 16


class Carved:
    def __init__(self, name, role, like, start):
        self.name, self.role, self.like, self.start = name, role, like, start
        self.nbytes = like.numel() * like.element_size()
        self.end = start + self.nbytes
        self.view = None

    def __repr__(self):
        return f"{self.role} {self.name} {tuple(self.like.shape)} {self.like.dtype} bytes [{self.start}, {self.end})"


class Arena:
    """specs: (name, role, tensor) in carving order; role 'in' (the tensor's bytes are copied in), 'out' (poison) or 'inout'
    (an output that aliases an input, as the header allows for some entries: the input's bytes, treated as an output)"""

    def __init__(self, specs, placement, pattern, device):
        assert specs and all(t.numel() > 0 and t.is_contiguous() for _, _, t in specs)
        self.placement, self.pattern = placement, pattern
        largest = max(t.numel() * t.element_size() for _, _, t in specs)
        self.guard = _up(max(MIN_GUARD, largest), 256)
        self.carved, cursor = [], self.guard
        for name, role, t in specs:
            c = Carved(name, role, t, place(cursor, t.numel() * t.element_size(), t.element_size(), placement))
            assert c.start - cursor >= 0
            self.carved.append(c)
            cursor = c.end + self.guard
        self.size = _up(cursor, 256)
        self.buf = torch.full((self.size,), pattern, dtype=torch.uint8, device=device)
        assert self.buf.data_ptr() % 256 == 0
        for c in self.carved:
            raw = self.buf[c.start:c.end]
            if c.role == "out":
                raw.fill_(POISON)
            else:
                raw.copy_(c.like.reshape(-1).view(torch.uint8))
            c.view = raw.view(c.like.dtype).view(c.like.shape)
            assert c.view.data_ptr() == self.buf.data_ptr() + c.start and c.view.is_contiguous()
        self._assert_layout()
        self.before = self.buf.clone()

    def _assert_layout(self):
        """the guard rule and the placement rule, as conditions"""
        prev_end = 0
        for c in self.carved:
            assert c.start - prev_end >= self.guard >= max(MIN_GUARD, c.nbytes), (c, prev_end, self.guard)
            p, e = c.view.data_ptr(), c.like.element_size()
            if self.placement == "aligned":
                assert p % 256 == 0
            else:
                assert p % e == 0 and p % (2 * e) != 0, c
                if e < 8 or c.nbytes % 16 == 0:
                    assert (p + c.nbytes) % 16 != 0, c
            prev_end = c.end
        assert self.size - prev_end >= self.guard

    def __getitem__(self, name):
        return next(c for c in self.carved if c.name == name).view

    def outputs(self):
        return {c.name: c.view for c in self.carved if c.role != "in"}

    def nearest(self, off):
        return min(self.carved, key=lambda c: 0 if c.start <= off < c.end else min(abs(off - c.start), abs(off - (c.end - 1))))

    def check(self, pattern):
        """One device-side comparison: every byte outside the carved outputs -- the guards and every input -- still holds what
        it held before the call.  Raises with the first offending offset and the carved tensor nearest to it."""
        assert pattern == self.pattern
        changed = self.buf != self.before
        for c in self.carved:
            if c.role != "in":
                changed[c.start:c.end] = False
        if bool(changed.any()):
            off = int(changed.nonzero()[0])
            c = self.nearest(off)
            where = (f"{off - c.start} bytes into" if c.start <= off < c.end
                     else f"{c.start - off} bytes before" if off < c.start else f"{off - c.end} bytes past the end of")
            n = int(changed.sum())
            raise AssertionError(f"stray write ({self.placement} placement, guard pattern {pattern:#04x}): arena offset {off} changed from "
                                 f"{int(self.before[off]):#04x} to {int(self.buf[off]):#04x}, {where} {c!r}; {n} bytes changed in all")

    def all_written(self, name):
        """no element of output `name` still holds the poison"""
        c = next(c for c in self.carved if c.name == name)
        assert c.role == "out", f"{name} is not a poisoned output"
        raw = self.buf[c.start:c.end].view(-1, c.like.element_size())
        left = (raw == POISON).all(dim=1)
        if bool(left.any()):
            idx = int(left.nonzero()[0])
            raise AssertionError(f"not fully written ({self.placement} placement): {int(left.sum())} of {left.numel()} elements of {c!r} "
                                 f"still hold the poison, the first at flat index {idx} = {_unravel(idx, c.like.shape)}")


def _unravel(idx, shape):
    out = []
    for s in reversed(shape):
        out.append(idx % s)
        idx //= s
    return tuple(reversed(out))


def same(a, b):
    """NaN positions are equal and numbers are equal (integers: equal)"""
    if tuple(a.shape) != tuple(b.shape) or a.dtype != b.dtype:
        return False
    if a.dtype.is_floating_point:
        return bool(((a == b) | (a.isnan() & b.isnan())).all())
    return bit_identical(a, b)


def bit_identical(a, b):
    return tuple(a.shape) == tuple(b.shape) and a.dtype == b.dtype and torch.equal(
        a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


# ------------------------------------------------------------------------------------------------ record and replay
class Recorder:
    """stands in for one C entry of the loaded library: passes every call on and keeps its arguments"""

    def __init__(self, fn):
        self.fn, self.calls = fn, []

    def __call__(self, *args):
        self.calls.append(args)
        return self.fn(*args)


def record(lib, entry, ordinary):
    """ordinary() with lib.<entry> recorded: (what ordinary returned, the one call's arguments, the real entry)"""
    real = getattr(lib, entry)
    rec = Recorder(real)
    setattr(lib, entry, rec)
    try:
        res = ordinary()
    finally:
        setattr(lib, entry, real)
    assert len(rec.calls) == 1, f"the ordinary call went through {entry} {len(rec.calls)} times"
    return res, rec.calls[0], real


def _pointer_fields(struct):
    return [name for name, typ in struct._fields_ if typ is C.c_void_p]


def pointers_of(args):
    """every non-NULL void* among the arguments, those in structs passed by reference included, in argument order"""
    out = []
    for a in args:
        if isinstance(a, C.c_void_p):
            if a.value:
                out.append(a.value)
        elif hasattr(a, "_obj") and isinstance(a._obj, C.Structure):
            out += [v for v in (getattr(a._obj, f) for f in _pointer_fields(a._obj)) if v]
    return out


def replay(real, args, swap):
    """real(*args) with every pointer that is a key of `swap` replaced by its value"""
    keep, new = [], []
    for a in args:
        if isinstance(a, C.c_void_p) and a.value in swap:
            a = C.c_void_p(swap[a.value])
        elif hasattr(a, "_obj") and isinstance(a._obj, C.Structure) and _pointer_fields(a._obj):
            s = type(a._obj).from_buffer_copy(a._obj)
            for f in _pointer_fields(s):
                v = getattr(s, f)
                if v in swap:
                    setattr(s, f, swap[v])
            keep.append(s)
            a = C.byref(s)
        new.append(a)
    return real(*new)


# ------------------------------------------------------------------------------------------------ host forms
class HostArena:
    """The same guard rule on the host: the output arrays of a *_host call as views of one larger numpy array, a guard band of
    max(64 KiB, the largest output) before the first, between any two and after the last.  It catches a device-to-host copy sized
    from the plan's padded buffer instead of the caller's array.  shapes: (name, shape, dtype) in carving order."""

    def __init__(self, shapes, pattern):
        import numpy as np
        self.np, self.pattern = np, pattern
        sizes = [int(np.prod(shape)) * np.dtype(dtype).itemsize for _, shape, dtype in shapes]
        self.guard = _up(max([MIN_GUARD] + sizes), 256)
        self.buf = np.full(sum(sizes) + (len(sizes) + 1) * (self.guard + 256) + 256, pattern, np.uint8)
        base = self.buf.ctypes.data
        self.ranges, self.views, cursor = [], {}, self.guard
        for (name, shape, dtype), size in zip(shapes, sizes):
            start = _up(base + cursor, 256) - base
            raw = self.buf[start:start + size]
            raw[:] = POISON
            self.ranges.append((name, start, start + size))
            self.views[name] = raw.view(dtype).reshape(shape)
            assert self.views[name].ctypes.data == base + start and self.views[name].flags.c_contiguous
            cursor = start + size + self.guard
        assert cursor <= self.buf.size

    def check(self):
        """every byte outside the carved outputs still holds the pattern; the first offending offset and the nearest output"""
        np = self.np
        keep = np.ones(self.buf.size, bool)
        for _, a, b in self.ranges:
            keep[a:b] = False
        bad = np.flatnonzero(keep & (self.buf != self.pattern))
        if bad.size:
            off = int(bad[0])
            name, a, b = min(self.ranges, key=lambda r: min(abs(off - r[1]), abs(off - (r[2] - 1))))
            where = f"{a - off} bytes before" if off < a else f"{off - b} bytes past the end of"
            raise AssertionError(f"stray host write (guard pattern {self.pattern:#04x}): offset {off} holds {int(self.buf[off]):#04x}, "
                                 f"{where} {name} [{a}, {b}); {bad.size} bytes changed in all")
