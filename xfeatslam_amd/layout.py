"""The output block of a device call: several arrays inside one device buffer.  A call states its arrays once, as a table of (name, dtype,
shape); the byte offsets, the pointers handed to the C call, the arrays parsed from the downloaded bytes and the tests' guard check all come
from that table."""
from __future__ import annotations

import numpy as np


def al(x: int) -> int:
    return (x + 255) & ~255


class Layout(dict):
    """Layout(fields, guard=0): fields = (name, dtype, shape) per array, shape the whole array's (an int for one dimension).  The arrays lie in
    the table's order at multiples of 256 bytes; guard > 0 leaves at least that many bytes the call never writes before the first array and
    after every array (for tests that fill them).  lay[name] = byte offset, lay[name + "_bytes"] = size, lay["bytes"] = size of the buffer.
    As a dict it holds the offsets and "bytes" (what the hand-written layouts returned); the sizes are answered on request."""

    def __init__(self, fields, guard: int = 0):
        super().__init__()
        self.guard = guard
        self.fields = tuple((name, np.dtype(dt), (shape,) if isinstance(shape, int) else tuple(shape)) for name, dt, shape in fields)
        self.names = tuple(f[0] for f in self.fields)
        self.sizes, off = {}, al(guard)
        for name, dt, shape in self.fields:
            nbytes = dt.itemsize * int(np.prod(shape, dtype=np.int64))
            self[name], self.sizes[name + "_bytes"] = off, nbytes
            off += al(nbytes) + al(guard)
        self["bytes"] = off

    def __missing__(self, key):
        return self.sizes[key]

    @classmethod
    def of(cls, table, guard: int = 0, **dims):
        """a table whose shapes name their dimensions ("B", "n1", ...) with the dimensions' values"""
        return cls([(name, dt, tuple(dims.get(d, d) for d in shape)) for name, dt, shape in table], guard)

    def parse(self, raw: np.ndarray) -> dict:
        """the downloaded bytes of the buffer -> dict of arrays (copies) with the table's dtypes and shapes"""
        assert raw.dtype == np.uint8 and raw.shape == (self["bytes"],)
        return {name: raw[self[name]:self[name] + self[name + "_bytes"]].view(dt).reshape(shape).copy() for name, dt, shape in self.fields}

    def zeros(self) -> dict:
        """dict of zeroed host arrays with the table's dtypes and shapes: what a host-pointer form of the call writes into"""
        return {name: np.zeros(shape, dt) for name, dt, shape in self.fields}

    def used(self, skip=()) -> np.ndarray:
        """bool per byte of the buffer: the byte belongs to an array (not counting the arrays named in skip)"""
        m = np.zeros(self["bytes"], bool)
        for name in self.names:
            m[self[name]:self[name] + self[name + "_bytes"]] = name not in skip
        return m

    def check_guards(self, raw: np.ndarray, fill: int = 0xA5, skip=()):
        """raw: the bytes of a buffer that held `fill` everywhere before the call.  Asserts that every array has at least `guard` bytes of no
        array before and after it inside the buffer, and that every byte outside the arrays, and inside the arrays named in skip (those the call
        was told not to write), still holds the fill"""
        assert raw.dtype == np.uint8 and raw.shape == (self["bytes"],), "the buffer is not the layout's"
        assert all(k in self.names for k in skip), skip
        used, g = self.used(), self.guard
        for name in self.names:
            a, b = self[name], self[name] + self[name + "_bytes"]
            assert a >= g and not used[a - g:a].any() and b + g <= self["bytes"] and not used[b:b + g].any(), "no %d bytes free around %s" % (g, name)
        bad = np.flatnonzero((raw != fill) & ~self.used(skip))
        if bad.size:
            at = int(bad[0])
            near = min(self.names, key=lambda k: 0 if self[k] <= at < self[k] + self[k + "_bytes"] else min(abs(at - self[k]), abs(at - self[k] - self[k + "_bytes"] + 1)))
            raise AssertionError("byte %d outside the written arrays holds 0x%02X, not the fill 0x%02X (nearest array: %s at %d, %d bytes)"
                                 % (at, int(raw[at]), fill, near, self[near], self[near + "_bytes"]))
