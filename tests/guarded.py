"""The guarded run of a device call, once for every rig and chain test: the output block (a xfeatslam_amd.layout.Layout) lies in a buffer filled
with FILL, every other buffer the call may write (workspace, in-place inputs, outputs outside the block) lies between two guards of FILL,
and after the call every byte that belongs to no array must still hold FILL.  No test lives here."""
import numpy as np

from xfeatslam_amd import capi

FILL = 0xA5


def outputs(lay, fill=FILL, keep=None):
    """a device buffer for the output block of lay, every byte = fill (keep: the caller's list of buffers to free, which it joins)"""
    out = capi.DeviceBuffer(lay["bytes"]).upload(np.full(lay["bytes"], fill, np.uint8))
    if keep is not None:
        keep.append(out)
    return out


def download(out, lay, fill=FILL, skip=()):
    """the bytes of the output block after the call, its guards checked (skip: arrays the call was told not to write)"""
    raw = out.download(np.uint8, lay["bytes"])
    lay.check_guards(raw, fill, skip)
    return raw


def problems(arrays, B, names=None):
    """dict of arrays with a leading B (Layout.parse) -> one dict per problem; a count per problem becomes an int"""
    pick = lambda a, p: a[p] if a.ndim > 1 else a[p].item()
    return [{k: pick(arrays[k], p) for k in (names or arrays)} for p in range(B)]


class Guarded:
    """a device buffer of exactly nbytes between two guards of `guard` bytes of fill; .ptr is the address of the inner bytes.  inner: the bytes
    it holds before the call (an array of nbytes bytes), or the byte to fill them with (None: fill)"""

    def __init__(self, nbytes, guard, fill=FILL, inner=None, what="the workspace"):
        self.nbytes, self.guard, self.fill, self.what = int(nbytes), guard, fill, what
        host = np.full(self.nbytes + 2 * guard, fill, np.uint8)
        if inner is not None:
            host[guard:guard + self.nbytes] = inner if np.isscalar(inner) else np.ascontiguousarray(inner).reshape(-1).view(np.uint8)
        self.buf = capi.DeviceBuffer(host.nbytes).upload(host)
        self.ptr = self.buf.ptr + guard

    def download(self):
        """the inner bytes as the call left them; asserts that both guards still hold the fill"""
        raw = self.buf.download(np.uint8, self.nbytes + 2 * self.guard)
        g = self.guard
        bad = np.flatnonzero(np.concatenate([raw[:g], raw[g + self.nbytes:]]) != self.fill)
        assert bad.size == 0, "a guard byte around %s (%d bytes) was written: byte %d" % (self.what, self.nbytes, int(bad[0]) - g if bad[0] < g else int(bad[0]) - g + self.nbytes)
        return raw[g:g + self.nbytes].copy()

    def free(self):
        self.buf.free()
