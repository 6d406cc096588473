"""Every `Context.*_layout` (xfeatslam_amd/extractor.py: one table per device call, xfeatslam_amd/layout.py: the offset rule and the guard check)
over B in {1, 3}, every size argument in {1, 63, 64, 257} and guard in {0, 256, 4096}: the structure of the block, the offsets the hand-written
layouts gave before the tables (tests/golden/output_layouts.json, written by tests/golden/make_output_layouts.py), that the guard check the GPU
rigs rely on (tests/guarded.py) sees a single byte out of place, and that parse returns what the table says.  CPU only."""
import inspect
import itertools
import json
import os

import numpy as np
import pytest

from xfeatslam_amd.extractor import Context
from xfeatslam_amd.layout import Layout

BATCHES, SIZES, GUARDS = (1, 3), (1, 63, 64, 257), (0, 256, 4096)
NEW = ("pose_optimize_layout", "sim3_optimize_layout", "sim3_merge_layout")             # no hand-written parent: exempt from the frozen offsets
LAYOUTS = sorted(k for k in dir(Context) if k.endswith("_layout"))
FILL = 0xA5


def cases(fn):
    """-> (key of the fixture or None, the layout) for every combination of the sweep"""
    args = list(inspect.signature(getattr(Context, fn)).parameters)
    assert args[-1] == "guard", (fn, args)
    sizes = [a for a in args[:-1] if a != "B"]
    for B in (BATCHES if "B" in args else (None,)):
        for ns in itertools.product(SIZES, repeat=len(sizes)):
            for guard in GUARDS:
                lay = getattr(Context, fn)(*([B] if B else []), *ns, guard)
                yield (None if B is None else "%d|%s|%d" % (B, ",".join(map(str, ns)), guard)), lay


def test_every_layout_is_swept():
    assert len(LAYOUTS) == 16 and all(k in LAYOUTS for k in NEW), LAYOUTS


@pytest.mark.parametrize("fn", LAYOUTS)
def test_structure(fn):
    for _, lay in cases(fn):
        assert isinstance(lay, Layout)
        g, ends, prev_end = lay.guard, [], 0
        for name, dt, shape in lay.fields:
            a, nb = lay[name], lay[name + "_bytes"]
            assert nb == dt.itemsize * int(np.prod(shape)) and nb > 0, (fn, name)
            assert a % 256 == 0, (fn, name, a)
            assert a >= prev_end + g, (fn, name, "overlaps its neighbour or stands less than the guard after it")
            prev_end = a + nb
            ends.append(prev_end)
        assert lay["bytes"] == ((prev_end + 255) & ~255) + ((g + 255) & ~255) and lay["bytes"] >= prev_end + g, fn
        assert int(lay.used().sum()) == sum(lay[n + "_bytes"] for n in lay.names), (fn, "the arrays are not disjoint")


@pytest.mark.parametrize("fn", [k for k in LAYOUTS if k not in NEW])
def test_offsets_are_those_of_the_hand_written_layouts(fn):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "output_layouts.json")) as f:
        frozen = json.load(f)[fn]
    n = 0
    for key, lay in cases(fn):
        assert list(lay.names) == frozen["names"], fn
        assert [lay[k] for k in lay.names] + [lay["bytes"]] == frozen["cases"][key], (fn, key)
        n += 1
    assert n == len(frozen["cases"]), (fn, "the sweep and the fixture differ")


def written(lay, skip=()):
    """a buffer of fill with every array (but those of skip) overwritten by bytes that are not the fill"""
    raw = np.full(lay["bytes"], FILL, np.uint8)
    raw[lay.used(skip)] = 0x11
    return raw


def raises(lay, raw, at, skip=()):
    bad = raw.copy()
    bad[at] ^= 0xFF
    with pytest.raises(AssertionError):
        lay.check_guards(bad, FILL, skip)


@pytest.mark.parametrize("fn", LAYOUTS)
def test_the_guard_check_sees_one_byte(fn):
    """With guard > 0 the bytes next to every array, the first and the last byte of the buffer are no array's: one byte planted there must be
    found.  With guard = 0 neighbours may touch (an array of a multiple of 256 bytes), so there the plants go wherever a byte next to an array
    belongs to none."""
    for _, lay in cases(fn):
        raw = written(lay)
        lay.check_guards(raw, FILL)
        used = lay.used()
        spots = [0, lay["bytes"] - 1] + [p for k in lay.names for p in (lay[k] - 1, lay[k] + lay[k + "_bytes"])]
        if lay.guard:
            assert all(0 <= p < lay["bytes"] and not used[p] for p in spots), fn
        for p in spots:
            if 0 <= p < lay["bytes"] and not used[p]:
                raises(lay, raw, p)
        with pytest.raises(AssertionError):
            lay.check_guards(raw[:-1], FILL)                                            # not the layout's buffer
        # an array the call was told not to write: untouched it passes, written it is found, at its first and at its last byte
        for k in (lay.names[0], lay.names[-1]):
            quiet = written(lay, skip=(k,))
            lay.check_guards(quiet, FILL, skip=(k,))
            with pytest.raises(AssertionError):
                lay.check_guards(raw, FILL, skip=(k,))
            raises(lay, quiet, lay[k], skip=(k,))
            raises(lay, quiet, lay[k] + lay[k + "_bytes"] - 1, skip=(k,))


def test_the_guard_check_refuses_a_table_without_its_guard():
    """the gap assertion: arrays laid out with less room than the guard they claim"""
    lay = Layout([("a", np.int32, (3, 5)), ("b", np.uint8, 7)], 256)
    lay.check_guards(written(lay), FILL)
    lay.guard = 4096
    with pytest.raises(AssertionError):
        lay.check_guards(written(lay), FILL)


def test_the_message_names_the_offset_and_the_array():
    lay = Context.fuse_search_layout(3, 63, 256)
    raw = written(lay)
    at = lay["proj"] + lay["proj_bytes"] + 5
    raw[at] = 0
    with pytest.raises(AssertionError, match=r"byte %d .*proj" % at):
        lay.check_guards(raw, FILL)


@pytest.mark.parametrize("fn", LAYOUTS)
def test_parse(fn):
    for _, lay in cases(fn):
        raw = np.full(lay["bytes"], FILL, np.uint8)
        want = {}
        for i, (name, dt, shape) in enumerate(lay.fields):
            want[name] = (np.arange(int(np.prod(shape))) * 3 + 7 * i + 1).astype(dt).reshape(shape)     # a ramp of its own per array
            raw[lay[name]:lay[name] + lay[name + "_bytes"]] = want[name].reshape(-1).view(np.uint8)
        got = lay.parse(raw)
        assert list(got) == list(lay.names)
        for name, dt, shape in lay.fields:
            assert got[name].dtype == dt and got[name].shape == shape and np.array_equal(got[name], want[name]), (fn, name)
            assert not np.shares_memory(got[name], raw), (fn, name, "a view, not a copy")
        z = lay.zeros()
        assert all(z[name].dtype == dt and z[name].shape == shape and not z[name].any() for name, dt, shape in lay.fields)
