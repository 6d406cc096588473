"""The output block of xfh_local_ba_device (xfeatslam_amd/local_ba.py: local_ba_layout, a module-level function) under the structure, planted-byte and parse
checks that tests/test_output_layout.py applies to the Context layouts, over nK, nP, nE in {1, 63, 64, 257} and guard in {0, 256, 4096}.  CPU only."""
import itertools

import numpy as np
import pytest

from xfeatslam_amd import local_ba
from xfeatslam_amd.layout import Layout

SIZES, GUARDS, FILL = (1, 63, 64, 257), (0, 256, 4096), 0xA5


def cases():
    for nK, nP, nE in itertools.product(SIZES, repeat=3):
        for guard in GUARDS:
            yield local_ba.local_ba_layout(nK, nP, nE, guard)


def test_table():
    lay = local_ba.local_ba_layout(3, 5, 7)
    assert lay.names == local_ba.NAMES == ("Tcw_out", "points_out", "erase", "chi2", "header", "final_chi2")
    assert [lay[k + "_bytes"] for k in lay.names] == [3 * 48, 5 * 12, 7, 7 * 4, len(local_ba.HEADER) * 4, 8] and len(local_ba.HEADER) == 10


def test_structure():
    for lay in cases():
        assert isinstance(lay, Layout)
        g, prev_end = lay.guard, 0
        for name, dt, shape in lay.fields:
            a, nb = lay[name], lay[name + "_bytes"]
            assert nb == dt.itemsize * int(np.prod(shape)) and nb > 0 and a % 256 == 0 and a >= prev_end + g, name
            prev_end = a + nb
        assert lay["bytes"] == ((prev_end + 255) & ~255) + ((g + 255) & ~255) and lay["bytes"] >= prev_end + g
        assert int(lay.used().sum()) == sum(lay[n + "_bytes"] for n in lay.names)


def written(lay, skip=()):
    raw = np.full(lay["bytes"], FILL, np.uint8)
    raw[lay.used(skip)] = 0x11
    return raw


def test_the_guard_check_sees_one_byte():
    for lay in cases():
        raw = written(lay)
        lay.check_guards(raw, FILL)
        used = lay.used()
        spots = [0, lay["bytes"] - 1] + [p for k in lay.names for p in (lay[k] - 1, lay[k] + lay[k + "_bytes"])]
        if lay.guard:
            assert all(0 <= p < lay["bytes"] and not used[p] for p in spots)
        for p in spots:
            if 0 <= p < lay["bytes"] and not used[p]:
                bad = raw.copy()
                bad[p] ^= 0xFF
                with pytest.raises(AssertionError):
                    lay.check_guards(bad, FILL)
        with pytest.raises(AssertionError):
            lay.check_guards(raw[:-1], FILL)


def test_parse():
    for lay in cases():
        raw = np.full(lay["bytes"], FILL, np.uint8)
        want = {}
        for i, (name, dt, shape) in enumerate(lay.fields):
            want[name] = (np.arange(int(np.prod(shape))) * 3 + 7 * i + 1).astype(dt).reshape(shape)
            raw[lay[name]:lay[name] + lay[name + "_bytes"]] = want[name].reshape(-1).view(np.uint8)
        got = lay.parse(raw)
        for name, dt, shape in lay.fields:
            assert got[name].dtype == dt and got[name].shape == shape and np.array_equal(got[name], want[name]) and not np.shares_memory(got[name], raw), name
