#!/usr/bin/env python
"""Freezes the byte offsets of every device call's output block: runs each `Context.*_layout` over the sweep of
tests/test_output_layout.py and writes tests/golden/output_layouts.json.  The committed file was written by this script at the last
commit whose layouts were hand-written loops (each returned a plain dict), so it records what the device wrappers and every raw-byte
comparison in the GPU tests relied on before the layouts became tables.  Layouts added later have no such parent and are not recorded.
Run:  python tests/golden/make_output_layouts.py      (needs the built library: two layouts ask it for a size)"""
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from xfeatslam_amd.extractor import Context          # noqa: E402

BATCHES, SIZES, GUARDS = (1, 3), (1, 63, 64, 257), (0, 256, 4096)
# layout -> number of size arguments after B
FROZEN = dict(search_projection_layout=2, fuse_search_layout=1, triangulation_search_layout=1, bow_search_layout=2, bow_transform_layout=1,
              bowdb_query_layout=1, map_projection_search_layout=2, sim3_search_layout=2, init_search_layout=2, triangulate_layout=1,
              two_view_layout=1, sim3_solve_layout=1, mlpnp_layout=1)


def sweep(n_sizes):
    return itertools.product(BATCHES, itertools.product(SIZES, repeat=n_sizes), GUARDS)


def key(B, sizes, guard):
    return "%d|%s|%d" % (B, ",".join(map(str, sizes)), guard)


def names_of(lay):
    """the arrays of a layout in offset order (a plain dict of the hand-written form also holds "bytes", "K" and name + "_bytes")"""
    ks = getattr(lay, "names", None) or [k for k in lay if k not in ("bytes", "K") and not k.endswith("_bytes")]
    return sorted(ks, key=lambda k: lay[k])


if __name__ == "__main__":
    out = {}
    for fn, n_sizes in FROZEN.items():
        cases = {}
        for B, sizes, guard in sweep(n_sizes):
            lay = getattr(Context, fn)(B, *sizes, guard)
            names = names_of(lay)
            cases[key(B, sizes, guard)] = [lay[k] for k in names] + [lay["bytes"]]
        out[fn] = dict(names=names, cases=cases)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "output_layouts.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
