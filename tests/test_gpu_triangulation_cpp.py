"""The C++ layer of SearchForTriangulation: XFmatcher::searchForTriangulation (include/xfeat/ORBmatcher_xfeat.h), the host-vector form and
the form on device-resident keyframes (records finished by XFgrid::buildFromRecord with a depth image), compiled with g++ like the other
drop-in classes: both produce the dump of the C ABI (xfh_triangulation_search) for the rig's scene written to a file, and that dump is the
restatement's answer (tests/ref_triangulation.py): vMatchedPairs in ascending idx1, the return value and the last...() arrays."""
import os
import subprocess

import numpy as np
import pytest

import ref_frame as RF
import ref_triangulation as RT
import triangulation_rig as TR
from conftest import ROOT
from xfeatslam_amd import capi

pytestmark = pytest.mark.gpu

F = np.float32


def gxx(src, exe, *libs):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, src),
                           "-L" + os.path.join(ROOT, "xfeatslam_amd"), "-lxfeat_hip", *libs, "-Wl,-rpath," + os.path.join(ROOT, "xfeatslam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])


rgbd = TR.rgbd


@pytest.fixture(scope="module")
def scene(gpu_lib):
    return TR.Scene()


@pytest.mark.parametrize("b,flags", [(0, 0), (1, RT.ONLY_STEREO), (2, RT.COARSE)])
def test_cpp_search_for_triangulation(scene, oracle_mod, tmp_path, b, flags):
    exe = str(tmp_path / "triangulation_test")
    gxx("tests/cpp/triangulation_test.cpp", exe)
    cam = RF.camera(k1=0.0)
    (k1, img1), (k2, img2) = rgbd(cam, scene.k1), rgbd(cam, scene.k2[b])
    assert (k1["ur"] >= 0).sum() >= 60 and (k2["ur"] >= 0).sum() >= 100
    n1, n2 = TR.N1, TR.N2
    assert (len(k1["xy"]), len(k2["xy"])) == (n1, n2)
    TR.write_in(tmp_path / "in.bin", cam, k1, img1, k2, img2, scene.F12[b], scene.ep[b], flags)
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = np.fromfile(tmp_path / "out.bin", np.int32)
    m = RT.order_free(scene.dist(oracle_mod, b), k1, k2, scene.F12[b], scene.ep[b], flags)
    lit = RT.literal(scene.dist(oracle_mod, b), k1, k2, scene.F12[b], scene.ep[b], flags)
    pairs = np.array(lit["pairs"], np.int32).reshape(-1, 2)
    assert [tuple(p) for p in pairs.tolist()] == sorted(lit["pairs"]) and len(pairs) == m["n_matches"] >= 4
    want = np.concatenate([[m["n_matches"], len(pairs)], pairs.ravel(), m["status"].astype(np.int32), m["match12"], m["best_dist"], m["n_candidates"], m["n_geom"]]).astype(np.int32)
    assert len(raw) == 3 * len(want), (len(raw), len(want))
    abi, host, dev = raw[:len(want)], raw[len(want):2 * len(want)], raw[2 * len(want):]
    assert np.array_equal(abi, want), np.nonzero(abi != want)[0][:8]
    assert np.array_equal(host, want) and np.array_equal(dev, want)
    print(f"neighbour {b} flags {flags}: statuses {np.bincount(m['status'], minlength=5).tolist()}, matches {m['n_matches']}")
