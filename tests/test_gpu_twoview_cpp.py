"""The C++ layer of the two-view reconstruction: ORB_SLAM3::XFtwoView (include/xfeat/TwoViewReconstruction_xfeat.h), compiled with g++ like the
other drop-in classes, in its device form and its host-container form, beside the C ABI's host-pointer form, on scenes of tests/twoview_rig.py:
the three return the same bool, header, pose, flags, points and match list, and these equal the rule of tests/ref_twoview.py (integers equal,
floats by bits)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_twoview as R
import twoview_rig as G
from conftest import ROOT

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def exe(gpu_lib, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("twoview") / "twoview_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "twoview_test.cpp"),
                           "-L" + os.path.join(ROOT, "xfeatslam_amd"), "-lxfeat_hip", "-Wl,-rpath," + os.path.join(ROOT, "xfeatslam_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", path])
    return path


@pytest.mark.parametrize("name", ("general", "plane", "rotation", "n7", "nonfinite"))
def test_cpp_two_view(tmp_path, exe, name):
    sc = G.rig()[name]
    n1, n2, iters = len(sc["xy1"]), len(sc["xy2"]), len(sc["draws"])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<5i5fd", n1, n2, iters, G.RAND_MAX, 50, *[float(c) for c in sc.get("cam", G.CAM)], float(sc["sigma"]), R.DEFAULT_COS))
        for a, dt in ((sc["xy1"], F), (sc["xy2"], F), (sc["m12"], np.int32), (sc["draws"], np.int32)):
            f.write(np.ascontiguousarray(a, dt).tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    w = G.rule_of(sc)
    ok = int(w["header"][1] >= R.OK_H)
    want = struct.pack("<i", ok) + w["header"].astype(np.int32).tobytes() + w["floats"][R.F_T21:R.F_T21 + 12].astype(F).tobytes() + w["tri"].tobytes()
    want += w["p3d"].astype(F).tobytes() + w["matches_out"].astype(np.int32).tobytes()
    raw = open(tmp_path / "out.bin", "rb").read()
    assert len(raw) == 3 * len(want)
    for k, form in enumerate(("device overload", "host containers", "xfh_two_view")):
        assert raw[k * len(want):(k + 1) * len(want)] == want, form
    print(f"{name}: returns {bool(ok)}, status {R.STATUS_NAMES[w['header'][1]]}")
