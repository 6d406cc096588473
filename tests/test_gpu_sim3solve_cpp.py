"""The C++ layer of the Sim3 solver: ORB_SLAM3::XFsim3Solver (include/xfeat/Sim3Solver_xfeat.h), compiled with g++ like the other drop-in classes,
in its device form and its host-container form, beside the C ABI's host-pointer form, on scenes of tests/sim3solve_rig.py: the three return the
same bool, header, similarity, flags and composed pose, and these equal the rule of tests/ref_sim3solve.py (integers equal, floats by bits).  The
class builds the iteration table itself from (prob, minInliers, maxIts), so the table of the scenes is checked against it on the way."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_sim3solve as R
import sim3solve_rig as G
from conftest import ROOT

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def exe(gpu_lib, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("sim3solve") / "sim3solve_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "sim3solve_test.cpp"),
                           "-L" + os.path.join(ROOT, "xfeatslam_amd"), "-lxfeat_hip", "-Wl,-rpath," + os.path.join(ROOT, "xfeatslam_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", path])
    return path


@pytest.mark.parametrize("name", ("first", "after64", "no_more", "n_below_min", "fixed_unit", "big"))
def test_cpp_sim3_solver(tmp_path, exe, name):
    sc = G.rig()[name]
    n1, M, iters = len(sc["point1"]), len(sc["points"]), len(sc["draws"][0])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<6i10f", n1, M, iters, G.RAND_MAX, sc["min_inliers"], int(sc["fix_scale"]), *[float(c) for c in sc["cam1"]], *[float(c) for c in sc["cam2"]], 9.0, 9.0))
        for a, dt in ((sc["points"], F), (sc["point1"], np.int32), (sc["matched"][0], np.int32), (sc["T1w"], F), (sc["T2w"][0], F), (sc["table"], np.int32),
                      (sc["draws"][0], np.int32)):
            f.write(np.ascontiguousarray(a, dt).tobytes())
        f.write(struct.pack("<di", G.PROB, G.MAX_ITS))
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    w = G.rule_of(sc)
    ok = int(w["header"][1] == R.CONVERGED)
    z = lambda k, n, dt: np.zeros(n, dt) if w[k] is None else np.asarray(w[k], dt)
    want = struct.pack("<i", ok) + w["header"].astype(np.int32).tobytes() + z("floats", 32, F).tobytes() + z("inliers", n1, np.uint8).tobytes()
    want += z("Tcw", 12, F).tobytes() + z("Ow", 3, F).tobytes()
    raw = open(tmp_path / "out.bin", "rb").read()
    assert len(raw) == 3 * len(want)
    for k, form in enumerate(("device overload", "host containers", "xfh_sim3_solve")):
        assert raw[k * len(want):(k + 1) * len(want)] == want, form
    print(f"{name}: returns {bool(ok)}, status {R.STATUS_NAMES[w['header'][1]]}")
