"""The C++ layer of the Sim3 optimisation: ORB_SLAM3::XFoptimizer::OptimizeSim3 (include/xfeat/Optimizer_xfeat.h), compiled with g++ like the other
drop-in classes, on scenes of tests/optsim3_rig.py: the return value, the similarity, the matches, the status, the chi2, the header and the composed
pose against the rule of tests/ref_optsim3.py under the comparison rules of tests/test_gpu_optsim3.py, twice on one object."""
import os
import struct
import subprocess

import numpy as np
import pytest

import optsim3_rig as G
import ref_optsim3 as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64


@pytest.fixture(scope="module")
def exe(gpu_lib, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("optsim3") / "optsim3_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "optsim3_test.cpp"),
                           "-L" + os.path.join(ROOT, "xfeatslam_amd"), "-lxfeat_hip", "-Wl,-rpath," + os.path.join(ROOT, "xfeatslam_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", path])
    return path


@pytest.mark.parametrize("name", ("one", "keep9", "out100", "all_points", "e1025"))
def test_cpp_optimize_sim3(tmp_path, exe, name):
    p = G.scene(name)
    n1, M1, nq, n2 = len(p["assigned"]), len(p["points1"]), len(p["points2"]), len(p["xy_un2"])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<7i", n1, M1, nq, n2, p["fix_scale"], p["all_points"], 1) + np.array(G.CAM, F).tobytes() + struct.pack("<f", p["th2"]))
        for k, dt in G.SIDE1 + G.SIDE2:
            f.write(np.ascontiguousarray(np.asarray(p[k], dt)).tobytes())
        f.write(np.asarray(p["S12"], F).tobytes() + np.asarray(p["Tmw"], F).tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = open(tmp_path / "out.bin", "rb").read()
    one = 4 + 52 + 4 * n1 + n1 + 8 * n1 + 64 + 64 + 8 + 48 + 12
    assert len(raw) == 2 * one and raw[:one] == raw[one:]               # the second call on the same object: the same bytes
    ret, o = struct.unpack("<i", raw[:4])[0], 4
    got = {}
    for key, dt, n in (("S12_out", F, 13), ("assigned_out", np.int32, n1), ("status", np.uint8, n1), ("chi2", F, 2 * n1), ("header", np.int32, 16), ("state", D, 8),
                       ("final_chi2", D, 1), ("Tcw", F, 12), ("Ow", F, 3)):
        size = n * np.dtype(dt).itemsize
        got[key] = np.frombuffer(raw[o:o + size], dt).copy()
        o += size
    got["chi2"], got["final_chi2"] = got["chi2"].reshape(n1, 2), float(got["final_chi2"][0])
    m = R.rule(p)
    assert ret == int(m["header"][6]) == int(got["header"][6])
    bad = R.outputs_agree(got, m, G.SIM3OPT_TOL)
    assert bad == [], bad
    print(f"{name}: OptimizeSim3 returned {ret} of {got['header'][0]} correspondences")
