"""The C++ layer of the essential-graph optimisation: ORB_SLAM3::XFoptimizer::OptimizeEssentialGraph (include/xfeat/Optimizer_xfeat.h), compiled with g++ like
the other drop-in classes, on two scenes of tests/essential_graph_rig.py: the status, the estimates, the poses, the points, the chi2 and the header against
the rule of tests/ref_essential_graph.py under the comparison rules of tests/test_gpu_essential_graph.py, the tables written back, twice on one object."""
import os
import struct
import subprocess

import numpy as np
import pytest

import essential_graph_rig as G
from conftest import ROOT
from xfeatslam_amd import essential_graph as EG

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64


@pytest.fixture(scope="module")
def exe(gpu_lib, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("essential_graph") / "essential_graph_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "essential_graph_test.cpp"),
                           "-L" + os.path.join(ROOT, "xfeatslam_amd"), "-lxfeat_hip", "-Wl,-rpath," + os.path.join(ROOT, "xfeatslam_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", path])
    return path


@pytest.mark.parametrize("name", ("ten_free", "scale_fixed"))
def test_cpp_optimize_essential_graph(tmp_path, exe, name):
    p = G.scene(name)
    nV, nE, nP, nS = G.dims(p)
    arrays = EG.host_arrays(p)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<8i", nV, nE, nP, nS, len(arrays[0]), len(arrays[1]), p["fix_scale"], p["max_iterations"]))
        for a in arrays:
            f.write(a.tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = open(tmp_path / "out.bin", "rb").read()
    one = 4 + 64 * nV + 48 * nV + 12 * nP + 4 * nE + 36 + 8 + arrays[0].nbytes + arrays[1].nbytes
    assert len(raw) == 2 * one and raw[:one] == raw[one:]               # the second call on the same object: the same bytes
    status, o = struct.unpack("<i", raw[:4])[0], 4
    got = {}
    for key, dt, shape in (("Sim3_out", D, (nV, 8)), ("Tcw_out", F, (nV, 12)), ("points_out", F, (nP, 3)), ("chi2", F, (nE,)), ("header", np.int32, (9,)),
                           ("final_chi2", D, (1,)), ("pose_table", F, arrays[0].shape), ("point_table", F, arrays[1].shape)):
        size = int(np.prod(shape)) * np.dtype(dt).itemsize
        got[key] = np.frombuffer(raw[o:o + size], dt).reshape(shape).copy()
        o += size
    got["final_chi2"] = float(got["final_chi2"][0])
    m = G.rule_of(name)
    assert status == int(m["header"][0]) == int(got["header"][0])
    bad = G.outputs_agree(got, m)
    assert bad == [], bad
    assert np.array_equal(got["pose_table"][p["kf_row"]], got["Tcw_out"]) and np.array_equal(got["point_table"][p["point_row"]], got["points_out"])
    print(f"{name}: OptimizeEssentialGraph status {status}, header {got['header'].tolist()}")
