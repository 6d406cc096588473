"""The C++ layer of the local bundle adjustment: ORB_SLAM3::XFoptimizer::LocalBundleAdjustment (include/xfeat/Optimizer_xfeat.h), compiled with g++ like the
other drop-in classes, on scenes of tests/local_ba_rig.py: the status, the poses, the points, the erase flags, the chi2 and the header against the rule of
tests/ref_local_ba.py under the comparison rules of tests/test_gpu_local_ba.py, the tables written back, twice on one object."""
import os
import struct
import subprocess

import numpy as np
import pytest

import local_ba_rig as G
from conftest import ROOT

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64


@pytest.fixture(scope="module")
def exe(gpu_lib, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("local_ba") / "local_ba_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "local_ba_test.cpp"),
                           "-L" + os.path.join(ROOT, "xfeatslam_amd"), "-lxfeat_hip", "-Wl,-rpath," + os.path.join(ROOT, "xfeatslam_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", path])
    return path


@pytest.mark.parametrize("name", ("one_free", "eleven_mixed", "special", "outliers", "aborted"))
def test_cpp_local_bundle_adjustment(tmp_path, exe, name):
    p = G.scene(name)
    nK, nP, nE = G.dims(p)
    arrays = [np.ascontiguousarray(np.asarray(p[k], dt)) for k, dt in G.INPUTS]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<6i", nK, nP, nE, len(arrays[0]), len(arrays[1]), p.get("max_iterations", 10)) + np.array(list(G.CAM) + [p["inv_sigma2"]], F).tobytes())
        for a in arrays:
            f.write(a.tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = open(tmp_path / "out.bin", "rb").read()
    one = 4 + 48 * nK + 12 * nP + nE + 4 * nE + 40 + 8 + arrays[0].nbytes + arrays[1].nbytes
    assert len(raw) == 2 * one and raw[:one] == raw[one:]               # the second call on the same object: the same bytes
    status, o = struct.unpack("<i", raw[:4])[0], 4
    got = {}
    for key, dt, shape in (("Tcw_out", F, (nK, 12)), ("points_out", F, (nP, 3)), ("erase", np.uint8, (nE,)), ("chi2", F, (nE,)), ("header", np.int32, (10,)),
                           ("final_chi2", D, (1,)), ("pose_table", F, arrays[0].shape), ("point_table", F, arrays[1].shape)):
        size = int(np.prod(shape)) * np.dtype(dt).itemsize
        got[key] = np.frombuffer(raw[o:o + size], dt).reshape(shape).copy()
        o += size
    got["final_chi2"] = float(got["final_chi2"][0])
    m = G.rule_of(name)
    assert status == int(m["header"][0]) == int(got["header"][0])
    bad = G.outputs_agree(got, m)
    assert bad == [], bad
    free = np.asarray(p["kf_fixed"]) == 0
    if status == 0:
        assert np.array_equal(got["pose_table"][p["kf_row"][free]], got["Tcw_out"][free]) and np.array_equal(got["pose_table"][p["kf_row"][~free]], arrays[0][p["kf_row"][~free]])
    else:
        assert np.array_equal(got["pose_table"], arrays[0]) and np.array_equal(got["point_table"], arrays[1])
    print(f"{name}: LocalBundleAdjustment status {status}, {got['header'][9]} of {nE} edges to erase")
