"""The C++ layer of the pose optimisation: ORB_SLAM3::XFoptimizer (include/xfeat/Optimizer_xfeat.h), compiled with g++ like the other drop-in
classes, on scenes of tests/poseopt_rig.py: the return value, the pose, the flags, the chi2 and the header against the rule of
tests/ref_poseopt.py (integers equal, floats within one float32 step), twice on one object, and the pose it leaves on the device."""
import os
import struct
import subprocess

import numpy as np
import pytest

import poseopt_rig as R
import ref_poseopt as RP
from conftest import ROOT

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def exe(gpu_lib, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("poseopt") / "poseopt_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "poseopt_test.cpp"),
                           "-L" + os.path.join(ROOT, "xfeatslam_amd"), "-lxfeat_hip", "-Wl,-rpath," + os.path.join(ROOT, "xfeatslam_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", path])
    return path


@pytest.mark.parametrize("name", ("n2", "n9_mono", "n64_stereo", "n65_mixed", "n1000"))
def test_cpp_pose_optimization(tmp_path, exe, name):
    s = R.scene(name)
    nt = s["nt"]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<3i", nt, s["nq"], int(s["uright"] is not None)) + s["Tcw"].astype(F).tobytes() + np.array(R.CAM, F).tobytes() + struct.pack("<f", R.INV_SIGMA2))
        f.write(s["xy_un"].tobytes() + (s["uright"].tobytes() if s["uright"] is not None else b"") + s["assigned"].tobytes() + s["points"].tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = open(tmp_path / "out.bin", "rb").read()
    one = 4 + 48 + nt + 4 * nt + 32 + 8
    assert len(raw) == 2 * one + 48 and raw[:one] == raw[one:2 * one]                          # the second call on the same object: the same bytes
    m = R.model(s)
    ret = struct.unpack("<i", raw[:4])[0]
    T = np.frombuffer(raw[4:52], F); ol = np.frombuffer(raw[52:52 + nt], np.uint8); c2 = np.frombuffer(raw[52 + nt:52 + 5 * nt], F)
    hdr = np.frombuffer(raw[52 + 5 * nt:84 + 5 * nt], np.int32)
    assert ret == int(m["header"][2]) and np.array_equal(hdr, m["header"]) and np.array_equal(ol, m["outlier"])
    assert RP.ulps(T, m["Tcw_out"]).max() <= 1 and RP.ulps(c2, m["chi2"]).max() <= 1
    assert raw[2 * one:] == raw[4:52]                                                          # the pose on the device is the pose returned
    print(f"{name}: PoseOptimization returned {ret} of {hdr[0]}")
