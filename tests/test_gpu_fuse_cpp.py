"""The C++ layer of Fuse: XFmatcher::fuse (include/xfeat/ORBmatcher_xfeat.h), host-vector and device-pointer overloads, compiled with g++
like the other drop-in classes: both produce the dump of the C ABI (xfh_fuse_search) for the rig's scene written to a file, and that
dump is the sequential restatement's answer (tests/ref_fuse.py)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_frame as RF
import ref_fuse as RU
import ref_window as RW
from conftest import ROOT
from fuse_rig import NL, SF, FuseRig
from xfeatslam_amd import capi

pytestmark = pytest.mark.gpu

F = np.float32


def gxx(src, exe, *libs):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, src),
                           "-L" + os.path.join(ROOT, "xfeatslam_amd"), "-lxfeat_hip", *libs, "-Wl,-rpath," + os.path.join(ROOT, "xfeatslam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])


@pytest.fixture(scope="module")
def scene(gpu_lib, weights_dense):
    """the 1000-feature rig's problem 1 on the host: frame 1's undistorted keypoints, descriptors and uright, the map points of frame 0.
    The C++ side builds the grid from the UNDISTORTED keypoints with the image as bounds (k1 = 0 in the camera it is given)."""
    fr = FuseRig(gpu_lib, weights_dense[1], 1000, 901)
    rg = fr.rig
    s = dict(xy=rg.xy[1].copy(), tg=rg.recs[1][1].copy(), ur=rg.ur[1].copy(), q=fr.qdesc.copy(), xyz=fr.xyz.copy(), nr=fr.normals.copy(), dd=fr.dist.copy(),
             flags=fr.flags.copy(), T=fr.poses[1].copy(), Ow=fr.Ow[1].copy())
    fr.close()
    return s


@pytest.mark.parametrize("sim3,th", [(0, 3.0), (1, 7.0)])
def test_cpp_fuse(scene, oracle_mod, tmp_path, sim3, th):
    exe = str(tmp_path / "fuse_test")
    gxx("tests/cpp/fuse_test.cpp", exe)
    s = scene
    cam = RF.camera(k1=0.0)
    b = tuple(float(x) for x in RF.bounds(cam))
    nt = nq = len(s["xy"])
    k = np.zeros(nt, capi.KP_DTYPE); k["x"] = s["xy"][:, 0]; k["y"] = s["xy"][:, 1]; k["size"] = 1; k["angle"] = -1
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<4i2f", nq, nt, NL, sim3, th, SF))
        f.write(struct.pack("<10f6i", *[float(cam[c]) for c in "fx fy cx cy k1 k2 p1 p2 k3 bf".split()], int(cam["width"]), int(cam["height"]), 0, 0, 0, 0))
        for a in (s["T"], s["Ow"], k, s["tg"], s["ur"], s["q"], s["xyz"], s["nr"], s["dd"], s["flags"]):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = np.fromfile(tmp_path / "out.bin", np.int32)
    per = 6 * nq + 1
    assert len(raw) == 3 * per
    abi, host, dev = raw[:per], raw[per:2 * per], raw[2 * per:]
    assert np.array_equal(abi, host) and np.array_equal(abi, dev)
    u, v, ur, rr, lv, st = RU.project(s["T"], s["Ow"], cam, b, th, SF, NL, s["xyz"], s["nr"], s["dd"])
    act = (s["flags"] & 1) != 0
    st = np.where(act, st, RU.INACTIVE).astype(np.uint8)
    x, y = s["xy"][:, 0].copy(), s["xy"][:, 1].copy()
    m = RU.search(oracle_mod, st, lv, u, v, rr, ur, s["q"], RW.build(x, y, b), x, y, b, s["tg"], uright=s["ur"], chi2=not sim3, init_dist=RU.INT_MAX if sim3 else 256)
    want = np.concatenate([[m["n_fused"]], m["best_idx"], m["status"].astype(np.int32), m["best_dist"], m["n_window"], m["n_tested"], np.where(act, lv, -1)])
    assert np.array_equal(abi, want.astype(np.int32)), np.nonzero(abi != want)[0][:8]
    print(f"sim3 {sim3} th {th}: statuses {np.bincount(m['status'], minlength=8).tolist()}, fused {m['n_fused']}")
    assert len(set(m["status"].tolist())) >= 7
