"""The C++ layer of SearchByProjection: XFmatcher::searchByProjection (include/xfeat/ORBmatcher_xfeat.h), host-vector and
device-pointer overloads, compiled with g++ like the other drop-in classes: both produce the dump of the C ABI
(xfh_search_projection) for one scene, and that dump is the sequential restatement's answer."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_frame as RF
import ref_projection as RP
import ref_window as RW
from conftest import ROOT
from xfeatslam_amd import capi

pytestmark = pytest.mark.gpu

F = np.float32


def gxx(src, exe, *libs):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, src),
                           "-L" + os.path.join(ROOT, "xfeatslam_amd"), "-lxfeat_hip", *libs, "-Wl,-rpath," + os.path.join(ROOT, "xfeatslam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])


@pytest.mark.parametrize("ratio,init", [(0.0, 1 << 30), (0.9, 256)])
def test_cpp_search_by_projection(gpu_lib, oracle_mod, tmp_path, ratio, init):
    exe = str(tmp_path / "projection_test")
    gxx("tests/cpp/projection_test.cpp", exe)
    cam = RF.camera(k1=0.0)                                             # keypoints are given undistorted; the bounds are the image
    b = tuple(float(x) for x in RF.bounds(cam))
    rng = np.random.RandomState(17)
    nt, nq, th_high, radius = 2000, 700, 1000, 15.0
    k = np.zeros(nt, capi.KP_DTYPE)
    k["x"] = rng.uniform(0, 640, nt).astype(F); k["y"] = rng.uniform(0, 480, nt).astype(F); k["size"] = 1; k["angle"] = -1
    tg = rng.randn(nt, 64); tg = (tg / np.linalg.norm(tg, axis=1, keepdims=True)).astype(F)
    # queries in clusters of four around one keypoint with nearly one descriptor: they compete for the same few keypoints
    src = np.repeat(rng.randint(0, nt, nq // 4), 4)
    q = tg[src] + 0.03 * rng.randn(nq, 64); q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)
    T = RP.pose(5, (2, 1), cam=cam)
    xyz, flags = RP.scene(5, np.stack([k["x"][src], k["y"][src]], 1), cam)
    skip = ((rng.rand(nt) < 0.1) * 3).astype(np.uint8)
    uright = np.where(rng.rand(nt) < 0.5, k["x"] - rng.uniform(15, 25, nt), -1).astype(F)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<4i2f", nq, nt, init, th_high, ratio, radius))
        f.write(struct.pack("<10f6i", *[float(cam[c]) for c in "fx fy cx cy k1 k2 p1 p2 k3 bf".split()], int(cam["width"]), int(cam["height"]), 0, 0, 0, 0))
        for a in (T, k, tg, q, xyz, flags, skip, uright):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = np.fromfile(tmp_path / "out.bin", np.int32)
    per = 5 * nq + nt + 1
    assert len(raw) == 3 * per
    abi, host, dev = raw[:per], raw[per:2 * per], raw[2 * per:]
    assert np.array_equal(abi, host) and np.array_equal(abi, dev)
    u, v, ur, st = RP.project(T, cam, b, xyz)
    st = np.where(flags & 1, st, RP.INACTIVE).astype(np.uint8)
    x, y = k["x"].copy(), k["y"].copy()
    m = RP.search(oracle_mod, st, (flags & 2) != 0, u, v, F(radius), ur, q, RW.build(x, y, b), x, y, b, tg, skip=skip, uright=uright,
                  init_dist=init, th_high=th_high, nn_ratio=ratio)
    want = np.concatenate([m["match_idx"], m["assigned"], [m["n_matches"]], m["status"].astype(np.int32), m["best_dist"], m["second_dist"], m["n_candidates"]])
    assert np.array_equal(abi, want.astype(np.int32))
    free = RP.search(oracle_mod, st, np.zeros(nq, bool), u, v, F(radius), ur, q, RW.build(x, y, b), x, y, b, tg, skip=skip, uright=uright,
                     init_dist=init, th_high=th_high, nn_ratio=ratio)
    print(f"matched {m['n_matches']}, differs from the claim-free answer in {(free['match_idx'] != m['match_idx']).sum()} queries")
    assert m["n_matches"] > 50 and (free["match_idx"] != m["match_idx"]).sum() > 10
