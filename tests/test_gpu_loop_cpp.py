"""The C++ layer of the loop-closing / relocalisation matchers: XFmatcher::searchByProjection(Sim3Form / RelocForm, ...) and
XFmatcher::searchBySim3 (include/xfeat/ORBmatcher_xfeat.h), host-vector and device / XFgrid overloads, compiled with g++ like the other
drop-in classes: both produce the dump of the C ABI's host forms (xfh_map_projection_search, xfh_sim3_search) for the rig's scene written
to a file, and that dump is the sequential restatement's answer (tests/ref_loop.py)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_frame as RF
import ref_loop as RL
import ref_window as RW
from conftest import ROOT
from loop_rig import NL, SF, LoopRig
from xfeatslam_amd import capi

pytestmark = pytest.mark.gpu

F = np.float32


def gxx(src, exe, *libs):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, src),
                           "-L" + os.path.join(ROOT, "xfeatslam_amd"), "-lxfeat_hip", *libs, "-Wl,-rpath," + os.path.join(ROOT, "xfeatslam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])


@pytest.fixture(scope="module")
def scene(gpu_lib, weights_dense, oracle_mod):
    """the 1000-feature rig's problem 0 on the host: frame 0's undistorted keypoints and descriptors, its map points, and the keyframe pair
    of SearchBySim3 (both keyframes are frame 0).  The C++ side builds the grid from the UNDISTORTED keypoints with the image as bounds
    (k1 = 0 in the camera it is given)."""
    lr = LoopRig(gpu_lib, weights_dense[1], 1000, 901, oracle_mod)
    rg = lr.rig
    s = dict(xy=rg.xy[0].copy(), tg=rg.recs[0][1].copy(), map={k: np.array(v, copy=True) for k, v in lr.scene.items() if k != "spots"}, T=lr.poses[0].copy(),
             Ow=lr.Ow[0].copy(), pair=[a.copy() for a in lr.pairs[0]], s1={k: v.copy() for k, v in lr.s1[0].items()}, s2={k: v.copy() for k, v in lr.s2[0].items()})
    lr.close()
    return s


@pytest.mark.parametrize("form,th", [(0, 4.0), (1, 15.0), (2, 15.0)])
def test_cpp_loop(scene, oracle_mod, tmp_path, form, th):
    exe = str(tmp_path / "loop_test")
    gxx("tests/cpp/loop_test.cpp", exe)
    s, m = scene, scene["map"]
    cam = RF.camera(k1=0.0)
    b = tuple(float(x) for x in RF.bounds(cam))
    n = len(s["xy"])
    ratio, orbdist = 1.5, 100
    k = np.zeros(n, capi.KP_DTYPE); k["x"] = s["xy"][:, 0]; k["y"] = s["xy"][:, 1]; k["size"] = 1; k["angle"] = -1
    T1, T2, M21, M12 = s["pair"]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<4i4f", n, NL, form, 0, th, SF, ratio, float(orbdist)))
        f.write(struct.pack("<10f6i", *[float(cam[c]) for c in "fx fy cx cy k1 k2 p1 p2 k3 bf".split()], int(cam["width"]), int(cam["height"]), 0, 0, 0, 0))
        for a, t in ((s["T"], F), (s["Ow"], F), (T1, F), (T2, F), (M21, F), (M12, F), (k, None), (s["tg"], F), (m["taken"], np.uint8), (m["qdesc"], F), (m["xyz"], F),
                     (m["normals"], F), (m["dist"], F), (m["flags"], np.uint8)):
            f.write(np.ascontiguousarray(a, t).tobytes())
        for sd in (s["s1"], s["s2"]):
            for a, t in ((sd["points"], F), (sd["dist"], F), (sd["mp_desc"], F), (sd["flags"], np.uint8)):
                f.write(np.ascontiguousarray(a, t).tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = np.fromfile(tmp_path / "out.bin", np.int32)
    per_map, per_sim3 = 7 * n + 1, 13 * n + 1
    assert len(raw) == 3 * per_map + 3 * per_sim3
    abi, host, dev = (raw[i * per_map:(i + 1) * per_map] for i in range(3))
    assert np.array_equal(abi, host) and np.array_equal(abi, dev)
    rest = raw[3 * per_map:]
    abi3, host3, dev3 = (rest[i * per_sim3:(i + 1) * per_sim3] for i in range(3))
    assert np.array_equal(abi3, host3) and np.array_equal(abi3, dev3)
    # the restatement on the same inputs
    x, y = s["xy"][:, 0].copy(), s["xy"][:, 1].copy()
    grid = RW.build(x, y, b)
    cform = (RL.FORM_SIM3, RL.FORM_SIM3_KF, RL.FORM_RELOC)[form]
    accept = float(F(orbdist)) if form == 2 else float(F(RL.TH_LOW) * F(ratio))
    u, v, rr, lv, st = RL.map_project(s["T"], s["Ow"], cam, b, th, SF, NL, cform, m["xyz"], m["normals"], m["dist"])
    act = (m["flags"] & 1) != 0
    st = np.where(act, st, RL.INACTIVE).astype(np.uint8)
    w = RL.map_search(oracle_mod, st, lv, u, v, rr, m["qdesc"], grid, x, y, b, s["tg"], taken=m["taken"], accept_max=accept)
    want = np.concatenate([[w["n_matches"]], w["match_idx"], w["status"].astype(np.int32), w["best_dist"], w["n_window"], w["n_tested"], np.where(act, lv, -1), w["assigned"]])
    assert np.array_equal(abi, want.astype(np.int32)), np.nonzero(abi != want)[0][:8]
    print(f"form {form} th {th}: statuses {np.bincount(w['status'], minlength=8).tolist()}, matches {w['n_matches']}")
    parts = []
    for q, T, M in ((s["s1"], T1, M21), (s["s2"], T2, M12)):
        u, v, rr, lv, st = RL.sim3_project(T, M, cam, b, th, SF, NL, q["points"], q["dist"])
        act = (q["flags"] & 1) != 0
        st = np.where(act, st, RL.INACTIVE).astype(np.uint8)
        w = RL.sim3_search(oracle_mod, st, lv, u, v, rr, q["mp_desc"], grid, x, y, b, s["tg"])
        parts.append((w, np.where(act, lv, -1)))
    m12, nfound = RL.sim3_agree(parts[0][0]["match"], parts[1][0]["match"])
    want = np.concatenate([[nfound], m12] + [a for w, lvl in parts for a in (w["match"], w["status"].astype(np.int32), w["best_dist"], w["n_window"], w["n_tested"], lvl)])
    assert np.array_equal(abi3, want.astype(np.int32)), np.nonzero(abi3 != want)[0][:8]
    print(f"SearchBySim3 th {th}: agreed {nfound}")
    assert nfound > 0
