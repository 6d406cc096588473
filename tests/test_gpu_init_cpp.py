"""The C++ and Python layers of SearchForInitialization: both XFmatcher::searchForInitialization overloads (include/xfeat/ORBmatcher_xfeat.h,
compiled with g++ like the other drop-in classes) and the Python ORBmatcher.SearchForInitialization produce the dump of the C ABI's host
form xfh_init_search for the rig's scene, and that dump is the literal restatement's answer (tests/ref_init.py)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_frame as RF
import ref_init as RI
import ref_window as RW
from conftest import ROOT
from init_rig import InitRig
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context, ORBmatcher

pytestmark = pytest.mark.gpu

F = np.float32


def gxx(src, exe, *libs):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, src),
                           "-L" + os.path.join(ROOT, "xfeatslam_amd"), "-lxfeat_hip", *libs, "-Wl,-rpath," + os.path.join(ROOT, "xfeatslam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])


@pytest.fixture(scope="module")
def scene(gpu_lib, weights_dense, oracle_mod):
    """the 1000-feature rig's problem 0 on the host.  The C++ side builds the grid from the UNDISTORTED keypoints with the image as bounds (k1 = 0
    in the camera it is given)."""
    r = InitRig(gpu_lib, weights_dense[1], 1000, 1200, oracle_mod)
    s = dict(xy=r.xy[1].copy(), q=r.q.copy(), pm=r.pm.copy(), tg=r.tg.copy(), flags=(np.random.RandomState(9).rand(r.nf) >= 0.1).astype(np.uint8))
    r.close()
    return s


@pytest.mark.parametrize("window,use_flags", [(100, 0), (10, 1)])
def test_cpp_and_python_layers(scene, oracle_mod, tmp_path, window, use_flags):
    exe = str(tmp_path / "init_test")
    gxx("tests/cpp/init_test.cpp", exe)
    s = scene
    cam = RF.camera(k1=0.0)
    b = tuple(float(x) for x in RF.bounds(cam))
    n = len(s["xy"])
    ratio = 0.9
    k = np.zeros(n, capi.KP_DTYPE); k["x"] = s["xy"][:, 0]; k["y"] = s["xy"][:, 1]; k["size"] = 1; k["angle"] = -1
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<4i4f", n, window, use_flags, 0, ratio, 0.0, 0.0, 0.0))
        f.write(struct.pack("<10f6i", *[float(cam[c]) for c in "fx fy cx cy k1 k2 p1 p2 k3 bf".split()], int(cam["width"]), int(cam["height"]), 0, 0, 0, 0))
        for a, t in ((k, None), (s["tg"], F), (s["q"], F), (s["pm"], F), (s["flags"], np.uint8)):
            f.write(np.ascontiguousarray(a, t).tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = np.fromfile(tmp_path / "out.bin", np.int32)
    per = 11 * n + 1
    assert len(raw) == 3 * per
    abi, host, dev = (raw[i * per:(i + 1) * per] for i in range(3))
    assert np.array_equal(abi, host) and np.array_equal(abi, dev)
    # the restatement on the same inputs
    x, y = s["xy"][:, 0].copy(), s["xy"][:, 1].copy()
    flags = s["flags"] if use_flags else None
    w = RI.literal(oracle_mod, s["q"], s["pm"], float(window), RW.build(x, y, b), x, y, b, s["tg"], flags=flags, nn_ratio=ratio, txy=s["xy"])
    want = np.concatenate([[w["n_matches"]], w["matches12"], w["status"].astype(np.int32), w["claim_idx"], w["best_dist"], w["second_dist"], w["n_window"], w["n_tested"],
                           w["matches21"], w["matched_distance"], np.ascontiguousarray(w["prev_out"], F).reshape(-1).view(np.int32)])
    assert np.array_equal(abi, want.astype(np.int32)), np.nonzero(abi != want)[0][:8]
    print(f"window {window} flags {use_flags}: statuses {np.bincount(w['status'], minlength=4).tolist()}, matches {w['n_matches']}, retractions {w['retractions']}")
    assert w["n_matches"] > 0
    if not use_flags:
        # the Python drop-in class (it has no flags: the reference's call)
        ctx = Context(nfeatures=n, max_height=int(cam["height"]), max_width=int(cam["width"]))
        nm, m12, pm = ORBmatcher(ratio, True, ctx).SearchForInitialization(k[:n], s["q"], k, s["tg"], s["pm"], windowSize=window, bounds=b)
        assert nm == w["n_matches"] and np.array_equal(m12, w["matches12"]) and pm.tobytes() == np.ascontiguousarray(w["prev_out"], F).tobytes()
        nm2, m122, _ = ORBmatcher(ratio, True, ctx).SearchForInitialization(k[:n], s["q"], k, s["tg"], s["pm"], windowSize=window)      # bounds = the ctx' image
        assert (nm2, m122.tolist()) == (nm, m12.tolist()) or b != (0.0, 0.0, float(cam["width"]), float(cam["height"]))
        ctx.close()
