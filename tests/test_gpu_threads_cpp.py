"""The C++ layer under the reference's threading model: tests/cpp/threads_test.cpp runs XFmatcher::searchByBoW (frame form),
searchForTriangulation and searchByBoW (keyframe form) from three std::threads at once, each on a ctx of its own with a matcher built per call,
the static DescriptorDistance in between, and compares every iteration byte for byte with the answers it computed serially before the threads
existed.  It is compiled with g++ -pthread like the other drop-in programs and run as a child process under a time limit.  Those serial answers
come back as dumps in the formats of bow_test.cpp / triangulation_test.cpp and are compared here with the restatements (tests/ref_bow.py,
tests/ref_triangulation.py), the way tests/test_gpu_bow_cpp.py and tests/test_gpu_triangulation_cpp.py compare theirs."""
import os
import subprocess

import numpy as np
import pytest

import bow_rig as BR
import ref_bow as RB
import ref_frame as RF
import ref_triangulation as RT
import triangulation_rig as TR
from conftest import ROOT

pytestmark = pytest.mark.gpu

F = np.float32
ROUNDS = 10


def gxx(src, exe, *libs):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, src),
                           "-L" + os.path.join(ROOT, "xfeatslam_amd"), "-lxfeat_hip", *libs, "-Wl,-rpath," + os.path.join(ROOT, "xfeatslam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])


def test_cpp_three_matcher_threads(gpu_lib, oracle_mod, tmp_path):
    exe = str(tmp_path / "threads_test")
    gxx("tests/cpp/threads_test.cpp", exe, "-pthread")
    bs, ts = BR.Scene(), TR.Scene()
    ratios = {False: 0.6, True: 0.9}
    names = {False: "bow_frame", True: "bow_keyframe"}
    for keyframe in (False, True):
        BR.write_in(tmp_path / (names[keyframe] + "_in.bin"), bs.s1, bs.s2[0], keyframe, ratios[keyframe])
    cam = RF.camera(k1=0.0)
    (k1, img1), (k2, img2) = TR.rgbd(cam, ts.k1), TR.rgbd(cam, ts.k2[0])
    TR.write_in(tmp_path / "triangulation_in.bin", cam, k1, img1, k2, img2, ts.F12[0], ts.ep[0], 0)
    r = subprocess.run([exe, str(tmp_path / "bow_frame_in.bin"), str(tmp_path / "triangulation_in.bin"), str(tmp_path / "bow_keyframe_in.bin"), str(tmp_path / "out"),
                        str(ROUNDS)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "threads_test ok" in r.stdout, (r.returncode, r.stderr[-2000:])
    print(r.stdout.strip())
    # the serial answers every iteration was compared with are the restatements' answers
    for keyframe in (False, True):
        ratio = float(F(ratios[keyframe]))
        m = bs.want(oracle_mod, 0, 0, keyframe, nn_ratio=ratio)
        lit = RB.literal(bs.dist(oracle_mod, 0, 0), bs.s1["node_of"], bs.s1["active"], bs.s2[0]["node_of"], bs.s2[0]["has"] if keyframe else None, int(keyframe), nn_ratio=ratio)
        assert lit["n_matches"] == m["n_matches"] >= 20 and np.array_equal(lit["match12"], m["match12"]) and np.array_equal(lit["assigned2"], m["assigned2"])
        want = np.concatenate([[m["n_matches"]], m["status"].astype(np.int32), m["match12"], m["best_dist"], m["second_dist"], m["n_candidates"], m["assigned2"]]).astype(np.int32)
        raw = np.fromfile(tmp_path / f"out_{names[keyframe]}.bin", np.int32)
        assert len(raw) == len(want) and np.array_equal(raw, want), (keyframe, len(raw), len(want), np.nonzero(raw != want)[0][:8] if len(raw) == len(want) else None)
    m = RT.order_free(ts.dist(oracle_mod, 0), k1, k2, ts.F12[0], ts.ep[0], 0)
    lit = RT.literal(ts.dist(oracle_mod, 0), k1, k2, ts.F12[0], ts.ep[0], 0)
    pairs = np.array(lit["pairs"], np.int32).reshape(-1, 2)
    assert [tuple(p) for p in pairs.tolist()] == sorted(lit["pairs"]) and len(pairs) == m["n_matches"] >= 4
    want = np.concatenate([[m["n_matches"], len(pairs)], pairs.ravel(), m["status"].astype(np.int32), m["match12"], m["best_dist"], m["n_candidates"], m["n_geom"]]).astype(np.int32)
    raw = np.fromfile(tmp_path / "out_triangulation.bin", np.int32)
    assert len(raw) == len(want) and np.array_equal(raw, want), (len(raw), len(want))
