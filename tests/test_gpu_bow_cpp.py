"""The C++ layer of SearchByBoW: XFmatcher::searchByBoW (include/xfeat/ORBmatcher_xfeat.h), the host-vector form and the form on
device-resident sides (the descriptor blocks of records, uploaded node blobs and flag bytes), in the frame and the keyframe form, compiled
with g++ like the other drop-in classes: both produce the dump of the C ABI (xfh_bow_search) for the rig's scene written to a file, and
that dump is the restatement's answer (tests/ref_bow.py): matchOfQuery, assignedQuery, the return value and the last...() arrays."""
import os
import subprocess

import numpy as np
import pytest

import bow_rig as BR
import ref_bow as RB
from conftest import ROOT

pytestmark = pytest.mark.gpu

F = np.float32


def gxx(src, exe, *libs):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, src),
                           "-L" + os.path.join(ROOT, "xfeatslam_amd"), "-lxfeat_hip", *libs, "-Wl,-rpath," + os.path.join(ROOT, "xfeatslam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])


@pytest.fixture(scope="module")
def scene(gpu_lib):
    return BR.Scene()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("bow") / "bow_test")
    gxx("tests/cpp/bow_test.cpp", path)
    return path


@pytest.mark.parametrize("b,keyframe,ratio", [(0, False, 0.6), (0, True, 1.5), (1, True, 0.9)])
def test_cpp_search_by_bow(scene, oracle_mod, tmp_path, exe, b, keyframe, ratio):
    s1, s2 = scene.s1, scene.s2[b]
    n1, n2 = BR.N1, BR.N2
    assert (len(s1["node_of"]), len(s2["node_of"])) == (n1, n2)
    BR.write_in(tmp_path / "in.bin", s1, s2, keyframe, ratio)
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = np.fromfile(tmp_path / "out.bin", np.int32)
    m = scene.want(oracle_mod, 0, b, keyframe, nn_ratio=float(F(ratio)))
    lit = RB.literal(scene.dist(oracle_mod, 0, b), s1["node_of"], s1["active"], s2["node_of"], s2["has"] if keyframe else None, int(keyframe), nn_ratio=float(F(ratio)))
    assert lit["n_matches"] == m["n_matches"] >= 20 and np.array_equal(lit["match12"], m["match12"]) and np.array_equal(lit["assigned2"], m["assigned2"])
    want = np.concatenate([[m["n_matches"]], m["status"].astype(np.int32), m["match12"], m["best_dist"], m["second_dist"], m["n_candidates"], m["assigned2"]]).astype(np.int32)
    assert len(raw) == 3 * len(want), (len(raw), len(want))
    abi, host, dev = raw[:len(want)], raw[len(want):2 * len(want)], raw[2 * len(want):]
    assert np.array_equal(abi, want), np.nonzero(abi != want)[0][:8]
    assert np.array_equal(host, want) and np.array_equal(dev, want)
    print(f"version {b} keyframe form {keyframe} nn_ratio {ratio}: statuses {np.bincount(m['status'], minlength=5).tolist()}, matches {m['n_matches']}")
