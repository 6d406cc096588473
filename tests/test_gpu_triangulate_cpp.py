"""The C++ layer of the triangulation call: ORB_SLAM3::XFmatcher::triangulate (include/xfeat/ORBmatcher_xfeat.h), compiled with g++ like the other
drop-in classes, in its host-container form and its device form, on scenes of tests/triangulate_rig.py: the list of new points against the rule of
tests/ref_triangulate.py (integers equal, floats by bits), the headers, and the points it leaves on the device."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_triangulate as RG
import triangulate_rig as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def exe(gpu_lib, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("triangulate") / "triangulate_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "triangulate_test.cpp"),
                           "-L" + os.path.join(ROOT, "xfeatslam_amd"), "-lxfeat_hip", "-Wl,-rpath," + os.path.join(ROOT, "xfeatslam_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", path])
    return path


def scenes(oracle_mod, name):
    if name == "main":
        s = R.main_scene()
        return s, RG.snapshot_matches(s.dists(oracle_mod), s.k1, s.k2, s.F12, s.ep), R.main_params(), R.SCALE_FACTOR, True
    if name == "main_mono":
        s = R.main_scene()
        m = RG.snapshot_matches(s.dists(oracle_mod), s.k1, s.k2, s.F12, s.ep)
        s.k1 = dict(s.k1, ur=None); s.k2 = [dict(k, ur=None) for k in s.k2]
        return s, m, R.main_params(), R.SCALE_FACTOR, False
    o, m = R.planted()
    return o, m, R.planted_params(), 1.25 / 1.5, True


@pytest.mark.parametrize("name", ("main", "main_mono", "planted"))
def test_cpp_triangulate(tmp_path, exe, oracle_mod, name):
    s, m, P, scale_factor, stereo = scenes(oracle_mod, name)
    B, n1, n2 = len(s.k2), len(s.k1["xy"]), len(s.k2[0]["xy"])
    assert float(F(1.5) * F(scale_factor)) == float(P["ratio_factor"])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<4i9f", B, n1, n2, int(stereo), *[float(R.CAM[c]) for c in ("fx", "fy", "cx", "cy", "bf")], float(P["sigma2"]), scale_factor,
                            float(P["scale_last"]), float(P["far_th"])))
        for k in [s.k1] + list(s.k2):
            f.write(k["xy"].astype(F).tobytes() + (k["ur"].astype(F).tobytes() + k["depth"].astype(F).tobytes() if stereo else b"") + np.asarray(k["Tcw"], F).tobytes()
                    + np.asarray(k["Ow"], F).tobytes())
        f.write(np.ascontiguousarray(m, np.int32).tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    w = RG.rule_from_matches(P, s.k1, s.k2, m)
    n = w["n_new"]
    want = struct.pack("<i", n)
    for j in range(n):
        i, b = int(w["new_idx1"][j]), int(w["new_b"][j])
        mx = w["new_dist"][j][2]
        want += struct.pack("<4i", i, b, int(w["new_idx2"][j]), int(w["kind"][b, i] != 0)) + w["new_xyz"][j].tobytes() + w["new_normal"][j].tobytes()
        want += F(mx / P["scale_last"]).tobytes() + F(mx).tobytes() + w["new_dist"][j].tobytes()
    want += w["header"].astype(np.int32).tobytes()
    raw = open(tmp_path / "out.bin", "rb").read()
    assert len(raw) == 2 * len(want) + 12 * n
    assert raw[:len(want)] == want, "host-container form"
    assert raw[len(want):2 * len(want)] == want, "device form"
    assert raw[2 * len(want):] == w["new_xyz"][:n].tobytes()                                   # the points on the device are the points returned
    print(f"{name}: {n} new map points, headers {w['header'].tolist()}")
