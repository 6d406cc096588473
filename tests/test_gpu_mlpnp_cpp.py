"""The C++ layer of the MLPnP solver: ORB_SLAM3::XFmlpnpSolver (include/xfeat/MLPnPsolver_xfeat.h), compiled with g++ like the other drop-in classes,
driven through the call sequence of Tracking.cc:3715-3773 -- SetRansacParameters, then iterate(chunk) three times on one solver, each call resuming
where the last returned -- in its device form and its host-container form, beside the C ABI's host-pointer form with start_iter, on scenes of
tests/mlpnp_rig.py: the three give the same bool, bNoMore, nInliers, header, pose, flags and mvpMapPoints, and these equal the rule of
tests/ref_mlpnp.py called with start_iter = the consumed count of the call before (integers equal, Tcw within one float32 step).  The class builds
its tables itself from (prob, minInliers, maxIts, eps), so the tables of the scenes are checked against it on the way."""
import os
import struct
import subprocess

import numpy as np
import pytest

import mlpnp_rig as G
import ref_mlpnp as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
F = np.float32
PARAMS = dict(n70=0.5, its70=0.4, n_equals_min=0.5, n9=0.5, none=0.5, planar=0.5)          # the eps each scene's tables were made with


@pytest.fixture(scope="module")
def exe(gpu_lib, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("mlpnp") / "mlpnp_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "mlpnp_test.cpp"),
                           "-L" + os.path.join(ROOT, "xfeatslam_amd"), "-lxfeat_hip", "-Wl,-rpath," + os.path.join(ROOT, "xfeatslam_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", path])
    return path


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_cpp_mlpnp_solver(tmp_path, exe, name):
    sc = G.rig()[name]
    n, nq, iters = sc["assigned"].shape[1], sc["points"].shape[1], sc["draws"].shape[1]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<7i5f", n, nq, iters, G.RAND_MAX, sc["chunk"], 0, 1, *[float(c) for c in sc["cam"]], sc["max_err"]))
        for a, dt in ((sc["xy"], F), (sc["assigned"][0], np.int32), (sc["points"][0], F), (sc["valid"][0], np.uint8), (sc["tables"][0], np.int32),
                      (sc["tables"][1], np.int32), (sc["draws"][0], np.int32)):
            f.write(np.ascontiguousarray(a, dt).tobytes())
        f.write(struct.pack("<diiff", 0.99, 10, 300, PARAMS[name], 5.991))
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = np.frombuffer(open(tmp_path / "out.bin", "rb").read(), np.uint8)
    per = 12 + 64 + 48 + n + 4 * n
    assert len(raw) == 9 * per
    start, cache, said = 0, {}, []
    for call in range(3):
        w = G.rule_of(sc, start_iter=start, cache=cache)
        st = int(w["header"][1])
        ok = st in (R.REFINED, R.BEST)
        for k, form in enumerate(("device overload", "host containers", "xfh_mlpnp_solve")):
            blk = raw[(3 * k + call) * per:(3 * k + call + 1) * per]
            assert blk[:12].view(np.int32).tolist() == [int(ok), int(st != R.REFINED), int(w["header"][5]) if ok else 0], (form, call)
            got = {"header": blk[12:76].view(np.int32)[None], "Tcw": blk[76:124].view(F)[None], "inliers": blk[124:124 + n][None], "assigned_out": blk[124 + n:].view(np.int32)[None]}
            z = dict(w)
            if st == R.TOO_FEW:                                                 # nothing but the header is written: the program's own initial values
                z.update(Tcw=np.zeros(12, F), inliers=np.zeros(n, np.uint8), assigned_out=np.full(n, -1, np.int32))
            elif not ok:
                z.update(Tcw=np.zeros(12, F))
            G.assert_equals_rule(got, z, 0)
        said.append(R.STATUS[st])
        if st != R.TOO_FEW:
            start = int(w["header"][8])
    print(f"{name}: {said}")
