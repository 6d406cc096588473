"""XFgrid / XFmatcher::searchWindow (include/xfeat/ORBmatcher_xfeat.h) compiled with g++ like the other drop-in classes and
compared with tests/ref_window.py + the oracle's best / second-best loop."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_window as RW
from conftest import ROOT
from xfeatslam_amd import capi

pytestmark = pytest.mark.gpu

F = np.float32


def test_cpp_grid_and_search_window(gpu_lib, oracle_mod, tmp_path):
    exe = str(tmp_path / "window_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "window_test.cpp"),
                           "-L" + os.path.join(ROOT, "xfeatslam_amd"), "-lxfeat_hip", "-Wl,-rpath," + os.path.join(ROOT, "xfeatslam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    b = (0.0, 0.0, 640.0, 480.0)
    rng = np.random.RandomState(31)
    nt, nq, init = 2000, 300, 256
    k = np.zeros(nt, capi.KP_DTYPE)
    k["x"][:1700] = rng.randint(0, 640, 1700); k["y"][:1700] = rng.randint(0, 480, 1700); k["size"][:1700] = 1; k["angle"] = -1
    tg = np.zeros((nt, 64), F)
    d = rng.randn(1700, 64); tg[:1700] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    src = rng.randint(0, 1700, nq)
    q = tg[src] + 0.05 * rng.randn(nq, 64); q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)
    uvr = np.stack([k["x"][src] + rng.uniform(-4, 4, nq), k["y"][src] + rng.uniform(-4, 4, nq), rng.choice([7.0, 15.0, 30.0], nq)], 1).astype(F)
    uvr[:6] = [(0, 0, 15), (640, 480, 15), (-50, 10, 7), (700, 500, 100), (320, 240, 1e4), (np.nan, 5, 7)]
    skip = (rng.rand(nt) < 0.3).astype(np.uint8)
    uright = np.where(rng.rand(nt) < 0.5, k["x"] - rng.uniform(0, 30, nt), -1).astype(F)
    urq = (uvr[:, 0] - rng.uniform(0, 30, nq)).astype(F)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<4i4f", nq, nt, init, 1, *b))
        for a in (k, tg, q, uvr, skip, uright, urq):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = np.fromfile(tmp_path / "out.bin", np.int32)
    res = raw[:10 * nq].reshape(10, nq)
    grid = RW.build(k["x"], k["y"], b)
    for lo, kw in ((0, {}), (5, dict(skip=skip, uright=uright, ur_query=urq))):
        off, ind = RW.csr(grid, k["x"], k["y"], uvr, b, **kw)
        a = oracle_mod.best2_csr(q, tg, off, ind, init)
        for i in range(4):
            assert np.array_equal(res[lo + i], a[i]), (lo, i)
        assert np.array_equal(res[lo + 4], np.diff(off))
    # featuresInArea: the index lists themselves, in visiting order, from both kinds of grid
    off, ind = RW.csr(grid, k["x"], k["y"], uvr, b)
    o = 10 * nq
    for _ in range(2):
        for i in range(nq):
            cnt = int(raw[o]); o += 1
            assert np.array_equal(raw[o:o + cnt], ind[off[i]:off[i + 1]]), i
            o += cnt
    assert o == len(raw)
