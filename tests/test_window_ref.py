"""The frame grid / window query restatement (tests/ref_window.py) against brute force, and the host side of the new
entry points: xfh_grid_unpack on well-formed and hostile blobs (also under AddressSanitizer + UBSan), xfh_grid_bytes, and the
argument errors that are detected before any HIP call.  No GPU."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_window as RW
from conftest import ROOT
from xfeatslam_amd import capi

F = np.float32
BOUNDS = {"vga": (0.0, 0.0, 640.0, 480.0), "720p": (0.0, 0.0, 1280.0, 720.0), "odd": (0.0, 0.0, 230.0, 170.0),
          "undist": (12.5, 7.25, 633.0, 471.5)}            # min > 0: keypoints left of / above the bounds round to negative cells


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    import __graft_entry__ as g
    if not os.path.exists(capi.LIB_PATH):
        g.build()


def keypoints(n, n_valid, bounds, seed):
    """n slots like an extraction record: n_valid integer-ish keypoints inside [0, max) at the front, default (0, 0) padding behind"""
    rng = np.random.RandomState(seed)
    x = np.zeros(n, F); y = np.zeros(n, F)
    x[:n_valid] = rng.randint(0, int(bounds[2]), n_valid); y[:n_valid] = rng.randint(0, int(bounds[3]), n_valid)
    return x, y


def brute_set(x, y, binned, u, v, r):
    u, v, r = F(u), F(v), F(r)
    return set(np.nonzero(binned & (np.abs(x - u) < r) & (np.abs(y - v) < r))[0].tolist())


@pytest.mark.parametrize("name", sorted(BOUNDS))
def test_restatement_against_brute_force(name):
    b = BOUNDS[name]
    x, y = keypoints(4096, 3500, b, 5)
    x[100:140] += F(0.37); y[200:260] -= F(0.21)                       # some non-integer coordinates
    px, py, ok = RW.cell_of(x, y, b)
    cs, items = RW.build(x, y, b)
    # dropped keypoints are exactly those whose rounded cell is 64 / 48 (the lost half cell) or negative
    mnx, mny, iw, ih = RW.geom(b)
    cx = np.array([float(np.float32((xi - mnx) * iw)) for xi in x]); cy = np.array([float(np.float32((yi - mny) * ih)) for yi in y])
    rx = np.sign(cx) * np.floor(np.abs(cx) + 0.5); ry = np.sign(cy) * np.floor(np.abs(cy) + 0.5)      # half away from zero, in float64 on fp32 values
    dropped = (rx < 0) | (rx >= 64) | (ry < 0) | (ry >= 48)
    assert np.array_equal(dropped, ~ok)
    assert np.all((rx[dropped] < 0) | (rx[dropped] == 64) | (ry[dropped] < 0) | (ry[dropped] == 48)) and dropped.any()
    assert (rx == 64).any() and (ry == 48).any()                        # the lost right-most / bottom half cell
    if name == "undist":
        assert (rx < 0).any() and (ry < 0).any()
    assert cs[0] == 0 and cs[-1] == len(items) == ok.sum() and np.all(np.diff(cs) >= 0)
    assert sorted(items.tolist()) == np.nonzero(ok)[0].tolist()
    cell = px.astype(int) * 48 + py.astype(int)
    for c in (0, 1, 48, 1000, 3071):
        m = items[cs[c]:cs[c + 1]]
        assert np.all(cell[m] == c) and np.all(np.diff(m) > 0)
    rng = np.random.RandomState(11)
    nq = 1000
    u = rng.uniform(b[0] - 30, b[2] + 30, nq).astype(F); v = rng.uniform(b[1] - 30, b[3] + 30, nq).astype(F)
    r = rng.choice([0.0, 0.5, 7.0, 15.0, 30.0, 100.0, 1e4], nq).astype(F)
    for q in range(nq):
        got = RW.features_in_area((cs, items), x, y, u[q], v[q], r[q], b)
        assert set(got.tolist()) == brute_set(x, y, ok, u[q], v[q], r[q]) and len(set(got.tolist())) == len(got)
        key = [(int(px[k]), int(py[k]), int(k)) for k in got]
        assert key == sorted(key)                                          # visiting order: column, row, index
    # not finite -> nothing; far outside -> the early returns
    for bad in [(np.nan, 10, 7), (10, np.inf, 7), (10, 10, np.nan), (10, 10, np.inf), (-1e30, 10, 7), (1e30, 10, 7), (10, -5000, 7)]:
        assert len(RW.features_in_area((cs, items), x, y, *bad, b)) == 0


def unpack_rc(blob, n, nbytes=None):
    cs = np.zeros(3073, np.int32); items = np.zeros(max(n, 1), np.int32); nb = C.c_int(-1)
    rc = capi.lib().xfh_grid_unpack(blob.ctypes.data, len(blob) if nbytes is None else nbytes, n, cs.ctypes.data, items.ctypes.data, C.byref(nb))
    return rc, cs, items, nb.value


def test_grid_unpack_wellformed_and_hostile():
    L = capi.lib()
    b = BOUNDS["vga"]
    n = 600
    x, y = keypoints(n, 500, b, 3)
    cs, items = RW.build(x, y, b)
    blob = RW.make_blob(cs, items, n, x, y, b)
    assert len(blob) == L.xfh_grid_bytes(n)
    rc, ocs, oit, nb = unpack_rc(blob, n)
    assert rc == 0 and nb == len(items) and np.array_equal(ocs, cs) and np.array_equal(oit[:nb], items) and np.all(oit[nb:] == -1)
    assert unpack_rc(blob, n, len(blob) - 1)[0] == 1 and unpack_rc(blob, n, 63)[0] == 1 and unpack_rc(blob, n, 0)[0] == 1      # truncated
    assert unpack_rc(blob, n + 1)[0] == 1 and unpack_rc(blob, -1)[0] == 1                                                     # another n
    for off, val in [(0, 7),                                 # magic
                     (8, n + 1), (8, -1),                    # n_binned out of range
                     (64, 5),                                # cell_start[0] != 0
                     (64 + 4 * 100, 1 << 30), (64 + 4 * 100, -3),     # cell_start not monotone / negative
                     (64 + 4 * 3072, len(items) - 1),        # the end is not n_binned
                     (12416, n), (12416 + 16 * 7, -1), (12416 + 16 * (len(items) - 1), 1 << 30)]:      # item >= n / negative
        bad = blob.copy(); bad[off:off + 4] = np.frombuffer(struct.pack("<i", val), np.uint8)
        assert unpack_rc(bad, n)[0] == 1, (off, val)
    assert L.xfh_grid_unpack(None, 100, 0, None, None, None) == 1
    # n = 0: header and cell_start only
    e = RW.make_blob(np.zeros(3073, np.int32), np.zeros(0, np.int32), 0, x, y, b)
    assert unpack_rc(e, 0)[0] == 0


def test_entry_points_without_gpu():
    L = capi.lib()
    assert L.xfh_grid_bytes(0) == 12416 and L.xfh_grid_bytes(4096) == 12416 + 16 * 4096 and L.xfh_grid_bytes(-5) == 0
    assert L.xfh_grid_bytes(capi.GRID_MAX_N) % 16 == 0 and capi.GRID_MAX_N >= 16384
    assert L.xfh_kernel_name(capi.K["GRID_BUILD"]) == b"k_grid_build" and L.xfh_kernel_name(capi.K["SEARCH_WINDOW"]) == b"k_search_window"
    assert L.xfh_kernel_name(10) == b"k_best2_csr" and L.xfh_kernel_name(12) == b"k_mnn_gemm_seg"       # existing ids keep their values
    gb = capi.GridBounds(0, 0, 640, 480)
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data
    # a NULL ctx is refused before anything touches HIP
    assert L.xfh_grid_build_device(None, p, 1, None, C.byref(gb), 0, p) == 1
    assert L.xfh_grid_build_records_device(None, p, 1, C.byref(gb), 0, p) == 1
    assert L.xfh_search_window_device(None, p, p, 1, p, p, 1, None, None, None, 256, p, p, p, p, p) == 1
    assert L.xfh_search_window(None, p, p, 1, p, C.byref(gb), p, 1, None, None, None, 256, p, p, p, p, p) == 1


def test_window_host_code_under_sanitizers(tmp_path):
    """xfh_grid_unpack on the same hostile blobs, and the argument checks, in the AddressSanitizer + UBSan build of the HOST code
    (make -C xfeatslam_amd/csrc asan; device code is not instrumented and nothing here runs on a GPU)"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "xfeatslam_amd", "csrc"), "asan", "-s", "-j8"])
    exe = str(tmp_path / "asan_window_test")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "asan_window_test.cpp"), "-L" + os.path.join(ROOT, "xfeatslam_amd"), "-lxfeat_hip_asan",
                           "-Wl,-rpath," + os.path.join(ROOT, "xfeatslam_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "asan_window_test ok" in r.stdout, r.stderr[-3000:]
