"""The RGB-D frame-finish restatement (tests/ref_frame.py) and the host entry points xfh_undistort_points / xfh_camera_bounds.
No GPU.

The host functions and the model are the same IEEE float64 sequence rounded to fp32 once, so they are compared for EQUALITY of
bits over every integer pixel of a 640 x 480 image, the (0, 0) padding point and the four corners.  The model itself is checked
by something that does not share its iteration: its output pushed through the FORWARD distortion model in float64 must land on the
input pixel.  Five iterations do not converge everywhere; measured by this module for the reference's TUM1 camera over the integer
points 0..640 x 0..480 (test_forward_model_residual prints them):

    iterations   largest |du|    largest |dv|     (pixels)
        5          0.1103          0.0894
        4          0.3403          0.2758
       20          3.7e-5          1.9e-5         (the fp32 rounding of the output; 5e-9 before it)

The bound asserted is 1.5 x the five-iteration value, 0.165 px in u and 0.134 px in v: the margin covers another sampling of the
image and is half of what one lost iteration costs.  A four-iteration loop, swapped tangential coefficients or a dropped y*y term
exceed it (test_corrupted_models_are_caught).
"""
import os
import subprocess

import numpy as np
import pytest

import ref_frame as RF
from conftest import ROOT
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context

F = np.float32
RES_U, RES_V = 0.1103, 0.0894                # measured, see above
BOUND_U, BOUND_V = 1.5 * RES_U, 1.5 * RES_V

CAMERAS = {
    "tum1": RF.camera(),
    "k1_only": RF.camera(k1=-0.3, k2=0, p1=0, p2=0, k3=0),
    # 1 + k1 r2 + k2 r4 goes through zero inside the image: icdist < 0 for the outer pixels (chosen on the model, asserted below)
    "icdist_negative": RF.camera(k1=-1.2, k2=0.1, p1=0.001, p2=-0.002, k3=0),
}


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    import __graft_entry__ as g
    if not os.path.exists(capi.LIB_PATH):
        g.build()


def cam_struct(c):
    return capi.Camera(*[float(c[k]) for k in "fx fy cx cy k1 k2 p1 p2 k3 bf".split()], int(c["width"]), int(c["height"]))


def image_points(w=640, h=480):
    """every integer point 0..w x 0..h (the four corners and the (0, 0) padding point among them)"""
    gx, gy = np.meshgrid(np.arange(w + 1), np.arange(h + 1))
    return np.stack([gx.ravel(), gy.ravel()], 1).astype(F)


@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_host_functions_equal_the_model_bit_for_bit(name):
    c = CAMERAS[name]
    pts = image_points()
    model, neg = RF.undistort(c, pts, with_branch=True)
    print(f"{name}: {int(neg.sum())} of {len(pts)} points take the icdist < 0 exit")
    if name == "icdist_negative":
        assert neg.sum() >= 1 and (~neg).sum() >= 1
        assert np.abs(model[neg] - pts[neg]).max() < 1e-3             # the exit returns (x0, y0): back to the pixel up to rounding
    else:
        assert neg.sum() == 0
    got = Context.undistort_points(cam_struct(c), pts)
    diff = np.nonzero((got.view(np.uint32) != model.view(np.uint32)).any(axis=1))[0]
    assert len(diff) == 0, (len(diff), pts[diff[:4]], got[diff[:4]], model[diff[:4]])
    b = Context.camera_bounds(cam_struct(c))
    assert RF.same_bits(np.array(b, F), np.array(RF.bounds(c), F)), (b, RF.bounds(c))
    # the bounds are made of the corners the point call returns
    corners = Context.undistort_points(cam_struct(c), [[0, 0], [640, 0], [0, 480], [640, 480]])
    assert b[0] == min(corners[0, 0], corners[2, 0]) and b[3] == max(corners[2, 1], corners[3, 1])


def test_k1_zero_copies_the_input():
    c = RF.camera(k1=0.0)                                            # the other four stay non-zero
    assert all(float(c[k]) != 0 for k in ("k2", "p1", "p2", "k3"))
    pts = np.concatenate([image_points(), np.array([[np.nan, 1], [np.inf, -np.inf], [1e30, -0.0], [123.456, 78.9]], F)])
    got = Context.undistort_points(cam_struct(c), pts)
    assert np.array_equal(got.view(np.uint32), pts.view(np.uint32))
    assert np.array_equal(RF.undistort(c, pts).view(np.uint32), pts.view(np.uint32))
    assert Context.camera_bounds(cam_struct(c)) == (0.0, 0.0, 640.0, 480.0) and tuple(map(float, RF.bounds(c))) == (0.0, 0.0, 640.0, 480.0)


def residual(c, und):
    r = np.abs(RF.distort(c, und.astype(np.float64)) - image_points().astype(np.float64))
    return float(r[:, 0].max()), float(r[:, 1].max())


def test_forward_model_residual():
    c = CAMERAS["tum1"]
    pts = image_points()
    for it in (5, 4, 20):
        print(f"iterations {it}: largest residual {residual(c, RF.undistort(c, pts, iterations=it))}")
    ru, rv = residual(c, RF.undistort(c, pts))
    assert abs(ru - RES_U) < 5e-4 and abs(rv - RES_V) < 5e-4, (ru, rv)          # the docstring's figures are this module's own
    assert ru < BOUND_U and rv < BOUND_V
    hu, hv = residual(c, Context.undistort_points(cam_struct(c), pts))           # and the library, through the same independent check
    assert hu < BOUND_U and hv < BOUND_V


def depth_images(seed, h=480, w=640):
    """seeded raw uint16 depth with about a third zeros, and its fp32 conversion with the reference's factor"""
    rng = np.random.RandomState(seed)
    raw = rng.randint(1, 65536, (h, w)).astype(np.uint16)
    raw[rng.rand(h, w) < 1 / 3] = 0
    return raw, (raw.astype(F) * (F(1) / F(RF.TUM1_DEPTH_FACTOR))).astype(F)


def test_corrupted_models_are_caught():
    """every deliberate mistake fails the check of the stage it hits: bit-equality with the library / the residual bound for the
    undistortion, equality with the right model on the test's own data for the depth stage (the GPU test compares the device with
    the same data)"""
    c = CAMERAS["tum1"]
    pts = image_points()
    lib = Context.undistort_points(cam_struct(c), pts)
    for kw in (dict(iterations=4), dict(corrupt="swap_p"), dict(corrupt="r2_no_y")):
        m = RF.undistort(c, pts, **kw)
        ru, rv = residual(c, m)
        print(kw, "residual", (ru, rv), "points that differ from the library", int((m != lib).any(axis=1).sum()))
        assert not RF.same_bits(m, lib)                                          # check 1
        assert ru > BOUND_U and rv > BOUND_V                                     # check 3
    raw, f32 = depth_images(3)
    rng = np.random.RandomState(4)
    kp = np.stack([rng.randint(0, 640, 4096), rng.randint(0, 480, 4096)], 1).astype(F)
    kp[-500:] = 0                                                                # padding slots
    un = RF.undistort(c, kp)
    scale = F(1) / F(RF.TUM1_DEPTH_FACTOR)
    good = RF.stereo(c, kp, un, raw, scale)
    assert (good[0] == -1).mean() > 0.2 and (good[0] > 0).mean() > 0.5
    assert all(RF.same_bits(a, b) for a, b in zip(good, RF.stereo(c, kp, un, f32)))       # both depth types are one conversion
    for cor in ("depth_at_undistorted", "uright_from_raw", "d_ge_0", "scale_f64"):
        bad = RF.stereo(c, kp, un, raw, scale, corrupt=cor)
        nd, nr = int((bad[0] != good[0]).sum()), int((bad[1] != good[1]).sum())
        print(cor, "depth values that differ", nd, "uright", nr)
        assert nr > 0 and (nd > 0 or cor == "uright_from_raw")
    # d >= 0: a zero depth would give uright = -inf
    assert np.isinf(RF.stereo(c, kp, un, raw, scale, corrupt="d_ge_0")[1]).any() and np.isfinite(good[1]).all()


def test_depth_sampling_edges():
    """a self-check of the MODEL's pixel addressing on an image whose values name their pixel (it needs no library and passes
    without the feature); the library meets the same image and coordinates in
    tests/test_gpu_frame.py::test_depth_sampling_edges_on_the_device"""
    c = RF.camera(width=8, height=6)
    img = np.arange(48, dtype=np.uint16).reshape(6, 8) + 1
    xy = np.array([[0, 0], [7.9, 5.9], [-0.5, -0.99], [8, 0], [0, 6], [-1, 0], [np.nan, 1], [1, np.inf], [1e30, 1], [3.7, 2.2]], F)
    d = RF.sample_depth(c, img, xy, 1.0)
    assert d.tolist() == [1, 48, 1, 0, 0, 0, 0, 0, 0, 20]


def test_png16_reader(tmp_path):
    """include/xfeat/image_io.h load_png16: 16-bit greyscale PNGs with every row filter, big-endian samples; 8-bit and truncated
    files are refused, and the 8-bit loader keeps refusing 16-bit files"""
    from pngutil import write_png
    from test_gpu_frame_cpp import write_png16
    exe = str(tmp_path / "png16_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "png16_test.cpp"), "-lz", "-o", exe])
    rng = np.random.RandomState(1)
    img = rng.randint(0, 65536, (37, 53)).astype(np.uint16)
    img[0, :4] = [0, 0xFFFF, 0x00FF, 0xFF00]
    for k, filters in enumerate([(0,), (1,), (2,), (3,), (4,), (0, 1, 2, 3, 4)]):
        p = str(tmp_path / f"d{k}.png")
        write_png16(p, img, filters)
        r = subprocess.run([exe, p], capture_output=True)
        assert r.returncode == 0, (filters, r.stderr[-2000:])
        assert np.array_equal(np.frombuffer(r.stdout, np.uint16).reshape(37, 53), img), filters
    raw = open(p, "rb").read()
    for cut in (0, 7, 20, 40, len(raw) // 2):
        (tmp_path / "cut.png").write_bytes(raw[:cut])
        assert subprocess.run([exe, str(tmp_path / "cut.png")], capture_output=True).returncode == 1, cut
    write_png(str(tmp_path / "g8.png"), (img >> 8).astype(np.uint8))
    assert subprocess.run([exe, str(tmp_path / "g8.png")], capture_output=True).returncode == 1


def test_entry_points_without_gpu():
    import ctypes as C
    L = capi.lib()
    assert L.xfh_kernel_name(capi.K["FRAME_FINISH"]) == b"k_frame_finish" and capi.K["FRAME_FINISH"] == 15
    assert C.sizeof(capi.Camera) == 64
    cam = cam_struct(CAMERAS["tum1"])
    buf = np.zeros(64, np.uint8); p = buf.ctypes.data
    gb = capi.GridBounds(0, 0, 640, 480)
    assert L.xfh_frame_finish_records_device(None, p, 1, C.byref(cam), None, 0, 0, 1.0, C.byref(gb), 0, p, p, p, None) == 1
    assert L.xfh_frame_finish(None, p, 1, C.byref(cam), None, 0, 0, 1.0, p, p, p) == 1
    assert L.xfh_undistort_points(None, p, 1, p) == 1 and L.xfh_undistort_points(C.byref(cam), p, -1, p) == 1
    assert L.xfh_undistort_points(C.byref(cam), None, 0, None) == 0
    assert L.xfh_camera_bounds(C.byref(cam), None) == 1
    cam.width = 0
    assert L.xfh_camera_bounds(C.byref(cam), C.byref(gb)) == 1


def test_frame_host_code_under_sanitizers(tmp_path):
    """xfh_undistort_points / xfh_camera_bounds on NaN / Inf / 1e30 coordinates and coefficients, n = 0 and a zero focal length, in
    the AddressSanitizer + UBSan build of the HOST code (device code is not instrumented and nothing here runs on a GPU)"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "xfeatslam_amd", "csrc"), "asan", "-s", "-j8"])
    exe = str(tmp_path / "asan_frame_test")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "asan_frame_test.cpp"), "-L" + os.path.join(ROOT, "xfeatslam_amd"), "-lxfeat_hip_asan",
                           "-Wl,-rpath," + os.path.join(ROOT, "xfeatslam_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "asan_frame_test ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
