"""The C++ layer of the RGB-D frame finish: XFgrid::buildFromRecord with a camera (include/xfeat/ORBmatcher_xfeat.h) compiled with
g++ like the other drop-in classes, and examples/frontend_replay.cpp --rgbd on a short synthetic sequence whose 16-bit depth PNGs
this test writes (include/xfeat/image_io.h: load_png16); both compared with tests/ref_frame.py / tests/ref_window.py and the
oracle's best / second-best loop, bit for bit."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import ref_frame as RF
import ref_window as RW
from conftest import ROOT
from xfeatslam_amd import capi, synth, weights as WT

pytestmark = pytest.mark.gpu

F = np.float32
CAM_FIELDS = "fx fy cx cy k1 k2 p1 p2 k3 bf".split()


def gxx(src, exe, *libs):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, src),
                           "-L" + os.path.join(ROOT, "xfeatslam_amd"), "-lxfeat_hip", *libs, "-Wl,-rpath," + os.path.join(ROOT, "xfeatslam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])


def write_png16(path, img, filters=(0, 1, 2, 3, 4)):
    """16-bit greyscale PNG (big-endian samples), rows cycling through the five filter types, which work on bytes two apart"""
    h, w = img.shape
    rows = img.astype(">u2").view(np.uint8).reshape(h, 2 * w)
    raw = bytearray()
    prev = np.zeros(2 * w, np.uint8)
    z2 = np.zeros(2, np.uint8)
    for y in range(h):
        cur = rows[y]
        ft = filters[y % len(filters)]
        a = np.concatenate([z2, cur[:-2]]).astype(np.int32); c = np.concatenate([z2, prev[:-2]]).astype(np.int32); b = prev.astype(np.int32)
        p = a + b - c
        pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
        pred = [0 * a, a, b, (a + b) >> 1, np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))][ft]
        raw.append(ft); raw += ((cur.astype(np.int32) - pred) & 255).astype(np.uint8).tobytes()
        prev = cur

    def chunk(ty, data):
        return struct.pack(">I", len(data)) + ty + data + struct.pack(">I", zlib.crc32(ty + data) & 0xffffffff)
    comp = zlib.compress(bytes(raw), 6)
    half = len(comp) // 2
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 0, 0, 0, 0)) + chunk(b"IDAT", comp[:half]) + chunk(b"IDAT", comp[half:])
                + chunk(b"IEND", b""))


def cam_bytes(c):
    return struct.pack("<10f6i", *[float(c[k]) for k in CAM_FIELDS], int(c["width"]), int(c["height"]), 0, 0, 0, 0)


@pytest.mark.parametrize("dtype", [capi.DEPTH_U16, capi.DEPTH_F32, capi.DEPTH_NONE])
def test_cpp_grid_from_record_with_camera(gpu_lib, oracle_mod, tmp_path, dtype):
    exe = str(tmp_path / "frame_test")
    gxx("tests/cpp/frame_test.cpp", exe)
    cam = RF.camera()
    H, W = 480, 640
    rng = np.random.RandomState(41)
    nt, nq, init = 2000, 300, 256
    k = np.zeros(nt, capi.KP_DTYPE)
    k["x"][:1700] = rng.randint(0, W, 1700); k["y"][:1700] = rng.randint(0, H, 1700); k["size"][:1700] = 1; k["angle"] = -1
    k["x"][:4] = [0, 639, 0, 639]; k["y"][:4] = [0, 0, 479, 479]                  # the corner pixels
    tg = np.zeros((nt, 64), F)
    d = rng.randn(1700, 64); tg[:1700] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    src = rng.randint(0, 1700, nq)
    q = tg[src] + 0.05 * rng.randn(nq, 64); q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)
    raw_xy = np.stack([k["x"], k["y"]], 1).astype(F)
    m_xy = RF.undistort(cam, raw_xy)
    uvr = np.stack([m_xy[src, 0] + rng.uniform(-4, 4, nq), m_xy[src, 1] + rng.uniform(-4, 4, nq), rng.choice([7.0, 15.0, 30.0], nq)], 1).astype(F)
    uvr[:5] = [(12, 15, 15), (626, 473, 15), (-50, 10, 7), (320, 240, 1e4), (np.nan, 5, 7)]
    yy, xx = np.mgrid[0:H, 0:W]
    depth16 = np.array([0, 5000, 10000], np.uint16)[(xx // 8 + yy // 8) % 3] + (rng.randint(0, 200, (H, W)) * ((xx // 8 + yy // 8) % 3 > 0)).astype(np.uint16)
    scale = F(1) / F(RF.TUM1_DEPTH_FACTOR)
    img = {capi.DEPTH_U16: depth16, capi.DEPTH_F32: (depth16.astype(F) * scale).astype(F), capi.DEPTH_NONE: None}[dtype]
    sc = scale if dtype == capi.DEPTH_U16 else F(1)
    urq = (uvr[:, 0] - rng.uniform(15, 45, nq)).astype(F)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<4i", nq, nt, init, dtype) + cam_bytes(cam) + struct.pack("<f", float(sc)))
        for a in (k, tg, q, uvr, urq) + ((img,) if img is not None else ()):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = np.fromfile(tmp_path / "out.bin", np.uint8)
    o = 0

    def take(dt, n):
        nonlocal o
        a = raw[o:o + 4 * n].view(dt); o += 4 * n
        return a
    b = tuple(take(F, 4))
    assert RF.same_bits(np.array(b, F), np.array(RF.bounds(cam), F))
    xy = take(F, 2 * nt).reshape(nt, 2); ur = take(F, nt); dz = take(F, nt)
    assert RF.same_bits(xy, m_xy)
    md, mr = RF.stereo(cam, raw_xy, xy, img, sc)
    assert RF.same_bits(dz, md) and RF.same_bits(ur, mr)
    if img is not None:
        assert (dz > 0).mean() > 0.4 and (dz == -1).mean() > 0.2
    res = take(np.int32, 5 * nq).reshape(5, nq)
    x1, y1 = xy[:, 0].copy(), xy[:, 1].copy()
    grid = RW.build(x1, y1, b)
    off, ind = RW.csr(grid, x1, y1, uvr, b, uright=ur, ur_query=urq)
    a = oracle_mod.best2_csr(q, tg, off, ind, init)
    for i in range(4):
        assert np.array_equal(res[i], a[i]), i
    assert np.array_equal(res[4], np.diff(off))
    off_all, ind_all = RW.csr(grid, x1, y1, uvr, b)
    if img is not None:
        assert off[-1] < off_all[-1]                                               # the right-coordinate check removes something
    for i in range(nq):                                                            # featuresInArea on the undistorted grid, visiting order
        cnt = int(take(np.int32, 1)[0])
        assert np.array_equal(take(np.int32, cnt), ind_all[off_all[i]:off_all[i + 1]]), i
    assert np.all(take(F, nt) == -1) and np.all(take(F, nt) == -1)                 # rebuilt without a depth image
    assert o == len(raw)
    # the grid of the RAW keypoints would answer differently: the inputs exercise distortion
    off_raw, _ = RW.csr(RW.build(k["x"], k["y"], (0.0, 0.0, 640.0, 480.0)), k["x"], k["y"], uvr, (0.0, 0.0, 640.0, 480.0))
    assert (np.diff(off_raw) != np.diff(off_all)).any()


def _read_dump(path, n, nf, rgbd):
    """frames of a frontend_replay dump -> [(nv, kp[nk][3], matches bytes, xy_un, uright, depth)], and the bytes without the --rgbd arrays"""
    raw = open(path, "rb").read()
    o, out, plain = 0, [], bytearray()
    for _ in range(n):
        s = o
        nv, nk = struct.unpack_from("<2i", raw, o); o += 8
        kp = np.frombuffer(raw, F, 3 * nk, o).reshape(nk, 3); o += 12 * nk
        nm, = struct.unpack_from("<i", raw, o); o += 4
        mb = raw[o:o + 12 * nm]; o += 12 * nm
        plain += raw[s:o]
        extra = (None, None, None)
        if rgbd:
            assert nk == nf
            xy = np.frombuffer(raw, F, 2 * nk, o).reshape(nk, 2); o += 8 * nk
            ur = np.frombuffer(raw, F, nk, o); o += 4 * nk
            dz = np.frombuffer(raw, F, nk, o); o += 4 * nk
            extra = (xy, ur, dz)
        out.append((nv, kp, mb) + extra)
    assert o == len(raw)
    return out, bytes(plain)


def test_frontend_replay_rgbd(gpu_lib, tmp_path):
    exe = str(tmp_path / "frontend_replay")
    gxx("examples/frontend_replay.cpp", exe, "-lz")
    (tmp_path / "w.xfhw").write_bytes(WT.pack_blob(WT.make_synthetic(1234, 6.0)))
    os.makedirs(tmp_path / "rgb"); os.makedirs(tmp_path / "depth")
    from pngutil import write_png
    nf, H, W, n = 300, 96, 160, 4
    cam = RF.camera(fx=129.3, fy=129.1, cx=79.7, cy=51.1, width=W, height=H)       # the TUM1 coefficients on a 160 x 96 image
    base = synth.image(H, W + 8 * n, 31)
    rng = np.random.RandomState(6)
    lines, depths = [], []
    for i in range(n):
        write_png(str(tmp_path / "rgb" / f"{i}.png"), base[:, 8 * i:8 * i + W], [0, 1, 2, 3, 4])
        dimg = rng.randint(1, 65536, (H, W)).astype(np.uint16); dimg[rng.rand(H, W) < 1 / 3] = 0
        dimg[0, 0], dimg[-1, -1] = 0xFFFF, 0x0100                                    # both bytes of a sample matter
        write_png16(str(tmp_path / "depth" / f"{i}.png"), dimg)
        depths.append(dimg)
        lines.append(f"{i}.0 rgb/{i}.png {i}.0 depth/{i}.png")
    (tmp_path / "assoc.txt").write_text("\n".join(lines) + "\n")
    factor = 5000.0
    opt = ",".join(repr(float(cam[k])) for k in CAM_FIELDS) + f",{factor}"
    scale = F(1) / F(factor)

    def run(name, *args):
        dump = str(tmp_path / name)
        r = subprocess.run([exe, str(tmp_path / "w.xfhw"), str(tmp_path / "assoc.txt"), str(tmp_path), "--dump", dump, *args], capture_output=True, text=True,
                           env=dict(os.environ, XFH_NFEATURES=str(nf)))
        assert r.returncode == 0, r.stderr
        return dump
    plain, plain_fast = run("plain.bin"), run("plain_fast.bin", "--fast")
    d_host, d_fast = run("rgbd.bin", "--rgbd", opt), run("rgbd_fast.bin", "--fast", "--rgbd", opt)
    assert open(d_host, "rb").read() == open(d_fast, "rb").read()                   # xfh_frame_finish and XFgrid on the record: the same values
    frames, stripped = _read_dump(d_fast, n, nf, True)
    # without the option the dump is the existing format, in both modes, and the option only ADDS the three arrays
    assert open(plain, "rb").read() == open(plain_fast, "rb").read() == stripped
    _read_dump(plain, n, nf, False)
    for i, (nv, kp, _, xy, ur, dz) in enumerate(frames):
        assert nv > 50
        raw_xy = np.ascontiguousarray(kp[:, :2])
        assert RF.same_bits(xy, RF.undistort(cam, raw_xy)), i
        md, mr = RF.stereo(cam, raw_xy, xy, depths[i], scale)
        assert RF.same_bits(dz, md) and RF.same_bits(ur, mr), i
        assert (dz > 0).sum() > 20 and (dz == -1).sum() > 10
    # a sequence without readable 16-bit depth maps is refused, not silently finished without depth
    write_png(str(tmp_path / "depth" / "0.png"), (depths[0] >> 8).astype(np.uint8))
    r = subprocess.run([exe, str(tmp_path / "w.xfhw"), str(tmp_path / "assoc.txt"), str(tmp_path), "--rgbd", opt], capture_output=True, text=True,
                       env=dict(os.environ, XFH_NFEATURES=str(nf)))
    assert r.returncode == 2 and "depth map" in r.stderr
