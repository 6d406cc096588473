#!/usr/bin/env python
"""Device time of finishing RGB-D frames on the device (profiles/frame_finish.md).

  new call      : xfh_frame_finish_records_device (k_frame_finish: undistort + depth / right coordinate + grid), TUM1 camera,
                  raw uint16 depth, one launch for B records
  grid alone    : xfh_grid_build_records_device (k_grid_build) on the same records.  `--grid-only` measures nothing else and binds
                  only the symbols the loaded library exports, so XFEAT_HIP_LIB=<libxfeat_hip.so of the parent commit> gives the
                  parent's figure on the same box
  host route    : per frame D2H of the keypoints, xfh_undistort_points and the depth lookup on the host, H2D of the undistorted
                  keypoints, xfh_grid_build_device -- what a caller with distortion had to do before (host wall clock, the
                  stream drained at the end)

4096 slots (3500 valid + padding), B = 1 and B = 64.  The ctx runs on a torch stream of this tool, torch.cuda events on that
stream bracket `--iters` back-to-back repetitions after `--warmup`; the device figures are taken five times (min .. max).

    python tools/frame_finish_timing.py [--iters 200] [--grid-only --label "parent commit"] [--out profiles/frame_finish_table.md]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_window as RW                                    # noqa: E402
from xfeatslam_amd import capi                             # noqa: E402

F = np.float32
NF, H, W = 4096, 480, 640
TUM1 = (517.306408, 516.469215, 318.643040, 255.313989, 0.262383, -0.953104, -0.005358, 0.002628, 1.163314, 40.0, W, H)


def records(ctx, B, n_valid=3500, seed=1):
    """B records as the extractor lays them out: header, keypoints (valid at both ends, padding between), descriptors unused"""
    rng = np.random.RandomState(seed)
    raw = np.zeros((B, ctx.rec_bytes), np.uint8)
    for b in range(B):
        mono = n_valid // 2
        valid = RW.valid_slots(NF, n_valid, mono)
        k = np.zeros(NF, capi.KP_DTYPE)
        k["x"][valid] = rng.randint(0, W, n_valid); k["y"][valid] = rng.randint(0, H, n_valid); k["size"][valid] = 1; k["angle"] = -1
        raw[b, :16] = np.array([n_valid, mono, n_valid, 0], np.int32).view(np.uint8)
        raw[b, ctx.kps_off:ctx.kps_off + 28 * NF] = k.view(np.uint8)
    return raw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--grid-only", action="store_true")
    ap.add_argument("--label", default="this build", help="names the library in the grid-alone row (e.g. 'parent commit')")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if a.grid_only:                                        # an older build of the library: bind what it has
        probe = C.CDLL(capi.LIB_PATH)
        capi.SYMBOLS[:] = [s for s in capi.SYMBOLS if hasattr(probe, s[0])]
    from xfeatslam_amd.extractor import Context
    L = capi.lib()
    lines = ["| B | call | us per call, 5 runs (min .. max) | us per frame (min) |", "|---|---|---|---|"]
    for B in (1, 64):
        ctx = Context(nfeatures=NF, max_height=32, max_width=32, max_batch=B)
        stream = torch.cuda.Stream()
        assert stream.cuda_stream != 0
        capi.check(L.xfh_set_stream(ctx.h, stream.cuda_stream), ctx.h)
        raw = records(ctx, B)
        rec = capi.DeviceBuffer(raw.nbytes).upload(raw)
        gbytes = ctx.grid_bytes(NF)
        grids = capi.DeviceBuffer(B * gbytes)

        def timed(fn):
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.iters):
                fn()
            e1.record(stream); e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / a.iters

        def row(name, ts):
            lines.append(f"| {B} | {name} | {min(ts):.1f} .. {max(ts):.1f} | {min(ts) / B:.2f} |")
            print(lines[-1], flush=True)

        raw_b = capi.GridBounds(0, 0, W, H)
        row(f"`xfh_grid_build_records_device`, {a.label}", [timed(lambda: capi.check(L.xfh_grid_build_records_device(ctx.h, rec.ptr, B, C.byref(raw_b), 0, grids.ptr), ctx.h)) for _ in range(5)])
        if not a.grid_only:
            cam = capi.Camera(*TUM1)
            bounds = capi.GridBounds(*Context.camera_bounds(cam))
            rng = np.random.RandomState(2)
            depth = rng.randint(1, 65536, (B, H, W)).astype(np.uint16); depth[rng.rand(B, H, W) < 1 / 3] = 0
            dd = capi.DeviceBuffer(depth.nbytes).upload(depth)
            side = capi.DeviceBuffer(B * NF * 16)
            xy, ur, dz = side.ptr, side.ptr + B * NF * 8, side.ptr + B * NF * 12
            scale = float(F(1) / F(5000))

            def finish(g=grids.ptr, d=dd.ptr, dt=capi.DEPTH_U16):
                capi.check(L.xfh_frame_finish_records_device(ctx.h, rec.ptr, B, C.byref(cam), d, dt, 2 * W, scale, C.byref(bounds), 0, xy, ur, dz, g), ctx.h)

            row("`xfh_frame_finish_records_device` (uint16 depth, grid)", [timed(finish) for _ in range(5)])
            row("`xfh_frame_finish_records_device` (no depth, grid)", [timed(lambda: finish(d=None, dt=capi.DEPTH_NONE)) for _ in range(5)])
            row("`xfh_frame_finish_records_device` (uint16 depth, side arrays only)", [timed(lambda: finish(g=None)) for _ in range(5)])
            # today's route, host wall clock
            kh = np.zeros(NF, capi.KP_DTYPE); kun = np.zeros(NF, capi.KP_DTYPE); dk = capi.DeviceBuffer(kun.nbytes)
            xy_h = np.zeros((NF, 2), F); un_h = np.zeros((NF, 2), F)

            def today():
                for b in range(B):
                    capi.check(L.xfh_memcpy_d2h(kh.ctypes.data, rec.ptr + b * ctx.rec_bytes + ctx.kps_off, kh.nbytes))
                    xy_h[:, 0] = kh["x"]; xy_h[:, 1] = kh["y"]
                    capi.check(L.xfh_undistort_points(C.byref(cam), xy_h.ctypes.data, NF, un_h.ctypes.data))
                    d = depth[b][kh["y"].astype(np.int64), kh["x"].astype(np.int64)].astype(F) * F(scale)
                    pos = d > 0
                    with np.errstate(all="ignore"):
                        _ur = np.where(pos, un_h[:, 0] - F(40.0) / d, F(-1))
                    kun[:] = kh; kun["x"] = un_h[:, 0]; kun["y"] = un_h[:, 1]
                    capi.check(L.xfh_memcpy_h2d(dk.ptr, kun.ctypes.data, kun.nbytes))
                    capi.check(L.xfh_grid_build_device(ctx.h, dk.ptr, NF, None, C.byref(bounds), 0, grids.ptr + b * gbytes), ctx.h)
                ctx.synchronize()

            ts = []
            for _ in range(5):
                today()
                reps = max(1, min(20, a.iters // B))
                t0 = time.perf_counter()
                for _ in range(reps):
                    today()
                ts.append((time.perf_counter() - t0) * 1e6 / reps)
            row("host route (host wall clock)", ts)
            # the two routes build the same grids
            finish(); ctx.synchronize()
            a_blob = grids.download(np.uint8, B * gbytes).copy()
            today()
            assert np.array_equal(grids.download(np.uint8, B * gbytes), a_blob)
            dd.free(); side.free(); dk.free()
        rec.free(); grids.free(); ctx.close()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
