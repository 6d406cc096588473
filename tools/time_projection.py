#!/usr/bin/env python
"""Device time of xfh_search_projection_device against what the library offered before it (profiles/search_projection.md).

  (a) xfh_search_window_device on the pre-projected (u, v, r): the baseline -- no claim order, the caller projects
  (b) xfh_search_projection_device, XFH_PROJ_POINTS, all claim bits clear
  (c) the same with the scene's claim bits (about half set)
  (d) the same, B = 8 problems (eight poses, the four current frames twice) in one call

nq = nt = 4096, radius 15, the seeded scene of tests/projection_rig.py (frames extracted and finished on the device).  Per leg:
a warm-up, then --iters back-to-back calls between two waits for the stream (HOST wall time per call by perf_counter: it holds the
ctypes and launch overhead of the calls as well as the device's work -- what a Python caller's loop sees, not device time), then
the same number of calls once per kernel with the library's dispatch-attached event timers (xfh_timing_enable / xfh_timing_read):
the kernels' own begin .. end.  The rounds k_proj_resolve took and the queries it searched a second time come from the
workspace header.  The A / B split under the profiler: rocprofv3 --kernel-trace --stats -- python tools/time_projection.py --iters 50

    python tools/time_projection.py [--iters 200] [--out FILE.md]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_projection as RP                                # noqa: E402
import projection_rig as TP                                # noqa: E402
from xfeatslam_amd import capi, weights as WT              # noqa: E402
from xfeatslam_amd.extractor import Context                # noqa: E402

F = np.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = capi.lib()
    assert L.xfh_device_count() > 0, "time_projection.py needs a GPU"
    nf, r, BB = 4096, 15.0, 8
    rig = TP.Rig(L, WT.pack_blob(WT.make_synthetic(1234, 6.0)), nf, 900)
    ctx, cam = rig.ctx, TP.cam_struct(TP.TUM1)
    rb, gb = ctx.rec_bytes, ctx.grid_bytes(nf)
    # eight problems: the records, grids and uright of the current frames 1 .. 4, twice
    recs = rig.rec.download(np.uint8, 5 * rb).reshape(5, rb); grids = rig.fin[3].download(np.uint8, 5 * gb).reshape(5, gb)
    order = [1, 2, 3, 4, 1, 2, 3, 4]
    up = lambda x: capi.DeviceBuffer(max(np.ascontiguousarray(x).nbytes, 16)).upload(x)
    d_rec, d_grid, d_ur = up(recs[order]), up(grids[order]), up(rig.ur[order])
    poses = np.stack([RP.pose(900 + p, TP.SHIFTS[p % 4], cam=TP.TUM1) for p in range(BB)])
    d_T, d_pts, d_q = up(poses), up(np.tile(rig.xyz, (BB, 1))), up(np.tile(rig.recs[0][1], (BB, 1)))
    fl_half = np.tile(rig.flags, BB); fl_clear = (fl_half & 1).astype(np.uint8)
    d_fl = {"clear": up(fl_clear), "half": up(fl_half)}
    u, v, ur, st = RP.project(poses[0], TP.TUM1, rig.bounds, rig.xyz)
    d_uvr, d_urq = up(np.stack([u, v, np.full(nf, r, F)], 1).astype(F)), up(ur)
    lay = Context.search_projection_layout(BB, nf, nf)
    out = capi.DeviceBuffer(lay["bytes"]); ws = capi.DeviceBuffer(Context.search_projection_workspace_bytes(nf, nf, BB))
    wout = capi.DeviceBuffer(20 * nf)
    tg = d_rec.ptr + ctx.desc_off

    def window():
        ctx.search_window_device(d_q.ptr, d_uvr.ptr, nf, d_grid.ptr, tg, nf, wout.ptr, 1 << 30, d_uright=d_ur.ptr, d_ur_query=d_urq.ptr)

    def proj(B, flags):
        return lambda: ctx.search_projection_device(capi.PROJ_POINTS, B, nf, d_pts.ptr, d_q.ptr, d_fl[flags].ptr, d_grid.ptr, tg, rb, nf, ws.ptr, out.ptr, radius=r,
                                                    d_Tcw=d_T.ptr, cam=cam, bounds=rig.bounds, d_uright=d_ur.ptr, init_dist=1 << 30, th_high=1000)

    def wall(fn):
        for _ in range(a.warmup):
            fn()
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e6 / a.iters

    def kernel_us(fn, name):
        ctx.timing_enable(capi.K[name])
        for _ in range(a.iters):
            fn()
        ctx.synchronize()
        n, ms = ctx.timing_read()
        ctx.timing_enable(capi.K["NONE"])
        return ms * 1e3 / max(n, 1) if n else 0.0

    legs = [("(a) xfh_search_window_device on pre-projected uvr", window, 1, ("SEARCH_WINDOW",)),
            ("(b) xfh_search_projection_device, claim bits clear", proj(1, "clear"), 1, ("PROJ_CANDIDATES", "PROJ_RESOLVE", "PROJ_COUNT")),
            ("(c) xfh_search_projection_device, half the claim bits set", proj(1, "half"), 1, ("PROJ_CANDIDATES", "PROJ_RESOLVE", "PROJ_COUNT")),
            ("(d) xfh_search_projection_device, B = 8, half the claim bits set", proj(BB, "half"), BB, ("PROJ_CANDIDATES", "PROJ_RESOLVE", "PROJ_COUNT"))]
    lines = [f"nq = nt = {nf}, radius {r:g}, {a.iters} back-to-back calls after {a.warmup} warm-up calls; visible queries {(np.where(rig.flags & 1, st, 0) == RP.VISIBLE).sum()}", "",
             "| leg | host wall us per call (perf_counter, launch overhead included), 3 runs | kernels, device us per launch (event timers) | sum of the kernels | rounds of k_proj_resolve per problem | queries searched a second time |", "|---|---|---|---|---|---|"]
    for name, fn, B, kernels in legs:
        walls = [wall(fn) for _ in range(3)]
        kus = [kernel_us(fn, k) for k in kernels]
        ks = ", ".join(f"{L.xfh_kernel_name(capi.K[k]).decode()} {t:.1f}" for k, t in zip(kernels, kus))
        rounds = redo = "-"
        if B and kernels[0] != "SEARCH_WINDOW":
            hdr = np.stack([ws.download(np.int32, 2, p * (ws.nbytes // BB)) for p in range(B)])
            rounds, redo = " ".join(str(x) for x in hdr[:, 0]), " ".join(str(x) for x in hdr[:, 1])
        lines.append(f"| {name} | {' / '.join(f'{w:.1f}' for w in walls)} | {ks} | {sum(kus):.1f} | {rounds} | {redo} |")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    print(text)
    for x in (d_rec, d_grid, d_ur, d_T, d_pts, d_q, d_uvr, d_urq, out, ws, wout) + tuple(d_fl.values()):
        x.free()
    rig.close()


if __name__ == "__main__":
    main()
