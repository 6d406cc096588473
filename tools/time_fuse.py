#!/usr/bin/env python
"""Device time of xfh_fuse_search_device (k_fuse_search) beside a floor (profiles/fuse_search.md).

nq = nt = 4096, the seeded scene of tests/fuse_rig.py (frames extracted and finished on the device), th = 3 and 7, the SE3 form
(chi-square gates on, init_dist 256), B = 1, 8 and 24 keyframes with query_problem_stride = 0 (LocalMapping::SearchInNeighbors: one
block of map points against every neighbour; the five frames of the rig in turn, each with its own pose).

  kernel   k_fuse_search per launch from the library's dispatch-attached event timers (xfh_timing_enable / xfh_timing_read): the
           kernel's own begin .. end, what rocprofv3 --kernel-trace shows
  floor    xfh_search_window_device (k_search_window) on the same (u, v, r) for the queries that REACH the search, one launch per
           keyframe, summed.  It does strictly less per query -- no projection, no culls, no chi-square gate, and the culled queries
           are not even in its grid of waves -- but it keeps a second best.  k_search_window's machine code is the parent
           commit's, instruction for instruction (the hook that gained two arguments is inlined away), so this build's figure is the parent's.

    python tools/time_fuse.py [--iters 200] [--out FILE.md]
"""
import argparse
import os
import socket
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_fuse as RU                                      # noqa: E402
import ref_projection as RP                                # noqa: E402
import fuse_rig as FR                                      # noqa: E402
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
    assert L.xfh_device_count() > 0, "time_fuse.py needs a GPU"
    nf, BMAX = 4096, 24
    fr = FR.FuseRig(L, WT.pack_blob(WT.make_synthetic(1234, 6.0)), nf, 900)
    rig, ctx, cam = fr.rig, fr.ctx, TP.cam_struct(TP.TUM1)
    rb, gb = ctx.rec_bytes, ctx.grid_bytes(nf)
    recs = rig.rec.download(np.uint8, 5 * rb).reshape(5, rb); grids = rig.fin[3].download(np.uint8, 5 * gb).reshape(5, gb)
    order = [p % 5 for p in range(BMAX)]
    shifts = [(0, 0)] + list(TP.SHIFTS)
    up = lambda x: capi.DeviceBuffer(max(np.ascontiguousarray(x).nbytes, 16)).upload(x)
    d_rec, d_grid, d_ur = up(recs[order]), up(grids[order]), up(rig.ur[order])
    poses = np.stack([RP.pose(900 + p, shifts[p % 5], cam=TP.TUM1) for p in range(BMAX)])
    Ow = np.stack([RU.camera_centre(T) for T in poses])
    d_T, d_O = up(poses), up(Ow)
    d_in = [up(x) for x in (fr.xyz, fr.normals, fr.dist, fr.qdesc, fr.flags)]
    out = capi.DeviceBuffer(Context.fuse_search_layout(BMAX, nf)["bytes"])
    wout = capi.DeviceBuffer(20 * nf)
    tg = d_rec.ptr + ctx.desc_off

    def kernel_us(fn, name):
        for _ in range(a.warmup):
            fn()
        ctx.synchronize()
        ctx.timing_enable(capi.K[name])
        for _ in range(a.iters):
            fn()
        ctx.synchronize()
        n, ms = ctx.timing_read()
        ctx.timing_enable(capi.K["NONE"])
        return ms * 1e3 / max(n, 1) if n else 0.0

    lines = [f"Box: {socket.gethostname()} ({L.xfh_version().decode()}).  Figures from two boxes of this pool differ by about +-2 %: compare columns of ONE run.", "",
             f"nq = nt = {nf}, SE3 form (chi-square gates, init_dist 256), query_problem_stride = 0, {a.iters} launches after {a.warmup} warm-up launches.", "",
             "| th | B | queries that reach the search (all problems) | fused | k_fuse_search, us per launch | floor: k_search_window on those queries, us (sum of B launches) | ratio |", "|---|---|---|---|---|---|---|"]
    for th in (3.0, 7.0):
        floor, reach, fused = [], [], []
        for p in range(BMAX):                                        # per keyframe: the (u, v, r) of the queries that reach the search, and the floor
            u, v, ur, r, lv, st = RU.project(poses[p], Ow[p], TP.TUM1, fr.bounds, th, FR.SF, FR.NL, fr.xyz, fr.normals, fr.dist)
            m = ((fr.flags & 1) != 0) & (st == RU.VISIBLE)
            uvr = np.stack([u[m], v[m], r[m]], 1).astype(F)
            d_uvr, d_q = up(uvr), up(fr.qdesc[m])
            nqv = int(m.sum())
            fn = lambda: ctx.search_window_device(d_q.ptr, d_uvr.ptr, nqv, d_grid.ptr + p * gb, tg + p * rb, nf, wout.ptr, 256)
            floor.append(kernel_us(fn, "SEARCH_WINDOW")); reach.append(nqv)
            d_uvr.free(); d_q.free()
        for B in (1, 8, 24):
            fn = lambda: ctx.fuse_search_device(B, nf, 0, d_in[0].ptr, d_in[1].ptr, d_in[2].ptr, d_in[3].ptr, d_in[4].ptr, d_T.ptr, d_O.ptr, cam, fr.bounds, th, fr.sf, fr.rmax,
                                                d_grid.ptr, tg, rb, nf, out.ptr, d_uright=d_ur.ptr, chi2=True, init_dist=256)
            t = kernel_us(fn, "FUSE_SEARCH")
            lay = Context.fuse_search_layout(B, nf)
            nfu = int(out.download(np.int32, B, lay["n_fused"]).sum())
            lines.append(f"| {th:g} | {B} | {sum(reach[:B])} | {nfu} | {t:.1f} | {sum(floor[:B]):.1f} | {t / max(sum(floor[:B]), 1e-9):.2f} |")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    print(text)
    for x in [d_rec, d_grid, d_ur, d_T, d_O, out, wout] + d_in:
        x.free()
    fr.close()


if __name__ == "__main__":
    main()
