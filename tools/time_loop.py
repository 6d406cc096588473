#!/usr/bin/env python
"""Device time of xfh_map_projection_search_device and xfh_sim3_search_device, kernel by kernel (profiles/loop_search.md).

The seeded scenes of tests/loop_rig.py (frames extracted and finished on the device) at nq = nt = 4096 and 1000, th = 4 and 15, B = 1 and
B = 8 problems (problem p: query block, pose, taken bytes and Sim3 of rig problem p mod 4, target frame resp. side 2 = frame p mod 4),
with target_shared / side1_shared off and on.  Map projection runs the Sim3 form with accept_max = 100 * 1.5.

  kernel   per launch from the library's dispatch-attached event timers (xfh_timing_enable / xfh_timing_read): the kernel's own begin ..
           end, what rocprofv3 --kernel-trace shows.  One kernel family is timed per pass, so a row takes as many passes as it has columns.
  rounds / re-searched   what k_proj_resolve leaves in the workspace header: its rounds and the queries it searched again in full, summed
           over the B problems.

There is no floor column: nothing in the parent commit does this work.

    python tools/time_loop.py [--iters 50] [--out FILE.md]
"""
import argparse
import os
import socket
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_loop as RL                                      # noqa: E402
import loop_rig as LR                                      # noqa: E402
import projection_rig as TP                                # noqa: E402
from oracle import oracle as O                             # noqa: E402
from xfeatslam_amd import capi, weights as WT              # noqa: E402
from xfeatslam_amd.extractor import Context                # noqa: E402

F = np.float32
BMAX = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = capi.lib()
    assert L.xfh_device_count() > 0, "time_loop.py needs a GPU"
    O.build()
    cam = TP.cam_struct(TP.TUM1)
    accept = float(F(RL.TH_LOW) * F(1.5))
    lines = [f"Box: {socket.gethostname()} ({L.xfh_version().decode()}).  Figures from two boxes of this pool differ by about +-2 %: compare columns of ONE run.", "",
             f"{a.iters} launches after {a.warmup} warm-up launches per figure; us per launch.", ""]
    mp = ["| nq = nt | th | B | target_shared | k_mapproj_candidates | k_proj_resolve | k_proj_count | sum | rounds | re-searched | matches |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    s3 = ["| n1 = n2 | th | B | side1_shared | k_sim3_search | k_sim3_agree | sum | agreed |", "|---|---|---|---|---|---|---|---|"]
    up = lambda x: capi.DeviceBuffer(max(np.ascontiguousarray(x).nbytes, 16)).upload(x)
    for seed, nf in ((900, 4096), (901, 1000)):
        lr = LR.LoopRig(L, WT.pack_blob(WT.make_synthetic(1234, 6.0)), nf, seed, O)
        rig, ctx = lr.rig, lr.ctx
        rb, gb = ctx.rec_bytes, ctx.grid_bytes(nf)
        recs = rig.rec.download(np.uint8, 5 * rb).reshape(5, rb); grids = rig.fin[3].download(np.uint8, 5 * gb).reshape(5, gb)
        order = [p % 4 for p in range(BMAX)]
        d_rec, d_grid = up(recs[order]), up(grids[order])
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

        # ---- map projection
        blocks = [lr.block(p) for p in order]
        cat = lambda k, t: up(np.ascontiguousarray(np.concatenate([b[k] for b in blocks]), t))
        d = [cat("xyz", F), cat("normals", F), cat("dist", F), cat("qdesc", F), cat("flags", np.uint8), up(lr.poses[order]), up(lr.Ow[order]), cat("taken", np.uint8)]
        out = capi.DeviceBuffer(Context.map_projection_search_layout(BMAX, nf, nf)["bytes"])
        ws = capi.DeviceBuffer(Context.map_projection_search_workspace_bytes(nf, nf, BMAX))
        per = Context.search_projection_workspace_bytes(nf, nf, 1)
        for th in (4.0, 15.0):
            for B in (1, BMAX):
                for shared in (0, 1):
                    fn = lambda: ctx.map_projection_search_device(RL.FORM_SIM3, B, nf, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, d[5].ptr, d[6].ptr, cam, lr.bounds, th,
                                                                  lr.sf, lr.rmax, d_grid.ptr, tg, rb, shared, nf, ws.ptr, out.ptr, d_taken=d[7].ptr, accept_max=accept)
                    t = [kernel_us(fn, k) for k in ("MAPPROJ_CANDIDATES", "PROJ_RESOLVE", "PROJ_COUNT")]
                    hdr = np.stack([ws.download(np.int32, 2, p * per) for p in range(B)])
                    lay = Context.map_projection_search_layout(B, nf, nf)
                    nm = int(out.download(np.int32, B, lay["n_matches"]).sum())
                    mp.append(f"| {nf} | {th:g} | {B} | {shared} | {t[0]:.1f} | {t[1]:.1f} | {t[2]:.1f} | {sum(t):.1f} | {int(hdr[:, 0].sum())} | {int(hdr[:, 1].sum())} | {nm} |")
                    print(mp[-1], flush=True)
        for x in d + [out, ws]:
            x.free()
        # ---- SearchBySim3
        types = dict(points=F, dist=F, mp_desc=F, flags=np.uint8)
        d1 = {k: up(np.ascontiguousarray(np.concatenate([lr.s1[p][k] for p in order]), types[k])) for k in LR.SIDE_IN}
        d2 = {k: up(np.ascontiguousarray(np.concatenate([lr.s2[p][k] for p in order]), types[k])) for k in LR.SIDE_IN}
        dT1, dT2 = up(np.stack([lr.pairs[p][0] for p in order])), up(np.stack([lr.pairs[p][1] for p in order]))
        dM21, dM12 = up(np.stack([lr.pairs[p][2] for p in order])), up(np.stack([lr.pairs[p][3] for p in order]))
        g1 = up(np.tile(grids[0], BMAX))
        lay = Context.sim3_search_layout(BMAX, nf, nf)
        out = capi.DeviceBuffer(lay["bytes"])
        for th in (4.0, 15.0):
            for B in (1, BMAX):
                for shared in (0, 1):
                    lay = Context.sim3_search_layout(B, nf, nf)
                    side1 = Context.sim3_side(nf, g1.ptr, rig.rec.ptr + ctx.desc_off, 0, d1["points"].ptr, d1["dist"].ptr, d1["mp_desc"].ptr, d1["flags"].ptr, dT1.ptr, out.ptr, lay, "1")
                    side2 = Context.sim3_side(nf, d_grid.ptr, tg, rb, d2["points"].ptr, d2["dist"].ptr, d2["mp_desc"].ptr, d2["flags"].ptr, dT2.ptr, out.ptr, lay, "2")
                    fn = lambda: ctx.sim3_search_device(B, shared, side1, side2, dM21.ptr, dM12.ptr, cam, lr.bounds, th, lr.sf, lr.rmax, out.ptr + lay["match12"],
                                                        out.ptr + lay["n_found"])
                    t = [kernel_us(fn, k) for k in ("SIM3_SEARCH", "SIM3_AGREE")]
                    nfo = int(out.download(np.int32, B, lay["n_found"]).sum())
                    s3.append(f"| {nf} | {th:g} | {B} | {shared} | {t[0]:.1f} | {t[1]:.1f} | {sum(t):.1f} | {nfo} |")
                    print(s3[-1], flush=True)
        for x in list(d1.values()) + list(d2.values()) + [dT1, dT2, dM21, dM12, g1, out, d_rec, d_grid]:
            x.free()
        lr.close()
    text = "\n".join(lines + ["## xfh_map_projection_search_device (the Sim3 form)", ""] + mp + ["", "## xfh_sim3_search_device", ""] + s3) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
