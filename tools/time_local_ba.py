#!/usr/bin/env python
"""Device time of xfh_local_ba_device (the fixed schedule of lba.hip.h) -> profiles/local_ba.md: us per kernel family and per call at (free, fixed, points,
observations per point) = (8, 8, 500, 4), (32, 32, 4000, 6) and (128, 64, 8000, 8), the cost of the all-idle schedule and the share of the call spent in the
factorisation.

  kernel     us per call in each kernel family, from the library's dispatch-attached event timers (xfh_timing_enable / xfh_timing_read): the sum over the
             family's launches of one call, idle ones included
  per call   host clock around `iters` calls that end in one synchronise, over iters
  all-idle   the same shape with no edge at a fixed keyframe: the plan finds status ABORTED and every kernel of the 530 scheduled ones returns at once

These are records, not thresholds.  There is no parent-commit baseline (the call is new).  The host code it replaces -- the reference's g2o -- cannot be
built and timed here, so no ratio against it is measured or claimed.

    python tools/time_local_ba.py [--iters 5] [--out FILE.md]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import local_ba_rig as G                                    # noqa: E402
from xfeatslam_amd import capi, local_ba                    # noqa: E402

SHAPES = ((8, 8, 500, 4), (32, 32, 4000, 6), (128, 64, 8000, 8))
FAMILIES = ("LBA_PLAN", "LBA_LINEARIZE", "LBA_POINT_BUILD", "LBA_BEGIN", "LBA_SCHUR", "LBA_SOLVE", "LBA_UPDATE", "LBA_EVALUATE", "LBA_DECIDE", "LBA_FINISH")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_ba.md"))
    a = ap.parse_args()
    L = capi.lib()
    assert L.xfh_device_count() > 0, "time_local_ba.py needs a GPU"
    rig = G.LbaRig(L)
    ctx = rig.ctx
    lines = ["# xfh_local_ba_device: LocalBundleAdjustment behind the triangulate -> fuse chain", "",
             "Written by `tools/time_local_ba.py`.  A fixed schedule of 4 + 53 x 10 + 2 = 536 launches around a control block (`lba.hip.h`); registers (clang 22 / ROCm 7.2, "
             "`-Rpass-analysis=kernel-resource-usage`): `k_lba_schur` 246 VGPRs, `k_lba_linearize<true>` 188, `k_lba_update` 82, every other kernel below 50; no kernel of "
             "`kernels_lba.hip` uses scratch or AGPRs.  The reference's g2o cannot be built and timed here: no ratio against it is measured or claimed.", "",
             f"One MI355X ({L.xfh_version().decode()}); nothing else of this process on the GPU.  {a.iters} calls per figure after 2 warm-up calls, back to back on one stream, "
             "mixed mono / stereo edges, 5 % gross outliers, write_back off.", "",
             "| free, fixed, points, obs/point | edges | header: iterations, trials, rejected, failures, erase | per call (host clock), us | all-idle schedule (ABORTED), us | "
             + " | ".join("`k_%s`" % f.lower() for f in FAMILIES) + " | factorisation share of the kernel time |", "|" + "---|" * (6 + len(FAMILIES))]
    for n_free, n_fixed, nP, per in SHAPES:
        p = G.make(7000 + n_free, n_free, n_fixed, nP, per, "mixed", outliers=0.05, init_fixed=False)
        idle = dict(p, edge_kf=p["edge_kf"].copy())
        G._no_fixed_edge(idle, None)
        row = []
        for prob in (p, idle):
            nK, nP_, nE = G.dims(prob)
            arrays = [np.ascontiguousarray(np.asarray(prob[k], dt)) for k, dt in G.INPUTS]
            dev = [capi.DeviceBuffer(x.nbytes).upload(x) for x in arrays]
            lay = local_ba.local_ba_layout(nK, nP_, nE)
            out, ws = capi.DeviceBuffer(lay["bytes"]), capi.DeviceBuffer(local_ba.workspace_bytes(nK, nP_, nE, n_free))
            cam = G.cam_struct()

            def call():
                local_ba.local_ba_device(ctx, nK, n_free, nP_, nE, dev[0].ptr, len(arrays[0]), dev[1].ptr, len(arrays[1]), *[d.ptr for d in dev[2:]], cam, ws.ptr, out.ptr, lay)
            for _ in range(2):
                call()
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                call()
            ctx.synchronize()
            wall = (time.perf_counter() - t0) * 1e6 / a.iters
            hdr = lay.parse(out.download(np.uint8, lay["bytes"]))["header"]
            fam = {}
            if prob is p:
                for f in FAMILIES:
                    ctx.timing_enable(capi.K[f])
                    for _ in range(a.iters):
                        call()
                    ctx.synchronize()
                    cnt, ms = ctx.timing_read()
                    ctx.timing_enable(capi.K["NONE"])
                    fam[f] = (ms * 1e3 / a.iters, cnt // a.iters)
            for d in dev + [out, ws]:
                d.free()
            row.append((wall, hdr, fam, nE))
        (wall, hdr, fam, nE), (wall_idle, hdr_idle, _, _) = row
        assert hdr[0] == 0 and hdr_idle[0] == 1, (hdr, hdr_idle)
        total = sum(v[0] for v in fam.values())
        lines.append(f"| {n_free}, {n_fixed}, {nP}, {per} | {nE} | {hdr[5]}, {hdr[6]}, {hdr[7]}, {hdr[8]}, {hdr[9]} | {wall:.0f} | {wall_idle:.0f} | "
                     + " | ".join(f"{fam[f][0]:.0f} ({fam[f][1]})" for f in FAMILIES) + f" | {fam['LBA_SOLVE'][0] / total:.2f} |")
        print(lines[-1], flush=True)
    lines += ["", "Kernel columns: us per call summed over the family's launches (their number per call in brackets), idle launches included; `k_lba_evaluate` is "
              "`k_lba_linearize<false>`, `k_lba_finish` includes `k_lba_header`.  The all-idle column is what the 530 scheduled launches of the Levenberg loop cost when none of "
              "them has work (plus the plan and the finish): the price of a schedule that needs no read-back.  A call whose optimisation ends after k iterations pays the idle "
              "price for the remaining launches.", ""]
    rig.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
