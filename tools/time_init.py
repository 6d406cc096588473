#!/usr/bin/env python
"""Device time of xfh_init_search_device, kernel by kernel, next to xfh_search_window_device on the same windows (profiles/init_search.md).

The seeded scenes of tests/init_rig.py (two frames extracted and finished on the device, the planted correspondences and structures) at
nq = nt = 4096 and 1000, window = 100 and 10, B = 1 and B = 4 problems (problem p: the scene's queries rotated by p * 37 places).

  kernel   per launch from the library's dispatch-attached event timers (xfh_timing_enable / xfh_timing_read): the kernel's own begin ..
           end, what rocprofv3 --kernel-trace shows.  One kernel family is timed per pass, so a row takes as many passes as it has columns.
  rounds / re-searched / ran out   what k_init_resolve leaves in the workspace header: its rounds, the queries it searched again in full and
           the lists that ran out (summed over the rounds), each summed over the B problems.
  k_search_window   xfh_search_window_device with the same queries, centres and radius: the cost of the walk without any resolution.

The list length K is a build constant (XFH_INIT_K); the table of another K comes from running this tool on a library built with it:
    make -C xfeatslam_amd/csrc init_k K=4 && XFEAT_HIP_LIB=tools/ab/init_k4.so python tools/time_init.py

    python tools/time_init.py [--iters 30] [--out FILE.md]
"""
import argparse
import os
import socket
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import init_rig as IR                                      # noqa: E402
from oracle import oracle as O                             # noqa: E402
from xfeatslam_amd import capi, weights as WT              # noqa: E402
from xfeatslam_amd.extractor import Context                # noqa: E402

F = np.float32
BMAX = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = capi.lib()
    assert L.xfh_device_count() > 0, "time_init.py needs a GPU"
    O.build()
    K = int(L.xfh_init_list_entries())
    lines = [f"Box: {socket.gethostname()} ({L.xfh_version().decode()}), K = {K}.  Figures from two boxes of this pool differ by about +-2 %: compare columns of ONE run.", "",
             f"{a.iters} launches after {a.warmup} warm-up launches per figure; us per launch.", "",
             "| nq = nt | window | B | K | k_init_candidates | k_init_resolve | k_init_final | sum | k_search_window (B times) | rounds | re-searched | ran out | matches | mean window |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    up = lambda x: capi.DeviceBuffer(max(np.ascontiguousarray(x).nbytes, 16)).upload(x)
    for seed, nf in ((1201, 4096), (1200, 1000)):
        rig = IR.InitRig(L, WT.pack_blob(WT.make_synthetic(1234, 6.0)), nf, seed, O)
        ctx = rig.ctx

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

        blocks = [rig.block(p) for p in range(BMAX)]
        dq = up(np.concatenate([b[0] for b in blocks])); dpm = up(np.concatenate([b[1] for b in blocks]))
        g = rig.fin[3].download(np.uint8, ctx.grid_bytes(nf), ctx.grid_bytes(nf))
        dg = up(np.tile(g, BMAX)); dxy = up(np.tile(rig.xy[1].reshape(-1), BMAX))
        out = capi.DeviceBuffer(Context.init_search_layout(BMAX, nf, nf)["bytes"])
        ws = capi.DeviceBuffer(Context.init_search_workspace_bytes(nf, nf, BMAX))
        per = Context.init_search_workspace_bytes(nf, nf, 1)
        swo = capi.DeviceBuffer(5 * nf * 4 + 1024)
        for window in (100.0, 10.0):
            uvr = up(np.concatenate([rig.pm, np.full((nf, 1), window, F)], 1).astype(F))
            sw = lambda: ctx.search_window_device(dq.ptr, uvr.ptr, nf, rig.dgrid, rig.dtg.ptr, nf, swo.ptr, init_dist=0x7fffffff)
            t_sw = kernel_us(sw, "SEARCH_WINDOW")
            for B in (1, BMAX):
                fn = lambda: ctx.init_search_device(B, nf, dq.ptr, dpm.ptr, dg.ptr, rig.dtg.ptr, 0, nf, ws.ptr, out.ptr, window=window, d_target_xy=dxy.ptr)
                t = [kernel_us(fn, k) for k in ("INIT_CANDIDATES", "INIT_RESOLVE", "INIT_FINAL")]
                hdr = np.stack([ws.download(np.int32, 4, p * per) for p in range(B)])
                lay = Context.init_search_layout(B, nf, nf)
                nm = int(out.download(np.int32, B, lay["n_matches"]).sum())
                nw = float(out.download(np.int32, B * nf, lay["n_window"]).mean())
                lines.append(f"| {nf} | {window:g} | {B} | {K} | {t[0]:.1f} | {t[1]:.1f} | {t[2]:.1f} | {sum(t):.1f} | {B * t_sw:.1f} | {int(hdr[:, 0].sum())} | "
                             f"{int(hdr[:, 1].sum())} | {int(hdr[:, 2].sum())} | {nm} | {nw:.0f} |")
                print(lines[-1], flush=True)
            uvr.free()
        for x in (dq, dpm, dg, dxy, out, ws, swo):
            x.free()
        rig.close()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
