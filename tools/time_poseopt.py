#!/usr/bin/env python
"""Device time of xfh_pose_optimize_device (k_pose_optimize) -> profiles/pose_optimization.md, and the discrepancies between the device and the
float64 restatement on the scenes of tests/poseopt_rig.py.

Scenes of tests/poseopt_rig.py's generator: 100, 500 and 2000 edges (nt = 4 x edges keypoint slots, half of the edges stereo), 0 % and 20 % gross
outliers, B = 1 and 8 (the same problem B times: one workgroup each).

  kernel     us per launch from the library's dispatch-attached event timers (xfh_timing_enable / xfh_timing_read): the kernel's own begin .. end
  per call   host clock around `iters` calls that end in one synchronise, over iters
  rounds, iterations, trials: the header the call writes

There is no parent-commit baseline (the call is new) and no threshold.  Host g2o was NOT timed: Eigen is not available where this runs, so no
comparison with the reference's own optimiser is made or claimed.

    python tools/time_poseopt.py [--iters 50] [--out FILE.md]
"""
import argparse
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import poseopt_rig as R                                     # noqa: E402
import ref_poseopt as RP                                    # noqa: E402
from xfeatslam_amd import capi                              # noqa: E402

F = np.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = capi.lib()
    assert L.xfh_device_count() > 0, "time_poseopt.py needs a GPU"
    rig = R.PoseRig(L)
    ctx = rig.ctx
    lines = [f"Box: {socket.gethostname()} ({L.xfh_version().decode()}); nothing else of this process on the GPU.", "",
             f"{a.iters} calls after {a.warmup} warm-up calls, back to back on one stream.", "",
             "| edges | nt | outliers | B | k_pose_optimize, us per launch | per call (host clock), us | us per problem | rounds | iterations | trials | rejected | n_bad |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    up = lambda x: capi.DeviceBuffer(x.nbytes + 16).upload(x)
    for n in (100, 500, 2000):
        for outl in (0.0, 0.2):
            s = R.make(seed=4000 + n, n_edges=n, nt=4 * n, kind="mixed", outliers=outl)
            nt, nq = s["nt"], s["nq"]
            for B in (1, 8):
                ins = [up(np.tile(np.ascontiguousarray(s[k]).reshape(1, -1), (B, 1))) for k in ("Tcw", "xy_un", "uright", "assigned", "points")]
                lay = ctx.pose_optimize_layout(B, nt)
                out = capi.DeviceBuffer(lay["bytes"])
                ws = capi.DeviceBuffer(ctx.pose_optimize_workspace_bytes(nt, B))

                def call():
                    ctx.pose_optimize_device(B, nt, nq, ins[0].ptr, rig.cam, ins[1].ptr, ins[2].ptr, ins[3].ptr, ins[4].ptr, ws.ptr, *[out.ptr + lay[k] for k in lay.names],
                                             R.INV_SIGMA2)

                for _ in range(a.warmup):
                    call()
                ctx.synchronize()
                ctx.timing_enable(capi.K["POSE_OPTIMIZE"])
                for _ in range(a.iters):
                    call()
                ctx.synchronize()
                cnt, ms = ctx.timing_read()
                ctx.timing_enable(capi.K["NONE"])
                kus = ms * 1e3 / max(cnt, 1)
                t0 = time.perf_counter()
                for _ in range(a.iters):
                    call()
                ctx.synchronize()
                wall = (time.perf_counter() - t0) * 1e6 / a.iters
                h = out.download(np.int32, 8, lay["header"])
                lines.append(f"| {n} | {nt} | {int(outl * 100)} % | {B} | {kus:.1f} | {wall:.1f} | {kus / B:.1f} | {h[3]} | {h[4]} | {h[5]} | {h[6]} | {h[1]} |")
                print(lines[-1], flush=True)
                for x in ins + [out, ws]:
                    x.free()
    lines += ["", "Device against the float64 restatement (the kernel's rule of tests/ref_poseopt.py) on the rig's scenes: flags and header equal or not, the largest",
              "difference of pose and classification chi2 in float32 steps, final_chi2 of both and their relative difference (a difference in doubles).", "",
              "| scene | header | flags and header equal | pose, float steps | chi2, float steps | final_chi2 device | final_chi2 restatement | relative difference |",
              "|---|---|---|---|---|---|---|---|"]
    worst = 0.0
    for name in R.SCENES:
        s = R.scene(name)
        res, _ = rig.run([s])
        m = R.model(s)
        r = res[0]
        rel = abs(r["final_chi2"] - m["final_chi2"]) / max(abs(m["final_chi2"]), 1e-300)
        worst = max(worst, rel)
        eq = np.array_equal(r["header"], m["header"]) and np.array_equal(r["outlier"], m["outlier"])
        lines.append(f"| {name} | {r['header'].tolist()} | {eq} | {int(RP.ulps(r['Tcw_out'], m['Tcw_out']).max())} | {int(RP.ulps(r['chi2'], m['chi2']).max())} | "
                     f"{r['final_chi2']:.17g} | {m['final_chi2']:.17g} | {rel:.1e} |")
        print(lines[-1], flush=True)
    lines += ["", f"Largest relative double discrepancy seen: {worst:.1e}."]
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    print(text)
    rig.close()


if __name__ == "__main__":
    main()
