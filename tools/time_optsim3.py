#!/usr/bin/env python
"""Device time of xfh_sim3_optimize_device (k_sim3_optimize, one launch) -> profiles/optimize_sim3.md, with the measured distance of the device
from the rule of tests/ref_optsim3.py alongside, and the spread of the float64 forms among themselves from which SIM3OPT_TOL is taken.

Scenes at loop-closing shapes: n1 = 4096 keypoint slots (the workspace instance of the kernel) of which about 30, 100 and 500 carry a
correspondence, 20 % of them gross outliers, B = 1 and 3 candidates.

  kernel     us per launch from the library's dispatch-attached event timers (xfh_timing_enable / xfh_timing_read)
  per call   host clock around `iters` calls that end in one synchronise, over iters

Without --gpu only the CPU part runs (the spread of the forms), and the file says that the kernel times are unmeasured.  There is no parent-commit
baseline (the call is new) and no threshold.  The host code it replaces -- the reference's g2o optimiser -- was NOT timed, so no speed-up over the
reference is measured or claimed.

    python tools/time_optsim3.py [--gpu] [--iters 200] [--out FILE.md]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import optsim3_rig as G                                     # noqa: E402
import ref_optsim3 as R                                     # noqa: E402
from xfeatslam_amd import capi                              # noqa: E402

SHAPES = ((1, 30), (1, 100), (1, 500), (3, 30), (3, 100), (3, 500))


def problems(B, pairs, n1=4096):
    out = pairs // 5
    return G.batch([G.make(seed=9000 + 10 * pairs + b, n_pairs=pairs - out, n1=n1, outliers=out) for b in range(B)])


def gpu_part(a, lines):
    L = capi.lib()
    assert L.xfh_device_count() > 0, "time_optsim3.py --gpu needs a GPU"
    rig = G.Sim3OptRig(L)
    ctx = rig.ctx
    lines += [f"One MI355X ({L.xfh_version().decode()}); nothing else of this process on the GPU.", "",
              f"{a.repeats} repeats of {a.iters} calls after {a.warmup} warm-up calls, back to back on one stream; n1 = 4096 keypoint slots, 20 % gross outliers.", "",
              "| B | pairs | problem 0: n_corr, n_bad, return, iterations, trials | passes of the slowest problem | k_sim3_optimize, us per launch: median (min .. max) | "
              "per call (host clock), us: median (min .. max) | device to rule: "
              + ", ".join(R.Tol._fields) + " | decisions equal to the rule's |", "|---|---|---|---|---|---|---|---|"]
    for B, pairs in SHAPES:
        ps = problems(B, pairs)
        (n1, M1, nq, n2), arrays, s12, tmw = G._inputs(ps, False)
        dev = [capi.DeviceBuffer(x.nbytes).upload(x) for x in arrays + [s12, tmw]]
        ws = capi.DeviceBuffer(int(L.xfh_sim3_optimize_workspace_bytes(n1, B)))
        lay = ctx.sim3_optimize_layout(B, n1)
        out = capi.DeviceBuffer(lay["bytes"])
        outs = [out.ptr + lay[k] for k in lay.names]
        cam = G.cam_struct()

        def call():
            ctx.sim3_optimize_device(B, n1, M1, nq, n2, False, [d.ptr for d in dev[:4]], [d.ptr for d in dev[4:10]], dev[10].ptr, 13, dev[11].ptr, cam, cam, ws.ptr,
                                     outs[0], outs[1], outs[2], outs[3], outs[4], 13, outs[5], outs[6], outs[7], outs[8], th2=G.TH2)
        for _ in range(a.warmup):
            call()
        ctx.synchronize()
        kus, walls = [], []
        for _ in range(a.repeats):                                          # the same command on the same code, a.repeats times: the spread
            ctx.timing_enable(capi.K["SIM3_OPTIMIZE"])
            for _ in range(a.iters):
                call()
            ctx.synchronize()
            cnt, ms = ctx.timing_read()
            ctx.timing_enable(capi.K["NONE"])
            kus.append(ms * 1e3 / max(cnt, 1))
            t0 = time.perf_counter()
            for _ in range(a.iters):
                call()
            ctx.synchronize()
            walls.append((time.perf_counter() - t0) * 1e6 / a.iters)
        for d in dev + [ws, out]:
            d.free()
        res, _ = rig.run(ps)
        worst, equal = dict.fromkeys(R.Tol._fields, 0.0), True
        for r, p in zip(res, ps):
            ref = R.rule(p)
            equal = equal and R.same_decisions(r, ref) == []
            for k, v in R.distances(r, ref, G.TH2).items():
                worst[k] = max(worst[k], v)
        h = res[0]["header"]
        passes = max(int(r["header"][8]) + int(r["header"][9]) + int(r["header"][7]) for r in res)
        span = lambda v: f"{sorted(v)[len(v) // 2]:.1f} ({min(v):.1f} .. {max(v):.1f})"
        lines.append(f"| {B} | {pairs} | {int(h[0])}, {int(h[3])}, {int(h[6])}, {int(h[8])}, {int(h[9])} | {passes} | {span(kus)} | {span(walls)} | "
                     + ", ".join(f"{worst[k]:.3g}" for k in R.Tol._fields) + f" | {'yes' if equal else 'NO'} |")
        print(lines[-1], flush=True)
    lines += ["", "Decisions: pair status, assigned_out and header[0:8].  The distances are in the units of SIM3OPT_TOL (below).", "",
              "The time of a launch is the time of its slowest workgroup, and a workgroup's time goes with its number of passes (iterations + trials + "
              "classifications: a BUILD pass costs 30 edge evaluations per pair, a TRIAL pass 2), which the data decide, not with B or the pair count alone: "
              "that is why the rows are not monotone in the pair count.", ""]
    rig.close()


def cpu_part(lines):
    lines += ["## The spread of the float64 forms among themselves", "",
              "The literal transcription, the kernel's rule, the rule with exp / sin / cos / sqrt moved by one double step under three seeds and the library's host form, on the rig's scenes "
              "and on 200 random small scenes (tests/test_optsim3_forms.py::test_spread_of_the_reference); nothing from the device is in this table.  "
              "SIM3OPT_TOL is twice the largest value, not below 1 float step and 1e-13.", "",
              "| output | unit | largest spread | where | SIM3OPT_TOL |", "|---|---|---|---|---|"]
    units = dict(state="relative to the largest entry", s12="float32 steps at the block's magnitude", tcw="float32 steps at the block's magnitude",
                 ow="float32 steps at the block's magnitude", chi2="float32 steps at max(chi2, th2)", final="relative to max(final_chi2, th2)")
    worst, where = dict.fromkeys(R.Tol._fields, 0.0), dict.fromkeys(R.Tol._fields, None)
    for name in list(G.SCENES) + list(range(200)):
        for k, v in G.spread(G.forms_of(name) + [G.host_of(name)]).items():
            if v > worst[k]:
                worst[k], where[k] = v, name
    for k in R.Tol._fields:
        lines.append(f"| {k} | {units[k]} | {worst[k]:.4g} | {where[k]} | {getattr(G.SIM3OPT_TOL, k):g} |")
    lines += [""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimize_sim3.md"))
    a = ap.parse_args()
    lines = ["# xfh_sim3_optimize_device: OptimizeSim3 between the two Sim3 projection searches", "",
             "Written by `tools/time_optsim3.py`.  One launch of `k_sim3_optimize`, one workgroup of 256 lanes per problem, one wave per SIMD.  Registers (tools/kres.sh, "
             "clang 22 / ROCm 7.2): `k_sim3_optimize<4>` (n1 <= 1024) 256 VGPRs + 216 AGPRs of spill space, `k_sim3_optimize<0>` 256 VGPRs + 150 AGPRs, both 0 bytes of "
             "scratch -- the <4> instance is 40 AGPRs from scratch, which no kernel of kernels_match.hip may use "
             "(tests/test_abi_and_host.py::test_search_kernel_register_contract).  No speed-up is claimed: the parent has no device path, and the reference's host g2o was not timed.", ""]
    if a.gpu:
        lines += ["## Kernel time", ""]
        gpu_part(a, lines)
    else:
        lines += ["## Kernel time", "", "NOT MEASURED: this file was written without `--gpu`; the kernel has not been timed on an MI355X.", ""]
    cpu_part(lines)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
