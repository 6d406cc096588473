#!/usr/bin/env python
"""Device time of xfh_sim3_solve_device (k_sim3solve_prepare, _fit, _count, _decide) and of xfh_sim3_merge_matches_device (its three launches)
-> profiles/sim3_solver.md, with the device compared bit for bit with the rule of tests/ref_sim3solve.py, the stated deviation of the
eigenvector measured, and the rule form measured against the literal form.

Scenes at the caller's shape: n1 = 4096 keypoint slots of which 300 carry a correspondence, none of them consistent, so that all 300 iterations
run (the longest call; a converging call stops counting early only on the host: the device always runs the table's count); B = 1, 3 and 8
candidates; shared draws.  The merge: J = 5 covisibles of n1 = n2 = 4096 over M = 20000 points.

  kernels    us per launch from the library's dispatch-attached event timers (xfh_timing_enable / xfh_timing_read), one kernel at a time
  per call   host clock around `iters` calls that end in one synchronise, over iters

Without --gpu only the CPU part runs (the deviations between the forms), and the file says that the kernel times are unmeasured.  There is no
parent-commit baseline (the calls are new) and no threshold.  The host code they replace -- the reference's Sim3Solver with up to 300 Eigen
eigen-decompositions -- was NOT timed: Eigen is not available where this runs, so no speed-up over the reference is measured or claimed.

    python tools/time_sim3_solver.py [--gpu] [--iters 50] [--out FILE.md]
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

import ref_sim3solve as R                                   # noqa: E402
import sim3solve_rig as G                                   # noqa: E402
from xfeatslam_amd import capi                              # noqa: E402
from xfeatslam_amd.extractor import Context                 # noqa: E402

F, D = np.float32, np.float64
KERNELS = ("SIM3SOLVE_PREPARE", "SIM3SOLVE_FIT", "SIM3SOLVE_COUNT", "SIM3SOLVE_DECIDE")


def gpu_part(a, lines):
    L = capi.lib()
    assert L.xfh_device_count() > 0, "time_sim3_solver.py --gpu needs a GPU"
    rig = G.Sim3SolveRig(L)
    ctx = rig.ctx
    lines += [f"Box: {socket.gethostname()} ({L.xfh_version().decode()}); nothing else of this process on the GPU.", "",
              f"{a.iters} calls after {a.warmup} warm-up calls, back to back on one stream; n1 = 4096, 300 correspondences, 300 iterations per problem.", "",
              "| B | N | status of problem 0 | " + " | ".join(f"k_{k.lower()}, us" for k in KERNELS) + " | per call (host clock), us |", "|---|---|---|" + "---|" * (len(KERNELS) + 1)]
    n1 = 4096
    for B in (1, 3, 8):
        s = G.scene(7000 + B, n1=n1, M=n1 * (B + 1), N=300, B=B, inlier_frac=0.0)
        M_b = len(s["points"])
        draws = s["draws"][0]
        ins = [s["points"], s["point1"], s["matched"], s["T1w"], s["T2w"], s["table"], draws]
        bufs = [capi.DeviceBuffer(np.asarray(x).nbytes).upload(np.ascontiguousarray(x)) for x in ins]
        lay = Context.sim3_solve_layout(B, n1, 0)
        out, ws = capi.DeviceBuffer(lay["bytes"]), capi.DeviceBuffer(L.xfh_sim3_solve_workspace_bytes(n1, M_b, B))
        cam1, cam2 = G.camera(G.CAM), G.camera(G.CAM2)

        def call():
            ctx.sim3_solve_device(B, n1, M_b, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, 0, bufs[4].ptr, cam1, cam2, bufs[5].ptr, len(draws), bufs[6].ptr, 0,
                                  G.RAND_MAX, ws.ptr, out.ptr)

        for _ in range(a.warmup):
            call()
        ctx.synchronize()
        kus = []
        for kid in KERNELS:
            ctx.timing_enable(capi.K[kid])
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
        wall = (time.perf_counter() - t0) * 1e6 / a.iters
        r = lay.parse(out.download(np.uint8, lay["bytes"]))
        lines.append(f"| {B} | {int(r['header'][0, 0])} | {R.STATUS_NAMES[r['header'][0, 1]]} after {int(r['header'][0, 7])} iterations | " + " | ".join(f"{k:.1f}" for k in kus)
                     + f" | {wall:.1f} |")
        print(lines[-1], flush=True)
        for b in bufs + [out, ws]:
            b.free()
    # the merge
    rng = np.random.RandomState(5)
    J, n2, Mm = 5, 4096, 20000
    m12, p2 = rng.randint(-2000, n2, (J, n1)).astype(np.int32), rng.randint(-2000, Mm, (J, n2)).astype(np.int32)
    bufs = [capi.DeviceBuffer(x.nbytes).upload(x) for x in (m12, p2)]
    ws, out = capi.DeviceBuffer(L.xfh_sim3_solve_workspace_bytes(n1, Mm, 1)), capi.DeviceBuffer(8 * n1 + 256)
    call = lambda: ctx.sim3_merge_matches_device(J, n1, n2, Mm, bufs[0].ptr, bufs[1].ptr, ws.ptr, out.ptr, out.ptr + 4 * n1, out.ptr + 8 * n1)
    for _ in range(a.warmup):
        call()
    ctx.synchronize()
    ctx.timing_enable(capi.K["SIM3SOLVE_MERGE"])
    for _ in range(a.iters):
        call()
    ctx.synchronize()
    cnt, ms = ctx.timing_read()
    ctx.timing_enable(capi.K["NONE"])
    t0 = time.perf_counter()
    for _ in range(a.iters):
        call()
    ctx.synchronize()
    wall = (time.perf_counter() - t0) * 1e6 / a.iters
    got = out.download(np.int32, 2 * n1 + 1)
    want = R.merge(m12, p2, Mm)
    same = np.array_equal(got[:n1], want[0]) and np.array_equal(got[n1:2 * n1], want[1]) and got[2 * n1] == want[2]
    lines += ["", f"The merge, J = {J}, n1 = n2 = {n1}, M = {Mm}: {ms * 1e3 / max(cnt, 1):.1f} us per launch over its three launches (k_sim3merge_init, _claim, _select), "
              f"{wall:.1f} us per call by the host clock; {int(got[2 * n1])} owners; equal to the rule: {same}.", ""]
    print(lines[-2], flush=True)
    for b in bufs + [ws, out]:
        b.free()
    # ---- the device against the rule, bit for bit ----
    lines += ["Device against the rule of tests/ref_sim3solve.py: 32-bit words of the float outputs that differ (a NaN equal to any NaN), and integer / flag outputs that differ.", "",
              "| scene | N | status | float words compared | float words that differ | integer outputs that differ |", "|---|---|---|---|---|---|"]
    scenes = G.rig()
    for name in ("first", "after64", "no_more", "collinear", "zero_rotation", "nan_point", "big", "big_outliers"):
        s = scenes[name]
        got, _ = rig.run(s)
        w = G.rule_of(s)
        fk = [k for k in ("floats", "Tcw", "Ow") if w[k] is not None]
        fw = sum(int((G.canonical_nan(got[k][0]).view(np.int32).ravel() != G.canonical_nan(w[k]).view(np.int32).ravel()).sum()) for k in fk)
        nf = sum(np.asarray(w[k]).size for k in fk)
        iw = int((got["header"][0] != w["header"]).sum()) + (int((got["inliers"][0] != w["inliers"]).sum()) if w["inliers"] is not None else 0)
        lines.append(f"| {name} | {int(w['header'][0])} | {R.STATUS_NAMES[w['header'][1]]} | {nf} | {fw} | {iw} |")
        print(lines[-1], flush=True)
    lines += [""]
    rig.close()


def cpu_part(lines):
    """the stated deviations, measured on the host: properties of the rule, not of the device"""
    import test_sim3solve_forms as TF                        # noqa: E402
    scenes = G.rig()
    # the fp64 Jacobi against LAPACK's symmetric eigen-solver in float64, and LAPACK's float32 general solver (the stand-in for Eigen's) against the same
    worst_j = worst_l = 0.0
    count = 0
    for name in ("after64", "big_outliers", "its65"):
        s = scenes[name]
        w = G.rule_of(s)
        for it in range(w["its"]):
            P1, P2 = w["X1"][w["sets"][it]], w["X2"][w["sets"][it]]
            Pr1, Pr2 = P1 - ((P1[0] + P1[1]) + P1[2]) / F(3), P2 - ((P2[0] + P2[1]) + P2[2]) / F(3)
            Mx = np.array([[(Pr2[0, i] * Pr1[0, j] + Pr2[1, i] * Pr1[1, j]) + Pr2[2, i] * Pr1[2, j] for j in range(3)] for i in range(3)], F)
            N = np.array([[(Mx[0, 0] + Mx[1, 1]) + Mx[2, 2], Mx[1, 2] - Mx[2, 1], Mx[2, 0] - Mx[0, 2], Mx[0, 1] - Mx[1, 0]],
                          [0, (Mx[0, 0] - Mx[1, 1]) - Mx[2, 2], Mx[0, 1] + Mx[1, 0], Mx[2, 0] + Mx[0, 2]],
                          [0, 0, (-Mx[0, 0] + Mx[1, 1]) - Mx[2, 2], Mx[1, 2] + Mx[2, 1]], [0, 0, 0, (-Mx[0, 0] - Mx[1, 1]) + Mx[2, 2]]], F)
            N = np.triu(N) + np.triu(N, 1).T
            ev, evec = np.linalg.eigh(N.astype(D))
            if ev[3] - ev[2] < 1e-3 * abs(ev[3]):                           # a near-double largest eigenvalue: the eigenvector is not defined to this precision
                continue
            ref = evec[:, 3]
            q = np.array(R.max_eigenvector(N.tolist())[0], D)
            e32, v32 = np.linalg.eig(N)
            l32 = v32.real[:, int(np.argmax(e32.real))].astype(D)
            sg = lambda v: v * np.sign(v @ ref)
            worst_j, worst_l = max(worst_j, float(np.abs(sg(q) - ref).max())), max(worst_l, float(np.abs(sg(l32) - ref).max()))
            count += 1
    lines += ["Deviation between the forms (measured on the CPU; properties of the rule, not of the device).", "",
              f"The eigenvector of the largest eigenvalue over the {count} minimal sets of the scenes after64, its65 and big_outliers whose largest eigenvalue is "
              f"separated by more than 1e-3 of itself: the rule's fp64 two-sided Jacobi against LAPACK's float64 symmetric solver: {worst_j:.3g} in the largest "
              f"component of the unit quaternion; LAPACK's float32 general solver (the stand-in for Eigen::EigenSolver<Matrix4f>) against the same: {worst_l:.3g}.", ""]
    print(lines[-2], flush=True)
    dev = [0.0, 0.0]
    differ = compared = 0
    tight = np.inf
    for s in list(scenes.values()) + G.random_scenes(200):
        n = s.get("name")
        rule, lit = G.rule_of(s), TF.literal_of(s)
        lit["best_n"] = int(lit["best"]["flags"].sum()) if lit["best"] else 0
        if n == "zero_rotation":
            continue
        try:
            TF.decisions_equal(rule, lit, n)
        except AssertionError:
            differ += 1
        if rule["header"][1] == R.TOO_FEW or rule["header"][5] in TF.DEGENERATE_ITERATIONS.get(n, ()) or not np.isfinite(rule["floats"][:12]).all():
            continue
        d = TF.deviation(rule, lit)
        dev = [max(dev[0], d[0]), max(dev[1], d[1])]
        compared += 1
    lines += [f"Rule form against the literal float32 form (the sequential iterate(20) loop, LAPACK's float32 general eigen-solver, atan2 -> angle-axis -> SO3",
              f"exponential) on the rig and 200 random scenes: {compared} reported similarities compared, {differ} scenes with a decision that differs.  Largest deviation",
              f"of an entry of T12: {dev[0]:.3g} in the rotation-and-scale block, {dev[1]:.3g} in the translation (scenes a few units across; the largest",
              f"figures come from the best hypothesis of calls that do NOT converge, fitted to an ill-conditioned triple).  tests/test_sim3solve_forms.py holds every scene to",
              f"4x these figures and the rig's inlier tests to a margin of 8x the deviation of the error they compare.  The zero-rotation scene is exempt: the literal",
              f"form divides 0 by 0 there.", ""]
    print("\n".join(lines[-7:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []
    if a.gpu:
        gpu_part(a, lines)
    else:
        lines += ["Kernel times: NOT MEASURED (this file was written by a run without --gpu).", ""]
    cpu_part(lines)
    lines += ["The host code these calls replace -- the reference's Sim3Solver with up to 300 Eigen eigen-decompositions per candidate -- was not timed: Eigen is not",
              "available where this runs.  No speed-up over the reference is measured or claimed.", ""]
    text = "\n".join(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
