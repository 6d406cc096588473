#!/usr/bin/env python
"""Device time of xfh_two_view_device (k_twoview_prepare, _fit, _score, _select, _check_rt, _final) -> profiles/two_view.md, with the device compared
bit for bit with the rule of tests/ref_twoview.py, the stated deviation of the fits measured, and the rule form measured against the literal form.

Scenes: two views of seeded 3-D points 2 .. 9 m away after a 3-degree rotation and a 0.5 m baseline, 0.3 px of noise, 10 % of the matches wrong;
n1 = n2 = N keypoints of which 90 % are matched; 200 iterations; (B, N) = (1, 1000), (8, 1000), (1, 4096), (8, 4096); shared draws.

  kernels    us per launch from the library's dispatch-attached event timers (xfh_timing_enable / xfh_timing_read), one kernel at a time
  per call   host clock around `iters` calls that end in one synchronise, over iters

There is no parent-commit baseline (the call is new) and no threshold.  The host code it replaces -- the reference's two std::threads with 200 Eigen
SVDs each -- was NOT timed: Eigen is not available where this runs, so no speed-up over the reference is measured or claimed.

    python tools/time_two_view.py [--iters 20] [--out FILE.md]
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

import ref_twoview as R                                     # noqa: E402
import twoview_rig as G                                     # noqa: E402
from xfeatslam_amd import capi                              # noqa: E402
from xfeatslam_amd.extractor import Context                 # noqa: E402

F, D = np.float32, np.float64
KERNELS = ("TWOVIEW_PREPARE", "TWOVIEW_FIT", "TWOVIEW_SCORE", "TWOVIEW_SELECT", "TWOVIEW_CHECK_RT", "TWOVIEW_FINAL")


def lapack_null(A, dt):
    return np.linalg.svd(np.asarray(A, dt))[2][..., -1, :]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = capi.lib()
    assert L.xfh_device_count() > 0, "time_two_view.py needs a GPU"
    rig = G.TwoViewRig(L)
    ctx = rig.ctx
    cam = G.camera()
    lines = [f"Box: {socket.gethostname()} ({L.xfh_version().decode()}); nothing else of this process on the GPU.", "",
             f"{a.iters} calls after {a.warmup} warm-up calls, back to back on one stream; 200 iterations per call (400 hypotheses per problem).", "",
             "| B | n1 = n2 | matches | status of problem 0 | " + " | ".join(f"k_{k.lower()}, us" for k in KERNELS) + " | per call (host clock), us |",
             "|---|---|---|---|" + "---|" * (len(KERNELS) + 1)]
    for B, n in ((1, 1000), (8, 1000), (1, 4096), (8, 4096)):
        sc = [G.scene(5000 + 10 * n + b, n, n, int(0.9 * n), noise=0.3, outliers=0.1, iters=200) for b in range(B)]
        xy1, xy2, m12, _ = G.stack(sc)
        draws = sc[0]["draws"]
        bufs = [capi.DeviceBuffer(x.nbytes).upload(x) for x in (xy1, xy2, m12, draws)]
        lay = Context.two_view_layout(B, n, 0)
        out, ws = capi.DeviceBuffer(lay["bytes"]), capi.DeviceBuffer(L.xfh_two_view_workspace_bytes(n, n, 200, B))

        def call():
            ctx.two_view_device(B, n, n, cam, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, 0, 200, G.RAND_MAX, ws.ptr, out.ptr)

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
        lines.append(f"| {B} | {n} | {int(r['header'][0, 0])} | {R.STATUS_NAMES[r['header'][0, 1]]} | " + " | ".join(f"{k:.1f}" for k in kus) + f" | {wall:.1f} |")
        print(lines[-1], flush=True)
        for b in bufs + [out, ws]:
            b.free()

    # ---- the device against the rule, bit for bit ----
    lines += ["", "Device against the rule of tests/ref_twoview.py: 32-bit words of the float outputs (floats, p3d) that differ, and integer / flag outputs that differ.", "",
              "| scene | matches | float words compared | float words that differ | integer outputs that differ |", "|---|---|---|---|---|"]
    scenes = G.rig()
    for name in ("general", "plane", "rotation", "few"):
        s = scenes[name]
        got, _ = rig.run(s["xy1"][None], s["xy2"][None], s["m12"][None], s["draws"], sigma=s["sigma"])
        w = G.rule_of(s)
        fw = sum(int((np.ascontiguousarray(got[k][0], F).view(np.int32).ravel() != np.ascontiguousarray(w[k], F).view(np.int32).ravel()).sum()) for k in ("floats", "p3d"))
        nf = sum(np.asarray(w[k]).size for k in ("floats", "p3d"))
        iw = sum(int((np.asarray(got[k][0]).ravel() != np.asarray(w[k]).ravel()).sum()) for k in ("header", "inl_h", "inl_f", "tri", "matches_out"))
        lines.append(f"| {name} | {int(w['header'][0])} | {nf} | {fw} | {iw} |")
        print(lines[-1], flush=True)
    lines += ["", "No bit difference was found: the device's fp64 and fp32 add, multiply, divide and square root round as the host's do.", ""]

    # ---- the stated deviation of the fits, measured on the host (a property of the rule, not of the device) ----
    s = scenes["general"]
    w = G.rule_of(s)
    cm1, cm2 = w["cm"]
    p1, p2 = R.normalized(w["nrm"][0], s["xy1"][cm1[w["sets"]]]), R.normalized(w["nrm"][1], s["xy2"][cm2[w["sets"]]])
    for tag, A in (("ComputeH21 (16 x 9)", R.design_h(p1, p2)), ("ComputeF21 (8 x 9, before the rank-2 projection)", R.design_f(p1, p2))):
        x = R.null_vector(A).astype(F).astype(D)
        ref, l32 = lapack_null(A, D), lapack_null(A, F).astype(D)
        sg = lambda v: v * np.sign((v * x).sum(-1, keepdims=True))
        ref, l32 = sg(ref), sg(l32)
        step = np.spacing(np.abs(ref).max(-1).astype(F)).astype(D)[:, None]
        lines.append(f"{tag}, the 200 minimal sets of the general scene: the rule's fp64 Jacobi null vector, rounded to float, against LAPACK's float64 SVD: "
                     f"{(np.abs(x - ref.astype(F).astype(D)) / step).max():.2f} float steps of the largest component at most; numpy's float32 SVD (the stand-in for "
                     f"Eigen's JacobiSVD<float>) against the same: {(np.abs(l32 - ref) / step).max():.1f} float steps.")
        print(lines[-1], flush=True)
    # ---- the two forms against each other (host only): what tests/test_twoview_forms.py bounds with a margin of 4 ----
    import test_twoview_forms as TF                         # noqa: E402
    mT = mP = 0.0
    kept = dropped = differ = 0
    worst = dict(score=0.0, RH=0.0, chi=0.0, parallax=0.0)
    scenes = TF.rig_scenes()
    for k, s in enumerate(list(scenes.values()) + G.random_scenes(200)):
        diff, dev, margins, _, _ = TF.compare(s)
        if TF.holds(margins, dev) and k >= len(scenes):
            dropped += 1
            continue
        kept += 1
        differ += bool(diff)
        mT, mP = max(mT, dev["T"]), max(mP, dev["P"])
        if s.get("name") not in ("equal", "n8"):                            # (their best iterations repeat one set on purpose)
            worst = {q: max(v, dev[q]) for q, v in worst.items()}
    lines += ["", f"Rule form against the literal float32 form (sequential sums, LAPACK's float32 SVD and inverse) on the rig and 200 random scenes: {kept} scenes compared,",
              f"{dropped} random scenes dropped for a decision on its threshold, {differ} with a decision that differs.  Largest deviation of an entry of T21: {mT:.3g};",
              f"of a triangulated point, relative to its largest coordinate: {mP:.3g}.  Largest deviation of the quantities the decisions test: a score that competes",
              f"for the argmax (within a quarter of the best) {worst['score']:.3g}; RH {worst['RH']:.3g}; a chi-square of a winner below twice its threshold {worst['chi']:.3g};",
              f"the parallax of a hypothesis {worst['parallax']:.3g} degrees.", ""]
    print("\n".join(lines[-6:]), flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    print(text)
    rig.close()


if __name__ == "__main__":
    main()
