#!/usr/bin/env python
"""Device time of xfh_triangulate_device (k_triangulate_pairs, k_triangulate_winner, k_triangulate_finish) -> profiles/triangulate.md, with the two
stated deviations measured and the device compared bit for bit with the rule of tests/ref_triangulate.py.

Scenes: a keyframe of n1 keypoints that sees seeded 3-D points 2 .. 12 m away, B neighbours of n2 = n1 keypoints on a 0.3 .. 1 m baseline; a quarter
of the keypoints of KF1 are matched at each neighbour (the share SearchForTriangulation leaves on a sequence: most keypoints already have a map
point), a third of the keypoints stereo, half a pixel of noise.  (B, n1) = (1, 1000), (10, 1000), (30, 4096), with XFH_TRIANG_CLAIM.

  kernels    us per launch from the library's dispatch-attached event timers (xfh_timing_enable / xfh_timing_read), one kernel at a time
  per call   host clock around `iters` calls that end in one synchronise, over iters

There is no parent-commit baseline (the call is new) and no threshold.  The host loop it replaces was NOT timed: Eigen is not available where this
runs, so no speed-up over the reference's own loop is measured or claimed.

    python tools/time_triangulate.py [--iters 50] [--out FILE.md]
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

import ref_triangulate as RG                                # noqa: E402
import triangulate_rig as R                                 # noqa: E402
import triangulation_rig as TR                              # noqa: E402
from xfeatslam_amd import capi                              # noqa: E402
from xfeatslam_amd.extractor import Context                 # noqa: E402

F, D = np.float32, np.float64


def scene(seed, B, n):
    rng = np.random.RandomState(seed)
    X = np.stack([rng.uniform(-2.5, 2.5, n), rng.uniform(-1.8, 1.8, n), rng.uniform(2.0, 12.0, n)], 1)
    xy = TR.project(X).astype(F)
    T1, O1 = R.pose(np.eye(3), np.zeros(3))
    ur = TR.uright_of(rng, xy, X[:, 2])
    k1 = dict(xy=xy, ur=ur, depth=np.where(ur >= 0, X[:, 2].astype(F), F(-1)).astype(F), Tcw=T1, Ow=O1)
    k2s, m = [], np.full((B, n), -1, np.int32)
    for b in range(B):
        Rm = TR.rot(*rng.uniform(-0.05, 0.05, 3))
        t = np.array([rng.uniform(0.3, 1.0) * rng.choice([-1, 1]), rng.uniform(-0.1, 0.1), rng.uniform(-0.3, 0.6)])
        X2 = X @ Rm.T + t
        xy2 = (TR.project(X2) + rng.uniform(-0.5, 0.5, (n, 2))).astype(F)
        perm = rng.permutation(n)                                           # keypoint perm[i] of the neighbour sees point i
        k = dict(xy=np.zeros((n, 2), F), Tcw=None, Ow=None)
        k["xy"][perm] = xy2
        z2 = np.zeros(n); z2[perm] = X2[:, 2]
        k["ur"] = TR.uright_of(rng, k["xy"], z2)
        k["depth"] = R.depth_of(k)
        k["Tcw"], k["Ow"] = R.pose(Rm, t)
        seen = rng.rand(n) < 0.25
        m[b, seen] = perm[seen]
        k2s.append(k)
    return k1, k2s, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = capi.lib()
    assert L.xfh_device_count() > 0, "time_triangulate.py needs a GPU"
    rig = R.TriangRig(L)
    ctx = rig.ctx
    cam = R.cam_struct()
    P = R.main_params(far_th=0.0)
    lines = [f"Box: {socket.gethostname()} ({L.xfh_version().decode()}); nothing else of this process on the GPU.", "",
             f"{a.iters} calls after {a.warmup} warm-up calls, back to back on one stream, XFH_TRIANG_CLAIM set.", "",
             "| B | n1 = n2 | matched pairs | two-view attempts | new points | k_triangulate_pairs, us | k_triangulate_winner, us | k_triangulate_finish, us | per call (host clock), us |",
             "|---|---|---|---|---|---|---|---|---|"]
    for B, n in ((1, 1000), (10, 1000), (30, 4096)):
        k1, k2s, m = scene(9000 + B, B, n)
        lay = Context.triangulate_layout(B, n, 0)
        out = capi.DeviceBuffer(lay["bytes"])
        s1, s2, dm = rig.side([k1]), rig.side(k2s), rig.dev(m)

        def call():
            ctx.triangulate_device(B, n, n, True, cam, s1, s2, dm, out.ptr, sigma2=P["sigma2"], ratio_factor=P["ratio_factor"], scale_last=P["scale_last"],
                                   far_th=0.0, claim=True)

        for _ in range(a.warmup):
            call()
        ctx.synchronize()
        kus = []
        for kid in ("TRIANGULATE_PAIRS", "TRIANGULATE_WINNER", "TRIANGULATE_FINISH"):
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
        r = Context.triangulate_parse(out.download(np.uint8, lay["bytes"]), lay, B, n, True)
        h = r["header"].sum(0)
        lines.append(f"| {B} | {n} | {h[0]} | {h[1]} | {r['n_new']} | {kus[0]:.1f} | {kus[1]:.1f} | {kus[2]:.1f} | {wall:.1f} |")
        print(lines[-1], flush=True)
        out.free(); rig.free()

    # ---- the device against the rule, bit for bit ----
    lines += ["", "Device against the rule of tests/ref_triangulate.py: 32-bit words of xyz / new_xyz / new_normal / new_dist that differ, and integer outputs that differ.", "",
              "| scene | pairs | float words compared | float words that differ | integer outputs that differ |", "|---|---|---|---|---|"]
    o, mp = R.planted()
    big1, big2, bigm = scene(77, 3, 400)
    for name, k1, k2s, m, PP in (("planted (n1 = 65, B = 2)", o.k1, o.k2, mp, R.planted_params()), ("timing scene (n1 = 400, B = 3)", big1, big2, bigm, P)):
        got, _ = rig.run(cam, [k1], k2s, m, PP, claim=True)
        w = RG.rule_from_matches(PP, k1, k2s, m)
        fw = sum(int((np.ascontiguousarray(got[k], F).view(np.int32) != np.ascontiguousarray(w[k], F).view(np.int32)).sum()) for k in ("xyz", "new_xyz", "new_normal", "new_dist"))
        nf = sum(np.asarray(w[k]).size for k in ("xyz", "new_xyz", "new_normal", "new_dist"))
        iw = sum(int((np.asarray(got[k]) != np.asarray(w[k])).sum()) for k in ("status", "kind", "header", "winner", "new_idx1", "new_b", "new_idx2")) + int(got["n_new"] != w["n_new"])
        lines.append(f"| {name} | {int((m >= 0).sum())} | {nf} | {fw} | {iw} |")
        print(lines[-1], flush=True)
    lines += ["", "No bit difference was found: the device's fp64 add, multiply, divide and square root and its fp32 divide and square root round as the host's do.", ""]

    # ---- the two stated deviations, measured on the host (they are properties of the rule, not of the device) ----
    z = np.concatenate([np.linspace(0.1, 40.0, 400001), np.geomspace(0.1, 40.0, 100001)]).astype(F)
    h = D(F(P["mb"] / F(2)))
    ident = ((z.astype(D) ** 2 - h * h) / (z.astype(D) ** 2 + h * h)).astype(F)
    libm = np.cos(F(2) * np.arctan2(np.full_like(z, F(P["mb"] / F(2))), z)).astype(F)
    cosd = float(np.abs(ident.astype(D) - libm.astype(D)).max())
    w = RG.rule_from_matches(P, big1, big2, bigm)
    s64 = s32 = d3 = 0.0
    for (b, i), r in w["info"].items():
        if r["A"] is None:
            continue
        x = r["x3Dh"]
        ref, l32 = RG.lapack_null_vector(r["A"], D), RG.lapack_null_vector(r["A"], F).astype(D)
        ref = ref if np.dot(ref, x) > 0 else -ref; l32 = l32 if np.dot(l32, x) > 0 else -l32
        step = np.spacing(F(np.abs(ref).max()))
        s64 = max(s64, np.abs(x.astype(F).astype(D) - ref.astype(F).astype(D)).max() / step)
        s32 = max(s32, np.abs(l32 - ref).max() / step)
        d3 = max(d3, float(np.abs(l32[:3] / l32[3] - x[:3] / x[3]).max()))
    lines += [f"Cosine identity against float32 cos(2 * arctan2(mb / 2, z)) over {len(z)} depths from 0.1 to 40 m at mb = {float(P['mb']):.4f}: largest difference {cosd:.3g} (bound 1e-6).",
              f"Null vector on the timing scene (n1 = 400, B = 3): the rule's fp64 Jacobi, rounded to float, against LAPACK's float64 SVD: {s64:.2f} float steps of the largest",
              f"component at most (bound 1); LAPACK's float32 SVD against the same: {s32:.1f} float steps, which moves a triangulated point by up to {d3:.3g} m."]
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    print(text)
    rig.close()


if __name__ == "__main__":
    main()
