#!/usr/bin/env python
"""Device time of xfh_mlpnp_solve_device (k_mlpnp_prepare, _fit, _count, _records, _refine, _decide) and of the three-call relocalisation chain
xfh_bow_search_device (shared = 2) -> xfh_mlpnp_solve_device -> xfh_pose_optimize_device -> the "Times" section of profiles/mlpnp.md.

The caller's shape: B = 8 candidate keyframes against one frame of n = 4096 keypoints, about 150 of which carry a correspondence per candidate,
70 % of them correct, 35 iterations (eps 0.5), chunk 5, shared draws.  The device always runs the whole loop (35 iterations per problem) whatever
the iteration at which the sequential loop would have returned.

  kernels     us per launch from the library's dispatch-attached event timers (xfh_timing_enable / xfh_timing_read), one kernel family at a time
  per call    host clock around `iters` calls that end in one synchronise, over iters; `repeats` such windows: median and (min .. max)
  host form   xfh_mlpnp_solve_host on ONE thread on the same problems, the same way

The device's outputs are compared with the host form's on the way (integers and flags equal, Tcw within one float32 step).  There is no
parent-commit baseline (the calls are new) and no threshold.  The reference's MLPnPsolver (one CPU thread per candidate, Eigen) was NOT timed: Eigen
is not available where this runs, so no speed-up over the reference is measured or claimed.  Without a GPU the tool fails: it does not fall back.

With --forms nothing is timed and no GPU is needed: the rule of tests/ref_mlpnp.py is held against the literal form of tests/ref_mlpnp_literal.py (with
Refine's result stored) on the 200 random scenes of tests/mlpnp_rig.py, and the largest |Tcw rule - Tcw literal|, rotation and translation entries
apart, goes into the "Forms" section of the same file; tests/test_mlpnp_forms.py allows 4x that figure.

    python tools/time_mlpnp.py [--iters 50] [--warmup 10] [--repeats 5] [--out profiles/mlpnp.md]
    python tools/time_mlpnp.py --forms [--out profiles/mlpnp.md]
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

import mlpnp_rig as G                                       # noqa: E402
import ref_mlpnp as R                                       # noqa: E402
from xfeatslam_amd import capi                              # noqa: E402
from xfeatslam_amd.extractor import Context                 # noqa: E402

F = np.float32
KERNELS = ("MLPNP_PREPARE", "MLPNP_FIT", "MLPNP_COUNT", "MLPNP_RECORDS", "MLPNP_REFINE", "MLPNP_DECIDE")
CHAIN = ("BOW_CANDIDATES", "BOW_RESOLVE") + KERNELS + ("POSE_OPTIMIZE",)
BEGIN, END = "<!-- times:begin (tools/time_mlpnp.py) -->", "<!-- times:end -->"
FBEGIN, FEND = "<!-- forms:begin (tools/time_mlpnp.py --forms) -->", "<!-- forms:end -->"
B, N_KP, N_CORR = 8, 4096, 150


def windows(ctx, call, a):
    """-> (median, min, max) us per call over a.repeats windows of a.iters calls"""
    w = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        for _ in range(a.iters):
            call()
        ctx.synchronize()
        w.append((time.perf_counter() - t0) * 1e6 / a.iters)
    return float(np.median(w)), min(w), max(w)


def kernel_times(ctx, call, kernels, a):
    out = []
    for kid in kernels:
        ctx.timing_enable(capi.K[kid])
        for _ in range(a.iters):
            call()
        ctx.synchronize()
        cnt, ms = ctx.timing_read()
        ctx.timing_enable(capi.K["NONE"])
        out.append((cnt / a.iters, ms * 1e3 / max(cnt, 1)))
    return out


def bow_sides(rng):
    """B candidate keyframes and one frame of N_KP rows each: N_CORR one-member nodes on both sides whose rows nearly agree, every other keypoint in no node"""
    node = np.full(N_KP, 0xFFFFFFFF, np.uint32)
    unit = lambda v: (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F)
    frame = dict(node_of=node.copy(), desc=unit(rng.randn(N_KP, 64)))
    fk = rng.choice(N_KP, N_CORR, replace=False)
    frame["node_of"][fk] = np.arange(N_CORR, dtype=np.uint32)
    cands = []
    for b in range(B):
        c = dict(node_of=node.copy(), desc=unit(rng.randn(N_KP, 64)), active=np.ones(N_KP, np.uint8))
        ck = rng.choice(N_KP, N_CORR, replace=False)
        c["node_of"][ck] = np.arange(N_CORR, dtype=np.uint32)
        c["desc"][ck] = unit(frame["desc"][fk] + 0.02 * rng.randn(N_CORR, 64))
        cands.append(c)
    return cands, frame


def put_section(path, begin, end, text):
    if os.path.exists(path):
        old = open(path).read()
        if begin in old and end in old:
            text = old[:old.index(begin)] + text.rstrip("\n") + old[old.index(end) + len(end):]
        else:
            text = old.rstrip("\n") + "\n\n" + text
    with open(path, "w") as f:
        f.write(text)
    print("wrote", path)


def forms(a):
    scenes = G.random_scenes()
    rot_d, tr_d, used, exempt = G.forms_deviation(scenes)
    text = "\n".join([FBEGIN, "## Forms", "",
                      f"The rule (`tests/ref_mlpnp.py`) against the literal form with Refine's result stored (`tests/ref_mlpnp_literal.py`) on the {len(scenes)} random scenes of "
                      f"`tests/mlpnp_rig.py` (0.5 px of noise, 30 % wrong matches, 12 iterations): {used} scenes report a pose in both forms, {exempt} of the {len(scenes)} are exempt "
                      "(the two least eigenvalues of `A^T A` of the reported solve within 1e-6 relative).", "",
                      f"Largest `|Tcw rule - Tcw literal|` of the float32 poses: rotation entries {rot_d:.3g}, translation entries {tr_d:.3g}.", "",
                      "`tests/test_mlpnp_forms.py` allows 4x these figures and never less than one float32 step of the entry (the format both forms round to).", FEND]) + "\n"
    put_section(a.out, FBEGIN, FEND, text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--forms", action="store_true")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlpnp.md"))
    a = ap.parse_args()
    if a.forms:
        return forms(a)
    L = capi.lib()
    assert L.xfh_device_count() > 0, "time_mlpnp.py needs a GPU: nothing is measured without one"
    ctx = Context(nfeatures=1, max_height=32, max_width=32)
    cam = G.camera()
    lines = [BEGIN, "## Times", "", f"Box: {socket.gethostname()} ({L.xfh_version().decode()}); nothing else of this process on the GPU.", "",
             f"B = {B} problems, n = {N_KP} keypoints, chunk 5, shared draws; {a.repeats} windows of {a.iters} calls after {a.warmup} warm-up calls, back to back on one stream, "
             "each window ending in one synchronise.  Kernel columns: us per launch from the dispatch-attached event timers, one kernel family at a time.", ""]
    bufs = []

    def dev(x):
        b = capi.DeviceBuffer(max(np.ascontiguousarray(x).nbytes, 16)).upload(np.ascontiguousarray(x))
        bufs.append(b)
        return b
    # ---- the solver alone --------------------------------------------------------------------------------------------------------------------
    s = G.scene(9000, n=N_KP, N=N_CORR, B=B, inlier_frac=0.7)
    nq, draws = s["points"].shape[1], s["draws"][0]
    max_iters = len(draws)
    ins = [dev(x) for x in (s["xy"], s["assigned"], s["points"], s["valid"], s["tables"][0], s["tables"][1], draws)]
    lay = Context.mlpnp_layout(B, N_KP, 0)
    out, ws = dev(np.zeros(lay["bytes"], np.uint8)), dev(np.zeros(L.xfh_mlpnp_workspace_bytes(N_KP, nq, B, max_iters), np.uint8))

    def solve():
        ctx.mlpnp_solve_device(B, N_KP, nq, ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, cam, s["max_err"], ins[4].ptr, ins[5].ptr, 5, None, max_iters, ins[6].ptr, 0,
                               G.RAND_MAX, ws.ptr, out.ptr)
    for _ in range(a.warmup):
        solve()
    ctx.synchronize()
    kt = kernel_times(ctx, solve, KERNELS, a)
    med, lo, hi = windows(ctx, solve, a)
    got = lay.parse(out.download(np.uint8, lay["bytes"]))
    t0 = time.perf_counter()
    host = G.host_of(dict(s, draws=s["draws"][:1]))
    host_us = (time.perf_counter() - t0) * 1e6
    hw = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        G.host_of(dict(s, draws=s["draws"][:1]))
        hw.append((time.perf_counter() - t0) * 1e6)
    same = all(np.array_equal(got[k], host[k]) for k in ("header", "inliers", "assigned_out")) and int(G.float_steps(got["Tcw"], host["Tcw"]).max()) <= 1
    hd = [dict(zip(R.HEADER, got["header"][b].tolist())) for b in range(B)]
    lines += [f"`xfh_mlpnp_solve_device`, N = {[h['N'] for h in hd]}, its = {hd[0]['its']} (all run on the device), statuses {[R.STATUS[h['status']] for h in hd]}, "
              f"winners {[h['winner'] for h in hd]}, Refine evaluations {[h['refines'] for h in hd]}; device against `xfh_mlpnp_solve_host`: "
              f"{'integers and flags equal, Tcw within one float32 step' if same else 'DIFFERENT'}.", "",
              "| " + " | ".join(f"k_{k.lower()}, us" for k in KERNELS) + " | per call, us: median (min .. max) | host form on one thread, us: median (min .. max) |",
              "|" + "---|" * (len(KERNELS) + 2),
              "| " + " | ".join(f"{us:.1f}" for _, us in kt) + f" | {med:.1f} ({lo:.1f} .. {hi:.1f}) | {np.median(hw):.0f} ({min(hw):.0f} .. {max(hw):.0f}) |", "",
              f"The host form's figure is Python's clock around the ctypes call for all {B} problems one after the other (first call {host_us:.0f} us); the "
              "reference gives each candidate a solver of its own and was not timed.", ""]
    print("\n".join(lines[-8:]), flush=True)
    assert same, "the device and the host form disagree"
    # ---- the chain ------------------------------------------------------------------------------------------------------------------------------
    import bow_rig as BR
    rng = np.random.RandomState(17)
    cands, frame = bow_sides(rng)
    s1, s2 = BR.BowRig.side(cands, "active"), BR.BowRig.side([frame], None)
    lay_b = Context.bow_search_layout(B, N_KP, N_KP, 0)
    out_b, ws_b = dev(np.zeros(lay_b["bytes"], np.uint8)), dev(np.zeros(Context.bow_search_workspace_bytes(N_KP, N_KP, B), np.uint8))
    d1 = [dev(s1[k]).ptr for k in ("blob", "flag", "desc")]; d2 = [dev(s2["blob"]).ptr, None, dev(s2["desc"]).ptr]

    def bow():
        ctx.bow_search_device(B, N_KP, N_KP, 2, *d1, s1["stride"], *d2, s2["stride"], ws_b.ptr, out_b.ptr, nn_ratio=0.75)
    bow()
    ctx.synchronize()
    raw = out_b.download(np.uint8, lay_b["bytes"])
    a2 = raw[lay_b["assigned2"]:lay_b["assigned2"] + 4 * B * N_KP].view(np.int32).reshape(B, N_KP)
    xy = np.stack([rng.uniform(20, 732, N_KP), rng.uniform(20, 460, N_KP)], 1).astype(F)
    pts = np.zeros((B, N_KP, 3), F)
    for b in range(B):
        Rm, t = G.rot(rng.randn(3), 25.0), rng.uniform(-1, 1, 3)
        blk = rng.uniform(-30, 30, (N_KP, 3))
        for k in np.nonzero(a2[b] >= 0)[0]:
            if rng.rand() < 0.3:
                continue
            px = xy[k] + 0.4 * rng.randn(2)
            Xc = rng.uniform(3, 9) * np.array([(px[0] - float(G.CAM[2])) / float(G.CAM[0]), (px[1] - float(G.CAM[3])) / float(G.CAM[1]), 1.0])
            blk[a2[b, k]] = (Xc - t) @ Rm
        pts[b] = blk
    tables = R.iterations_table(N_KP)
    cin = [dev(x) for x in (xy, pts, tables[0], tables[1], np.tile(xy, (B, 1, 1)))]         # the optimiser takes d_xy_un [B][nt][2]: the frame's keypoints once per candidate
    out_m = dev(np.zeros(lay["bytes"], np.uint8))
    ws_m = dev(np.zeros(L.xfh_mlpnp_workspace_bytes(N_KP, N_KP, B, max_iters), np.uint8))
    ws_p = dev(np.zeros(Context.pose_optimize_workspace_bytes(N_KP, B), np.uint8))
    po = [dev(np.zeros(nb, np.uint8)) for nb in (48 * B, N_KP * B, 4 * N_KP * B, 32 * B, 8 * B)]

    def chain():
        bow()
        ctx.mlpnp_solve_device(B, N_KP, N_KP, cin[0].ptr, out_b.ptr + lay_b["assigned2"], cin[1].ptr, None, cam, G.MAX_ERR, cin[2].ptr, cin[3].ptr, 5, None, max_iters,
                               ins[6].ptr, 0, G.RAND_MAX, ws_m.ptr, out_m.ptr, min_matches=15, d_n_matches=out_b.ptr + lay_b["n_matches"])
        ctx.pose_optimize_device(B, N_KP, N_KP, out_m.ptr + lay["Tcw"], cam, cin[4].ptr, None, out_m.ptr + lay["assigned_out"], cin[1].ptr, ws_p.ptr, *[b.ptr for b in po],
                                 inv_sigma2=1.0)
    for _ in range(a.warmup):
        chain()
    ctx.synchronize()
    kt = kernel_times(ctx, chain, CHAIN, a)
    med, lo, hi = windows(ctx, chain, a)
    gm = lay.parse(out_m.download(np.uint8, lay["bytes"]))
    ret = po[3].download(np.uint8, 32 * B).view(np.int32).reshape(B, 8)[:, 2]
    lines += [f"The chain `xfh_bow_search_device` (shared = 2) -> `xfh_mlpnp_solve_device` -> `xfh_pose_optimize_device` on one stream, nothing read back in between: "
              f"BoW matches {[int((r >= 0).sum()) for r in a2]}, MLPnP statuses {[R.STATUS[v] for v in gm['header'][:, 1]]}, PoseOptimization returns {ret.tolist()}.", "",
              "| kernel family | launches per chain | us per launch |", "|---|---|---|"]
    lines += [f"| k_{k.lower()} | {n:.0f} | {us:.1f} |" for k, (n, us) in zip(CHAIN, kt)]
    lines += ["", f"Per chain (host clock): {med:.1f} us median ({lo:.1f} .. {hi:.1f}).", END]
    print("\n".join(lines[-16:]), flush=True)
    for b in bufs:
        b.free()
    ctx.close()
    put_section(a.out, BEGIN, END, "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
