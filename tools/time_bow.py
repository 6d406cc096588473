#!/usr/bin/env python
"""Device time of xfh_bow_search_device (k_bow_candidates, k_bow_resolve) -> profiles/bow_search.md.

Synthetic keyframes of nfeatures = 1000 and 4096 keypoints with about ten and about forty members per vocabulary node (node ids uniform
over nfeatures / 10 resp. nfeatures / 40 nodes).  A base keyframe and 20 keyframes derived from it: six keypoints in ten keep the base
keypoint's node and a row at DescriptorDistance 5 .. 120 from its row (a true correspondence), the others get a random node and a random
unit row; nine in ten keypoints are active resp. eligible.  Three shapes, frame form (flags 0, eligible2 = NULL), nn_ratio 0.7:
  B = 1                one derived keyframe against the base (TrackReferenceKeyFrame)
  B = 10, shared = 2   ten derived keyframes against the base as side 2 (Relocalization: the candidates against one frame)
  B = 20, shared = 1   the base as side 1 against twenty derived keyframes (LoopClosing: the current keyframe against its covisibles)

  one launch   each kernel per launch from the library's dispatch-attached event timers (xfh_timing_enable / xfh_timing_read): the
               kernel's own begin .. end, what rocprofv3 --kernel-trace shows; the three memsets of a call are in neither column
  B calls      the same B problems as B separate B = 1 calls, the times of both kernels summed (launch gaps are not in either column)
  re-searches  queries whose truncated candidate list ran out of unclaimed entries (the workspace counter), of the queries resolved

There is no parent-commit baseline (the call is new) and no threshold: the file records what was measured, on which box and clock state.
The reference's own loop cannot be built without OpenCV: no speed-up over it is claimed.

    python tools/time_bow.py [--iters 200] [--out FILE.md]
"""
import argparse
import os
import socket
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import bow_rig as BR                                       # noqa: E402
import triangulation_rig as TR                             # noqa: E402
from xfeatslam_amd import capi                              # noqa: E402
from xfeatslam_amd.extractor import Context                 # noqa: E402

F = np.float32
KERNELS = ("BOW_CANDIDATES", "BOW_RESOLVE")


def base_keyframe(rng, n, per_node):
    return dict(node_of=rng.randint(0, max(n // per_node, 1), n).astype(np.uint32), desc=TR.unit_rows(rng, n), flag=(rng.rand(n) < 0.9).astype(np.uint8))


def derived(rng, base, per_node):
    n = len(base["node_of"])
    k = base_keyframe(rng, n, per_node)
    keep = rng.rand(n) < 0.6
    step = np.sqrt(rng.uniform(5, 120, n) / 512.0)[:, None] * TR.unit_rows(rng, n).astype(np.float64)
    rows = base["desc"].astype(np.float64) + step
    rows = (rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(F)
    perm = rng.permutation(n)                               # a correspondence is not at the same index
    k["node_of"][perm[keep]] = base["node_of"][keep]; k["desc"][perm[keep]] = rows[keep]
    return k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = capi.lib()
    assert L.xfh_device_count() > 0, "time_bow.py needs a GPU"
    ctx = Context(nfeatures=1, max_height=32, max_width=32)
    BMAX = 20
    sclk = capi.C.c_double(0.0); spread = capi.C.c_double(0.0)
    clock = "not read"
    if L.xfh_bench_sclk(ctx.h, 4096, capi.C.byref(sclk), capi.C.byref(spread)) == 0:
        clock = f"{sclk.value:.0f} MHz shader clock under f32 MFMA load, read by xfh_bench_sclk just before the runs ({spread.value:.0f} cycles per MFMA)"

    def kernel_us(fn, kid):
        for _ in range(a.warmup):
            fn()
        ctx.synchronize()
        ctx.timing_enable(capi.K[kid])
        for _ in range(a.iters):
            fn()
        ctx.synchronize()
        n, ms = ctx.timing_read()
        ctx.timing_enable(capi.K["NONE"])
        return ms * 1e3 / max(n, 1) if n else 0.0

    lines = [f"Box: {socket.gethostname()} ({L.xfh_version().decode()}); clock state: {clock}; nothing else of this process on the GPU.", "",
             f"Frame form, nn_ratio 0.7, th_low 100, init_dist 256, {a.iters} calls after {a.warmup} warm-up calls, back to back on one stream (the inputs stay in L2 / "
             "Infinity Cache between calls: a warm-cache figure).", "",
             "| nfeatures | members per node | B | shared | matches | queries resolved | full re-searches | k_bow_candidates, us per launch | k_bow_resolve, us per launch | "
             "B separate calls, us (both kernels, summed) | per problem in the one call, us |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for nf in (1000, 4096):
        for per_node in (10, 40):
            rng = np.random.RandomState(nf + per_node)
            base = base_keyframe(rng, nf, per_node)
            der = [derived(rng, base, per_node) for _ in range(BMAX)]
            sb, sd = BR.BowRig.side([base], "flag"), BR.BowRig.side(der, "flag")
            up = lambda x: capi.DeviceBuffer(max(np.ascontiguousarray(x).nbytes, 16)).upload(x)
            db = {k: up(sb[k]) for k in ("blob", "flag", "desc")}; dd = {k: up(sd[k]) for k in ("blob", "flag", "desc")}
            out = capi.DeviceBuffer(Context.bow_search_layout(BMAX, nf, nf)["bytes"])
            ws = capi.DeviceBuffer(Context.bow_search_workspace_bytes(nf, nf, BMAX))
            nb = Context.nodes_bytes(nf)
            at = lambda d, s, first: (d["blob"].ptr + first * nb, d["flag"].ptr + first * nf, d["desc"].ptr + first * s["stride"], s["stride"])

            def call(B, shared, first=0):
                """shared 1: the base is side 1; otherwise the derived keyframes are side 1 and the base is side 2"""
                s1 = at(db, sb, 0) if shared == 1 else at(dd, sd, first)
                s2 = at(dd, sd, first) if shared == 1 else at(db, sb, 0)
                ctx.bow_search_device(B, nf, nf, shared, s1[0], s1[1], s1[2], s1[3], s2[0], None, s2[2], s2[3], ws.ptr, out.ptr, nn_ratio=0.7)

            for B, shared in ((1, 0), (10, 2), (20, 1)):
                t = [kernel_us(lambda: call(B, shared), kid) for kid in KERNELS]
                lay = Context.bow_search_layout(B, nf, nf)
                ctx.synchronize()
                nm = int(out.download(np.int32, B, lay["n_matches"]).sum())
                cnt = ws.download(np.int32, 4 * B).reshape(B, 4).astype(np.int64).sum(0)
                sep = sum(kernel_us(lambda b=b: call(1, 0 if shared != 1 else 1, b), kid) for b in range(B) for kid in KERNELS)
                lines.append(f"| {nf} | {per_node} | {B} | {shared} | {nm} | {int(cnt[1])} | {int(cnt[0])} | {t[0]:.1f} | {t[1]:.1f} | {sep:.1f} | {(t[0] + t[1]) / B:.2f} |")
                print(lines[-1], flush=True)
            for x in list(db.values()) + list(dd.values()) + [out, ws]:
                x.free()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    print(text)
    ctx.close()


if __name__ == "__main__":
    main()
