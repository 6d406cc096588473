#!/usr/bin/env python
"""Device time of xfh_triangulation_search_device (k_triangulation_search) -> profiles/triangulation_search.md.

A synthetic keyframe of nfeatures = 1000 and 4096 keypoints against B = 1, 10 and 20 neighbours of the same size (LocalMapping::
CreateNewMapPoints: 10 to 20 covisible neighbours), side1_shared = 1.  Keypoints are uniform over a VGA image, a third with depth, a tenth
with a map point; node ids are uniform over `nfeatures / 10` nodes (about ten members per node and keyframe, what a level-4 cut of a
10^6-word vocabulary gives), F12 and the epipole come from the two-view geometry of tests/triangulation_rig.py.  Descriptors are random unit
rows: the time does not depend on their values, every survivor of the geometry costs one 64-float distance.

  one launch   k_triangulation_search per launch from the library's dispatch-attached event timers (xfh_timing_enable / xfh_timing_read):
               the kernel's own begin .. end, what rocprofv3 --kernel-trace shows
  B calls      the same B problems as B separate B = 1 calls, the kernel times summed (launch gaps are not in either column)

There is no parent-commit baseline (the call is new) and no threshold: the file records what was measured, on which box and clock state.

    python tools/time_triangulation.py [--iters 200] [--out FILE.md]
"""
import argparse
import os
import socket
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import triangulation_rig as TR                             # noqa: E402
from xfeatslam_amd import capi                              # noqa: E402
from xfeatslam_amd.extractor import Context                 # noqa: E402

F = np.float32


def keyframe(rng, n):
    xy = np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)], 1).astype(F)
    ur = np.where(rng.rand(n) < 1 / 3, xy[:, 0] - F(40.0) / rng.uniform(1, 8, n).astype(F), -1).astype(F)
    ur[ur < 0] = -1
    return dict(node_of=rng.randint(0, max(n // 10, 1), n).astype(np.uint32), xy=xy, ur=ur, has=(rng.rand(n) < 0.1).astype(np.uint8), desc=TR.unit_rows(rng, n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = capi.lib()
    assert L.xfh_device_count() > 0, "time_triangulation.py needs a GPU"
    ctx = Context(nfeatures=1, max_height=32, max_width=32)
    BMAX = 20
    sclk = capi.C.c_double(0.0); spread = capi.C.c_double(0.0)
    clock = "not read"
    if L.xfh_bench_sclk(ctx.h, 4096, capi.C.byref(sclk), capi.C.byref(spread)) == 0:
        clock = f"{sclk.value:.0f} MHz shader clock under f32 MFMA load, read by xfh_bench_sclk just before the runs ({spread.value:.0f} cycles per MFMA)"

    def kernel_us(fn):
        for _ in range(a.warmup):
            fn()
        ctx.synchronize()
        ctx.timing_enable(capi.K["TRIANGULATION_SEARCH"])
        for _ in range(a.iters):
            fn()
        ctx.synchronize()
        n, ms = ctx.timing_read()
        ctx.timing_enable(capi.K["NONE"])
        return ms * 1e3 / max(n, 1) if n else 0.0

    lines = [f"Box: {socket.gethostname()} ({L.xfh_version().decode()}); clock state: {clock}; nothing else of this process on the GPU.", "",
             f"side1_shared = 1, default flags, th_low 100, {a.iters} launches after {a.warmup} warm-up launches, the launches back to back on one stream "
             "(inputs of 20 neighbours stay in L2 / Infinity Cache between launches: a warm-cache figure).", "",
             "| nfeatures | B | sum n_candidates | sum n_geom | matches | one launch, us | B separate calls, us (sum of kernel times) | per pair in the one launch, us |",
             "|---|---|---|---|---|---|---|---|"]
    for nf in (1000, 4096):
        rng = np.random.RandomState(nf)
        k1 = keyframe(rng, nf)
        k2 = [keyframe(rng, nf) for _ in range(BMAX)]
        geo = [TR.neighbour(7000 + b, *TR.keyframe1(7100), 0.0)[1:] for b in range(BMAX)]      # F12 and the epipole of BMAX seeded poses
        s1, s2 = TR.TriRig.side([k1]), TR.TriRig.side(k2)
        up = lambda x: capi.DeviceBuffer(max(np.ascontiguousarray(x).nbytes, 16)).upload(x)
        d1 = {k: up(s1[k]) for k in ("blob", "xy", "ur", "has", "desc")}; d2 = {k: up(s2[k]) for k in ("blob", "xy", "ur", "has", "desc")}
        dF, de = up(np.stack([g[0] for g in geo]).astype(F)), up(np.stack([g[1] for g in geo]).astype(F))
        out = capi.DeviceBuffer(Context.triangulation_search_layout(BMAX, nf)["bytes"])
        nb = Context.nodes_bytes(nf)

        def call(B, first=0):
            ctx.triangulation_search_device(B, nf, nf, True, d1["blob"].ptr, d1["xy"].ptr, d1["ur"].ptr, d1["has"].ptr, d1["desc"].ptr, s1["stride"],
                                            d2["blob"].ptr + first * nb, d2["xy"].ptr + first * 8 * nf, d2["ur"].ptr + first * 4 * nf, d2["has"].ptr + first * nf,
                                            d2["desc"].ptr + first * s2["stride"], s2["stride"], dF.ptr + 36 * first, de.ptr + 8 * first, out.ptr)

        for B in (1, 10, 20):
            t = kernel_us(lambda: call(B))
            lay = Context.triangulation_search_layout(B, nf)
            ctx.synchronize()
            nc = int(out.download(np.int32, B * nf, lay["n_candidates"]).astype(np.int64).sum()); ng = int(out.download(np.int32, B * nf, lay["n_geom"]).astype(np.int64).sum())
            nm = int(out.download(np.int32, B, lay["n_matches"]).sum())
            sep = sum(kernel_us(lambda b=b: call(1, b)) for b in range(B))
            lines.append(f"| {nf} | {B} | {nc} | {ng} | {nm} | {t:.1f} | {sep:.1f} | {t / B:.2f} |")
            print(lines[-1], flush=True)
        for x in list(d1.values()) + list(d2.values()) + [dF, de, out]:
            x.free()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    print(text)
    ctx.close()


if __name__ == "__main__":
    main()
