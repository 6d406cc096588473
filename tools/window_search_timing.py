#!/usr/bin/env python
"""Device time of the windowed search, new route against the route the library offered before it (profiles/window_search.md).

  new route    : xfh_grid_build_device + xfh_search_window_device (k_grid_build + k_search_window)
  earlier route: xfh_memcpy_h2d of the CSR offsets + indices that tests/ref_window.py built on the host + xfh_best2_csr_device
                 (k_best2_csr).  The host time to build the lists and the D2H of the keypoints are NOT counted, which favours it.

VGA bounds, 4096 slots (3500 valid + padding at (0, 0)), nq = 4096, r in {7, 15, 30, 100}, both grid flags.  The ctx runs on
a torch stream of this tool (xfh_set_stream; not the default stream, whose handle 0 would mean "the ctx's own stream" to
xfh_set_stream), so torch.cuda events on that stream bracket `--iters` back-to-back repetitions after a warm-up; the earlier route is
measured five times and its max - min is the margin the comparison allows.  Kernel-alone times: run this tool under
`rocprofv3 --kernel-trace --stats -- python tools/window_search_timing.py --iters 50` and read k_search_window / k_best2_csr.

    python tools/window_search_timing.py [--iters 200] [--out profiles/window_search_table.md]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_window as RW                                    # noqa: E402
from xfeatslam_amd import capi                             # noqa: E402
from xfeatslam_amd.extractor import Context                # noqa: E402

F = np.float32
BOUNDS = (0.0, 0.0, 640.0, 480.0)


def scene(nt=4096, n_valid=3500, nq=4096, seed=1):
    rng = np.random.RandomState(seed)
    k = np.zeros(nt, capi.KP_DTYPE)
    mono = n_valid // 2
    valid = RW.valid_slots(nt, n_valid, mono)
    k["x"][valid] = rng.randint(0, 640, n_valid); k["y"][valid] = rng.randint(0, 480, n_valid); k["size"][valid] = 1; k["angle"] = -1
    tg = np.zeros((nt, 64), F)
    d = rng.randn(n_valid, 64); tg[valid] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    src = np.nonzero(valid)[0][rng.randint(0, n_valid, nq)]
    q = tg[src] + 0.06 * rng.randn(nq, 64); q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)
    uv = np.stack([k["x"][src] + rng.uniform(-3, 3, nq), k["y"][src] + rng.uniform(-3, 3, nq)], 1).astype(F)
    return k, valid, (n_valid, mono), tg, q, uv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    L = capi.lib()
    ctx = Context(nfeatures=64, max_height=32, max_width=32)
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    capi.check(L.xfh_set_stream(ctx.h, stream.cuda_stream), ctx.h)
    k, valid, header, tg, q, uv = scene()
    nt, nq = len(k), len(q)
    up = lambda x: capi.DeviceBuffer(max(np.ascontiguousarray(x).nbytes, 16)).upload(x)
    dk, dt, dq = up(k), up(tg), up(q)
    dh = up(np.array([header[0], header[1], 0, 0], np.int32))
    grid = capi.DeviceBuffer(ctx.grid_bytes(nt)); out = capi.DeviceBuffer(20 * nq); duvr = capi.DeviceBuffer(12 * nq)
    gb = capi.GridBounds(*BOUNDS)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.iters):
            fn()
        e1.record(stream); e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters            # us per repetition

    o = [out.ptr + 4 * nq * j for j in range(5)]
    lines = ["| r | flags | candidates / query (mean, max) | new route us (grid + search) | grid us | search us | earlier route us, 5 runs (min .. max) | h2d us | k_best2_csr us | new <= earlier max |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for flags in (0, capi.GRID_SKIP_PADDING):
        rgrid = RW.build(k["x"], k["y"], BOUNDS, valid if flags else None)
        for r in (7.0, 15.0, 30.0, 100.0):
            uvr = np.concatenate([uv, np.full((nq, 1), r, F)], 1).astype(F)
            duvr.upload(uvr)
            off, ind = RW.csr(rgrid, k["x"], k["y"], uvr, BOUNDS)
            doff, dind = capi.DeviceBuffer(off.nbytes), capi.DeviceBuffer(max(ind.nbytes, 16))

            def build():
                capi.check(L.xfh_grid_build_device(ctx.h, dk.ptr, nt, dh.ptr, C.byref(gb), flags, grid.ptr), ctx.h)

            def search():
                capi.check(L.xfh_search_window_device(ctx.h, dq.ptr, duvr.ptr, nq, grid.ptr, dt.ptr, nt, None, None, None, 256, *o), ctx.h)

            def h2d():
                capi.check(L.xfh_memcpy_h2d(doff.ptr, off.ctypes.data, off.nbytes)); capi.check(L.xfh_memcpy_h2d(dind.ptr, ind.ctypes.data, ind.nbytes))

            def best2():
                capi.check(L.xfh_best2_csr_device(ctx.h, dq.ptr, nq, dt.ptr, nt, doff.ptr, dind.ptr, 256, *o[:4]), ctx.h)

            t_new = timed(lambda: (build(), search()))
            t_grid, t_search = timed(build), timed(search)
            h2d()
            olds = [timed(lambda: (h2d(), best2())) for _ in range(5)]
            t_h2d, t_b2 = timed(h2d), timed(best2)
            # same answers from both routes, checked once per point
            torch.cuda.synchronize()
            b2 = out.download(np.int32, 4 * nq).reshape(4, nq).copy()
            build(); search(); torch.cuda.synchronize()
            sw = out.download(np.int32, 5 * nq).reshape(5, nq)
            assert np.array_equal(sw[:4], b2) and np.array_equal(sw[4], np.diff(off))
            cnt = np.diff(off)
            lines.append(f"| {r:g} | {flags} | {cnt.mean():.1f}, {cnt.max()} | {t_new:.1f} | {t_grid:.1f} | {t_search:.1f} | {min(olds):.1f} .. {max(olds):.1f} | "
                         f"{t_h2d:.1f} | {t_b2:.1f} | {'yes' if t_new <= max(olds) else 'NO'} |")
            print(lines[-1], flush=True)
            doff.free(); dind.free()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    print(text)
    ctx.close()


if __name__ == "__main__":
    main()
