#!/usr/bin/env python
"""single-frame latency of the host-pointer API (what XFextractor::operator() costs a SLAM thread)

    python tools/latency_check.py [--paced]
    python tools/latency_check.py --host-forms [--calls 20]      wall time per call of the seven host-pointer matcher / search forms at
                                                                 nfeatures 4096, one JSON line {form: median us}; $XFEAT_HIP_LIB names another
                                                                 build of the library to measure (profiles/host_forms.md)
"""
import ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from xfeatslam_amd import capi, synth, weights as WT
from xfeatslam_amd.extractor import Context, XFextractor


def host_forms(calls):
    nf, rng = 4096, np.random.RandomState(1)
    ctx = Context(nfeatures=nf, max_height=64, max_width=64)
    d1, d2 = synth.descriptor_sets(nf, nf, noise=0.3)
    k = np.zeros(nf, capi.KP_DTYPE); k["x"] = rng.uniform(0, 639, nf); k["y"] = rng.uniform(0, 479, nf); k["size"] = 1
    src = rng.randint(0, nf, nf)
    uvr = np.stack([k["x"][src], k["y"][src], np.full(nf, 15.0)], 1).astype(np.float32)
    off = (np.arange(nf + 1) * 64).astype(np.int32); ind = rng.randint(0, nf, nf * 64).astype(np.int32)                # bench.py's aux legs
    off2 = (np.arange(nf + 1) * 16).astype(np.int32); ind2 = rng.randint(0, nf, nf * 16).astype(np.int32)
    cam = capi.Camera(fx=517.3, fy=516.5, cx=318.6, cy=255.3, k1=0.2624, k2=-0.9531, p1=-0.0054, p2=0.0026, k3=1.1633, bf=40.0, width=640, height=480)
    depth = rng.randint(0, 30000, (480, 640)).astype(np.uint16)
    bounds, flags = (0.0, 0.0, 640.0, 480.0), np.full(nf, 3, np.uint8)
    forms = {
        "xfh_match_mnn 4096x4096": lambda: ctx.match_mnn(d1, d2),
        "xfh_distance_i32 4096x4096": lambda: ctx.distance_i32(d1, d2),
        "xfh_best2_csr 4096 queries x 64 candidates": lambda: ctx.best2_csr(d1, d2, off, ind),
        "xfh_search_window 4096x4096, r 15": lambda: ctx.search_window(d1[src], uvr, k, bounds, d2),
        "xfh_frame_finish 4096 keypoints, VGA uint16 depth": lambda: ctx.frame_finish(k, cam, depth, 1.0 / 5000.0),
        "xfh_search_projection 4096x4096, given, r 15": lambda: ctx.search_projection(capi.PROJ_GIVEN, uvr, d1[src], flags, k, bounds, d2, nn_ratio=0.9),
        "xfh_distinctive_csr 4096 groups x 16 rows": lambda: ctx.distinctive_csr(d1, off2, ind2),
    }
    res = {}
    for name, fn in forms.items():
        for _ in range(3):
            fn()
        ts = []
        for _ in range(calls):
            t = time.perf_counter(); fn(); ts.append(time.perf_counter() - t)
        res[name] = float(np.median(ts) * 1e6)
    ctx.close()
    print(json.dumps(res), flush=True)


if "--host-forms" in sys.argv:
    host_forms(int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 20)
    sys.exit(0)
blob = WT.pack_blob(WT.make_synthetic(1234, 6.0))
for (H, W, nf) in [(480, 640, 1000), (480, 640, 4096), (720, 1280, 2000)]:
    ex = XFextractor(nf, 1.2, 8, 20, 7, weights=blob, max_height=H, max_width=W)
    img = synth.image(H, W, 42)
    for _ in range(5): ex(img)
    ts = []
    for _ in range(50):
        t = time.perf_counter(); ex(img); ts.append(time.perf_counter() - t)
    if "--paced" in sys.argv:                     # one call every 33 ms, as a 30-Hz SLAM loop would: the GPU idles (and clocks down) between frames
        tp = []
        for _ in range(40):
            time.sleep(0.033); t = time.perf_counter(); ex(img); tp.append(time.perf_counter() - t)
        tp = np.array(tp) * 1e3
        print(f"{H}x{W} nfeatures {nf}: one call every 33 ms: median {np.median(tp):.3f} ms  min {tp.min():.3f}  p90 {np.percentile(tp, 90):.3f}", flush=True)
    ts = np.array(ts) * 1e3
    print(f"{H}x{W} nfeatures {nf}: xfh_extract median {np.median(ts):.3f} ms  min {ts.min():.3f}  p90 {np.percentile(ts, 90):.3f}  (n_valid {ex.n_valid})", flush=True)
    d1 = np.zeros((nf, 64), np.float32)
    ret, k, d = ex(img)
    ts = []
    for _ in range(30):
        t = time.perf_counter(); ex.ctx.match_mnn(d, d); ts.append(time.perf_counter() - t)
    print(f"   xfh_match_mnn {nf}x{nf} host API median {np.median(np.array(ts)) * 1e3:.3f} ms", flush=True)
    ex.ctx.close()
