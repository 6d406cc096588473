#!/usr/bin/env python
"""Device time of xfh_bowdb_query_device (k_bowdb_score, k_bowdb_select) -> profiles/bow_database.md.

Databases of n_slots = 256, 1024, 4096 and 8192 keyframes with about 1000 words per BowVector (stride 1024; every vector draws its words from a
universe of 20 000, so two vectors share about 50 words and every slot is listed), ten covisibility neighbours per keyframe, a random
insertion order (d_seq), B = 1 and 8 queries per call, both forms.  Successive calls take successive queries of 16 kept in device memory.

  per kernel     us per launch from the library's dispatch-attached event timers (xfh_timing_enable / xfh_timing_read): the kernel's own
                 begin .. end, what rocprofv3 --kernel-trace shows
  per call       host clock around `iters` calls that end in one synchronise, over iters: both kernels and the launch gap
  scanned        the bytes of database ids one query must read, the words of all slots * 4 (values are fetched on a hit only), over the time
                 of k_bowdb_score: a rate of USEFUL bytes, not a memory-traffic measurement

There is no parent-commit baseline (the call is new) and no threshold.  The dense scan reads the whole database per query; the host's inverted
file touches only the shared postings.  That host walk was NOT timed: whether the scan wins at a given database size is not measured here.

    python tools/time_bowdb.py [--iters 100] [--out FILE.md]
"""
import argparse
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from xfeatslam_amd import capi                              # noqa: E402
from xfeatslam_amd.extractor import Context                 # noqa: E402

F = np.float32
KERNELS = ("BOWDB_SCORE", "BOWDB_SELECT")
STRIDE, UNIVERSE, QUERIES, NN = 1024, 20000, 16, 10


def vectors(rng, count):
    ids, vals, nw = np.full((count, STRIDE), 0xFFFFFFFF, np.uint32), np.zeros((count, STRIDE), np.float64), np.zeros(count, np.int32)
    for s in range(count):
        k = int(rng.randint(960, STRIDE + 1))
        v = rng.rand(k) + 0.01
        ids[s, :k], vals[s, :k], nw[s] = np.sort(rng.choice(UNIVERSE, k, replace=False)), v / v.sum(), k
    return ids, vals, nw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = capi.lib()
    assert L.xfh_device_count() > 0, "time_bowdb.py needs a GPU"
    ctx = Context(nfeatures=1, max_height=32, max_width=32)
    sclk = capi.C.c_double(0.0); spread = capi.C.c_double(0.0)
    clock = "not read"
    if L.xfh_bench_sclk(ctx.h, 4096, capi.C.byref(sclk), capi.C.byref(spread)) == 0:
        clock = f"{sclk.value:.0f} MHz shader clock under f32 MFMA load, read by xfh_bench_sclk just before the runs ({spread.value:.0f} cycles per MFMA)"
    rng = np.random.RandomState(91)
    up = lambda x: capi.DeviceBuffer(x.nbytes + 16).upload(x)
    qi, qv, qn = vectors(rng, 2 * QUERIES)
    dqi, dqv, dqn = up(qi), up(qv), up(qn)
    lines = [f"Box: {socket.gethostname()} ({L.xfh_version().decode()}); clock state: {clock}; nothing else of this process on the GPU.", "",
             f"stride {STRIDE}, 960 .. {STRIDE} words per vector from a universe of {UNIVERSE}, {NN} neighbours per slot, d_seq a permutation, {a.iters} calls after "
             f"{a.warmup} warm-up calls, back to back on one stream; successive calls take successive queries of {QUERIES} kept in device memory.", "",
             "| n_slots | form | B | k_bowdb_score, us per launch | k_bowdb_select, us per launch | both, us per query | per call (host clock), us | "
             "scanned ids per query, MB | useful scan rate of k_bowdb_score, GB/s | listed | scored | candidates |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for n in (256, 1024, 4096, 8192):
        ids, vals, nw = vectors(rng, n)
        d_ids, d_vals, d_nw = up(ids), up(vals), up(nw)
        d_seq = up(rng.permutation(n).astype(np.uint32))
        d_neigh = up(rng.randint(0, n, (n, NN)).astype(np.int32))
        for form, fname in ((capi.BOWDB_FORM_RELOC, "RELOC"), (capi.BOWDB_FORM_NBEST, "NBEST")):
            for B in (1, 8):
                lay = Context.bowdb_query_layout(B, n)
                out = capi.DeviceBuffer(lay["bytes"])
                ws = capi.DeviceBuffer(Context.bowdb_query_workspace_bytes(n, B))
                state = up(np.zeros((B, n), F))
                turn = [0]

                def call():
                    first = turn[0] % QUERIES              # (the buffer holds 2 * QUERIES queries: a call of B <= QUERIES never runs off its end)
                    turn[0] += B
                    ctx.bowdb_query_device(B, n, form, dqi.ptr + 4 * first * STRIDE, dqv.ptr + 8 * first * STRIDE, dqn.ptr + 4 * first, STRIDE, d_ids.ptr, d_vals.ptr,
                                           d_nw.ptr, STRIDE, d_seq.ptr, d_neigh.ptr, NN, None, state.ptr, ws.ptr, out.ptr)

                def kernel_us(kid):
                    for _ in range(a.warmup):
                        call()
                    ctx.synchronize()
                    ctx.timing_enable(capi.K[kid])
                    for _ in range(a.iters):
                        call()
                    ctx.synchronize()
                    cnt, ms = ctx.timing_read()
                    ctx.timing_enable(capi.K["NONE"])
                    return ms * 1e3 / max(cnt, 1) if cnt else 0.0

                t = [kernel_us(kid) for kid in KERNELS]
                for _ in range(a.warmup):
                    call()
                ctx.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.iters):
                    call()
                ctx.synchronize()
                wall = (time.perf_counter() - t0) * 1e6 / a.iters
                res = Context.bowdb_query_parse(out.download(np.uint8, lay["bytes"]), lay, B, n)
                scan = int(nw.sum()) * 4
                lines.append(f"| {n} | {fname} | {B} | {t[0]:.1f} | {t[1]:.1f} | {(t[0] + t[1]) / B:.1f} | {wall:.1f} | {scan / 1e6:.2f} | "
                             f"{B * scan / max(t[0], 1e-9) / 1e3:.0f} | {np.mean([r['n_listed'] for r in res]):.0f} | {np.mean([r['n_scored'] for r in res]):.0f} | "
                             f"{np.mean([r['n_candidates'] for r in res]):.0f} |")
                print(lines[-1], flush=True)
                for x in (out, ws, state):
                    x.free()
        for x in (d_ids, d_vals, d_nw, d_seq, d_neigh):
            x.free()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    print(text)
    for x in (dqi, dqv, dqn):
        x.free()
    ctx.close()


if __name__ == "__main__":
    main()
