#!/usr/bin/env python
"""Device time of xfh_bow_transform_device (k_vocab_descend, k_vocab_finish) -> profiles/bow_transform.md.

Frames of n = 4096 rows of random bits (every row takes its own path down the tree), B = 1, 8 and 64 frames per call, levelsup = 4, on two
synthetic vocabularies with random descriptor bytes and random positive weights:
  ORBvoc shape   k = 10, L = 6: 1 111 111 nodes, 35.6 MB of descriptors, a blob of 62 MB (the real ORBvoc.txt is not needed for a time: the
                 walk depends on the shape of the tree, not on what it was trained on)
  small          k = 10, L = 3: 1111 nodes, a blob of 62 KB that stays in L2 (the vocabulary of the tests)
64 different frames are kept in device memory and successive calls take successive frames, so a call does not walk the paths the call before
it has just pulled into the caches.

  per kernel     us per launch from the library's dispatch-attached event timers (xfh_timing_enable / xfh_timing_read): the kernel's own
                 begin .. end, what rocprofv3 --kernel-trace shows
  per call       host clock around `iters` calls that end in one synchronise, over iters: both kernels and the launch gaps
  gathered       the bytes the descent must read per frame, n * L * k * 32 (every level reads the k descriptors of one node), over the time
                 of k_vocab_descend: a rate of USEFUL bytes, not a memory-traffic measurement

There is no parent-commit baseline (the call is new) and no threshold.  The host path this call replaces -- the download of the descriptors,
DBoW2's transform on the CPU, xfh_nodes_pack and the upload of the blob -- cannot be built here without OpenCV: no speed-up over it is
claimed.

    python tools/time_vocab.py [--iters 100] [--out FILE.md]
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
KERNELS = ("VOCAB_DESCEND", "VOCAB_FINISH")
N, FRAMES = 4096, 64


def regular_vocabulary(k, L, seed):
    rng = np.random.RandomState(seed)
    n = (k ** (L + 1) - 1) // (k - 1)
    parent = np.zeros(n, np.uint32); parent[1:] = (np.arange(1, n, dtype=np.int64) - 1) // k
    first_leaf = (k ** L - 1) // (k - 1)
    word = np.zeros(n, np.uint32); word[first_leaf:] = np.arange(n - first_leaf, dtype=np.uint32)
    weight = np.zeros(n, np.float64); weight[first_leaf:] = rng.uniform(0.05, 9.0, n - first_leaf)
    desc = rng.randint(0, 256, (n, 32), dtype=np.uint8)
    return Context.vocab_pack(parent, word, weight, desc, L)[0], n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = capi.lib()
    assert L.xfh_device_count() > 0, "time_vocab.py needs a GPU"
    ctx = Context(nfeatures=1, max_height=32, max_width=32)
    sclk = capi.C.c_double(0.0); spread = capi.C.c_double(0.0)
    clock = "not read"
    if L.xfh_bench_sclk(ctx.h, 4096, capi.C.byref(sclk), capi.C.byref(spread)) == 0:
        clock = f"{sclk.value:.0f} MHz shader clock under f32 MFMA load, read by xfh_bench_sclk just before the runs ({spread.value:.0f} cycles per MFMA)"
    rng = np.random.RandomState(77)
    stride = N * 256
    rows = capi.DeviceBuffer(2 * FRAMES * stride).upload(np.frombuffer(rng.bytes(2 * FRAMES * stride), np.uint8))
    out = capi.DeviceBuffer(Context.bow_transform_layout(FRAMES, N)["bytes"])
    ws = capi.DeviceBuffer(Context.bow_transform_workspace_bytes(N, FRAMES))
    lines = [f"Box: {socket.gethostname()} ({L.xfh_version().decode()}); clock state: {clock}; nothing else of this process on the GPU.", "",
             f"n = {N} rows per frame, levelsup 4, {a.iters} calls after {a.warmup} warm-up calls, back to back on one stream; successive calls take successive "
             f"frames of {FRAMES} kept in device memory.", "",
             "| vocabulary | nodes | blob, MB | B | k_vocab_descend, us per launch | k_vocab_finish, us per launch | both, us per frame | per call (host clock), us | "
             "gathered per frame, MB | useful gather rate of k_vocab_descend, GB/s | words per frame |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for label, k, depth in (("ORBvoc shape (k = 10, L = 6)", 10, 6), ("small (k = 10, L = 3)", 10, 3)):
        blob, nn = regular_vocabulary(k, depth, 1000 + depth)
        nb = Context.vocab_bytes(nn)
        dv = capi.DeviceBuffer(nb).upload(blob[:nb])
        turn = [0]

        def call(B):
            first = turn[0] % FRAMES                       # (the buffer holds 2 * FRAMES frames: a call of B <= FRAMES never runs off its end)
            turn[0] += B
            ctx.bow_transform_device(B, N, dv.ptr, nb, rows.ptr + first * stride, stride, ws.ptr, out.ptr, levelsup=4)

        def kernel_us(B, kid):
            for _ in range(a.warmup):
                call(B)
            ctx.synchronize()
            ctx.timing_enable(capi.K[kid])
            for _ in range(a.iters):
                call(B)
            ctx.synchronize()
            n, ms = ctx.timing_read()
            ctx.timing_enable(capi.K["NONE"])
            return ms * 1e3 / max(n, 1) if n else 0.0

        for B in (1, 8, 64):
            t = [kernel_us(B, kid) for kid in KERNELS]
            for _ in range(a.warmup):
                call(B)
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                call(B)
            ctx.synchronize()
            wall = (time.perf_counter() - t0) * 1e6 / a.iters
            lay = Context.bow_transform_layout(B, N)
            nw = out.download(np.int32, B, lay["n_words"])
            gather = N * depth * k * 32
            lines.append(f"| {label} | {nn} | {nb / 1e6:.1f} | {B} | {t[0]:.1f} | {t[1]:.1f} | {(t[0] + t[1]) / B:.1f} | {wall:.1f} | {gather / 1e6:.2f} | "
                         f"{B * gather / max(t[0], 1e-9) / 1e3:.0f} | {float(nw.mean()):.0f} |")
            print(lines[-1], flush=True)
        dv.free()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    print(text)
    for x in (rows, out, ws):
        x.free()
    ctx.close()


if __name__ == "__main__":
    main()
