#!/usr/bin/env python
"""Device time of xfh_essential_graph_device (essgraph.hip.h) -> profiles/essential_graph.md: per call and per kernel family at 16, 128 and 192 (the limit) free
keyframes on a chain-plus-covisibility graph with one loop, the header of each run, the relative residual of the blocked solver at each size, and the
blocked LDL^T against k_lba_solve at n = 768 in alternating rounds of one session.

  kernel     us per call in each kernel family, from the library's dispatch-attached event timers (xfh_timing_enable / xfh_timing_read): the sum over the
             family's launches of one call
  per call   host clock around one call (the call is synchronous)
  residual   |(H + lambda I) x - b| / |b| of the FIRST solve of the run, an accepted one at lambda = 1e-16: a second call with max_iterations = 1 leaves the
             edge records (both Jacobians), the vertex sums (diagonal blocks, b) and x in the workspace, from which H is rebuilt here with numpy (S itself
             is factorised in place); and |S x - b| / |b| of xfh_debug_eg_solve on a well-conditioned SPD system of the same size, for comparison
  registers  read from clang's -Rpass-analysis=kernel-resource-usage remarks for kernels_essgraph.hip when the profile is written

These are records, not thresholds.  There is no parent-commit baseline (the call is new).  The host code it replaces -- the reference's g2o -- cannot be
built and timed here, so no ratio against it is measured or claimed.

    python tools/time_essential_graph.py [--sizes 16,128,192] [--rounds 4] [--bench "figure"] [--out FILE.md]
"""
import argparse
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import essential_graph_rig as G                              # noqa: E402
from xfeatslam_amd import capi, essential_graph as EG       # noqa: E402

FAMILIES = ("EG_PLAN", "EG_LINEARIZE", "EG_FILL", "EG_FACTOR", "EG_SUBST", "EG_EVALUATE", "EG_FINISH")
D = np.float64


def timed(ctx, family, fn):
    ctx.timing_enable(capi.K[family])
    fn()
    ctx.synchronize()
    cnt, ms = ctx.timing_read()
    ctx.timing_enable(capi.K["NONE"])
    return ms * 1e3, cnt


def debug_solve(L, ctx, fn, n, S, b, extra=()):
    S, x, flag = S.copy(), np.zeros(n, D), np.zeros(1, np.int32)
    rc = getattr(L, fn)(ctx.h, n, S.ctypes.data, b.ctypes.data, x.ctypes.data, *extra, flag.ctypes.data)
    assert rc == 0 and flag[0] == 1, (fn, rc, flag)
    return x


def resources():
    """-> 'k_eg_x N VGPRs / M bytes of LDS, ..' from the compiler's remarks for kernels_essgraph.hip, scratch and AGPR use named when there is any"""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return "not read (no hipcc where the profile was written)"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(ROOT, "xfeatslam_amd", "csrc", "kernels_essgraph.hip"), "-o", os.devnull], capture_output=True, text=True, timeout=600)
    field = lambda key: re.findall(key + r": (\S+)", r.stderr)
    names, vgpr, agpr, scratch, lds = field("Function Name"), field(r"    VGPRs"), field("AGPRs"), field(r"ScratchSize \[bytes/lane\]"), field(r"LDS Size \[bytes/block\]")
    assert names and len(names) == len(vgpr) == len(agpr) == len(scratch) == len(lds), r.stderr[-2000:]
    out = []
    for nm, v, a, sc, l in sorted(zip(names, vgpr, agpr, scratch, lds), key=lambda t: -int(t[1])):
        m = re.search(r"\d+(k_eg_[a-z_]+)(?:ILb([01])E)?", nm)
        label = m.group(1) + ("" if m.group(2) is None else "<true>" if m.group(2) == "1" else "<false>")
        out.append(f"`{label}` {v}" + (f" / {l} B LDS" if int(l) > 64 else "") + (f" / {sc} B scratch" if int(sc) else "") + (f" / {a} AGPRs" if int(a) else ""))
    return "VGPRs per kernel: " + ", ".join(out) + "; scratch and AGPRs are named where a kernel uses any"


def ws_offsets(nV, nE, n_free):
    """the arrays of the workspace as eg_ws (essgraph_math.h) lays them out; checked against the library's own size"""
    n, o, off = 7 * max(n_free, 1), 0, {}
    for name, size in (("ctl", 104), ("v_free", 4 * nV), ("free_v", 4 * EG.MAX_FREE), ("v_cnt", 4 * nV), ("v_lead", 4 * nV), ("v_loop", 4 * nV), ("v_begin", 4 * (nV + 1)),
                       ("v_edges", 8 * nE), ("edge_ok", 4 * nE), ("vScw", 64 * nV), ("Smw", 64 * nV), ("est", 128 * nV), ("sims", 29 * 64 * nV), ("meas", 64 * nE),
                       ("rec", 106 * 8 * nE), ("v_sum", 36 * 8 * nV), ("v_chi", 8 * nV), ("b", 8 * n), ("x", 8 * n), ("S", 8 * n * n)):
        off[name] = o
        o += (size + 255) & ~255
    assert o == EG.workspace_bytes(nV, nE, n_free), "the workspace layout of essgraph_math.h has changed"
    return off


def first_solve_residual(p, raw, nV, nE, n_free):
    """|(H + 1e-16 I) x - b| / |b| of the one solve of a max_iterations = 1 call, H rebuilt from the workspace bytes `raw` (everything in front of S)"""
    off, n = ws_offsets(nV, nE, n_free), 7 * n_free
    take = lambda name, dt, count: np.frombuffer(raw[off[name]:off[name] + count * np.dtype(dt).itemsize].tobytes(), dt)
    v_free, ok = take("v_free", np.int32, nV), take("edge_ok", np.int32, nE)
    rec, v_sum = take("rec", D, 106 * nE).reshape(nE, 106), take("v_sum", D, 36 * nV).reshape(nV, 36)
    b, x = take("b", D, n), take("x", D, n)
    H, iu = np.zeros((n, n), D), np.triu_indices(7)
    for v in range(nV):
        f = v_free[v]
        if f >= 0:
            blk = np.zeros((7, 7), D)
            blk[iu] = v_sum[v, :28]
            H[7 * f:7 * f + 7, 7 * f:7 * f + 7] = blk + np.triu(blk, 1).T
    for e in np.nonzero(ok)[0]:
        fi, fj = v_free[p["edge_i"][e]], v_free[p["edge_j"][e]]
        if fi >= 0 and fj >= 0:
            Ji, Jj = rec[e, 8:57].reshape(7, 7), rec[e, 57:106].reshape(7, 7)
            H[7 * fi:7 * fi + 7, 7 * fj:7 * fj + 7] += Ji.T @ Jj
            H[7 * fj:7 * fj + 7, 7 * fi:7 * fi + 7] += Jj.T @ Ji
    H[np.diag_indices(n)] += 1e-16
    ev = np.linalg.eigvalsh(H) if n <= 2048 else None
    return float(np.linalg.norm(H @ x - b) / np.linalg.norm(b)), (float(ev[-1] / ev[0]) if ev is not None else float("nan"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,128,192")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--bench", default="", help="the front end's figure of bench.py --gpus 1 --steps 20 --warmup 5, to be recorded")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "essential_graph.md"))
    a = ap.parse_args()
    L = capi.lib()
    assert L.xfh_device_count() > 0, "time_essential_graph.py needs a GPU"
    rig = G.EgRig(L)
    ctx = rig.ctx
    lines = ["# xfh_essential_graph_device: OptimizeEssentialGraph behind the Sim3 Fuse of loop closing", "",
             "Written by `tools/time_essential_graph.py`.  The host launches one step at a time and reads the control record back after every trial (`essgraph.hip.h`); a "
             "factorisation is 2 x ceil(7 n_free / 64) launches.  The reference's g2o cannot be built and timed here: no ratio against it is measured or claimed.", "",
             "Registers (`-Rpass-analysis=kernel-resource-usage` on `kernels_essgraph.hip`, read when this file was written).  " + resources() + ".", "",
             f"One MI355X ({L.xfh_version().decode()}); nothing else of this process on the GPU.  One call per figure after one warm-up call; a chain of n_free + 1 keyframes "
             "(the first fixed) with covisibility edges to the second neighbour, one loop connection, three corrected keyframes, bFixScale off, write_back off, optimize(20).", "",
             "| free | edges | header: iterations, trials, rejected, failures | per call (host clock), us | " + " | ".join("`k_%s`" % f.lower() for f in FAMILIES)
             + " | factorisation + substitution share | first solve: residual, cond(H) | solver alone on an SPD system of that size: residual |", "|" + "---|" * (7 + len(FAMILIES))]
    for n_free in [int(v) for v in a.sizes.split(",")]:
        p = G.make(8000 + n_free, n_free, covis=2, n_points=64)
        nV, nE, nP, nS = G.dims(p)
        arrays = EG.host_arrays(p)
        dev = [capi.DeviceBuffer(max(x.nbytes, 8)).upload(x) for x in arrays]
        lay = EG.essential_graph_layout(nV, nP, nE)
        out, ws = capi.DeviceBuffer(lay["bytes"]), capi.DeviceBuffer(EG.workspace_bytes(nV, nE, n_free))

        def call():
            EG.essential_graph_device(ctx, nV, n_free, nE, nP, nS, dev[0].ptr, len(arrays[0]), dev[1].ptr, len(arrays[1]), *[d.ptr for d in dev[2:]], ws.ptr, out.ptr, lay)
        call()
        t0 = time.perf_counter()
        call()
        wall = (time.perf_counter() - t0) * 1e6
        hdr = lay.parse(out.download(np.uint8, lay["bytes"]))["header"]
        fam = {f: timed(ctx, f, call) for f in FAMILIES}
        EG.essential_graph_device(ctx, nV, n_free, nE, nP, nS, dev[0].ptr, len(arrays[0]), dev[1].ptr, len(arrays[1]), *[d.ptr for d in dev[2:]], ws.ptr, out.ptr, lay,
                                  max_iterations=1)
        h1 = lay.parse(out.download(np.uint8, lay["bytes"]))["header"]
        res1, cond = first_solve_residual(p, ws.download(np.uint8, ws_offsets(nV, nE, n_free)["S"]), nV, nE, n_free)
        first = f"{res1:.2e}, {cond:.1e}" + ("" if h1[4:8].tolist() == [1, 1, 0, 0] else " (NOT accepted: header %s)" % h1[4:8].tolist())
        for d in dev + [out, ws]:
            d.free()
        n = 7 * n_free
        S, b = G.spd_system(n, n)
        x = debug_solve(L, ctx, "xfh_debug_eg_solve", n, S, b)
        res = float(np.linalg.norm(S @ x - b) / np.linalg.norm(b))
        total = sum(v[0] for v in fam.values())
        assert hdr[0] == 0, hdr
        lines.append(f"| {n_free} | {nE} | {hdr[4]}, {hdr[5]}, {hdr[6]}, {hdr[7]} | {wall:.0f} | " + " | ".join(f"{fam[f][0]:.0f} ({fam[f][1]})" for f in FAMILIES)
                     + f" | {(fam['EG_FACTOR'][0] + fam['EG_SUBST'][0]) / total:.2f} | {first} | {res:.2e} |")
        print(lines[-1], flush=True)
    lines += ["", "Kernel columns: us per call summed over the family's launches (their number per call in brackets).  `k_eg_linearize` is the BUILD step (`k_eg_sims<true>`, "
              "`k_eg_edges<true>`, `k_eg_vertices<true>`, `k_eg_begin`), `k_eg_evaluate` the rest of a trial (`k_eg_update`, `k_eg_sims<false>`, `k_eg_edges<false>`, "
              "`k_eg_vertices<false>`, `k_eg_decide`), `k_eg_factor` both LDL^T kernels.  The memset of S in front of `k_eg_fill` is in no family; the host clock includes it and "
              "the read-backs.  First solve: a further call with `max_iterations` = 1 (one trial, accepted, lambda = 1e-16) leaves the edge records, the vertex sums, b and x in the workspace; H is "
              "rebuilt from them on the host and the column is |(H + lambda I) x - b| / |b| with the condition number of H (not computed above 2048 unknowns).  The last column is "
              "`xfh_debug_eg_solve` on a well-conditioned SPD system of 7 x free unknowns made on the host.", ""]
    # the blocked solver against the one-workgroup solver of LocalBundleAdjustment, alternating in one session
    n = 768
    S, b = G.spd_system(n, 768)
    rounds = []
    for _ in range(a.rounds):
        new = timed(ctx, "EG_FACTOR", lambda: debug_solve(L, ctx, "xfh_debug_eg_solve", n, S, b))[0] + timed(ctx, "EG_SUBST", lambda: debug_solve(L, ctx, "xfh_debug_eg_solve", n, S, b))[0]
        old = timed(ctx, "LBA_SOLVE", lambda: debug_solve(L, ctx, "xfh_debug_lba_solve", n, S, b, (0x3C,)))[0]
        rounds.append((new, old))
    x_new, x_old = debug_solve(L, ctx, "xfh_debug_eg_solve", n, S, b), debug_solve(L, ctx, "xfh_debug_lba_solve", n, S, b, (0x3C,))
    lines += ["## The blocked LDL^T against `k_lba_solve` at n = 768", "",
              f"The same system through `xfh_debug_eg_solve` (24 launches of `k_eg_ldlt_*` and `k_eg_subst`) and `xfh_debug_lba_solve` (`k_lba_solve`, one workgroup), alternating, "
              f"{a.rounds} rounds in one session, kernel time from the event timers; the two solutions have {'the same bits' if x_new.tobytes() == x_old.tobytes() else 'DIFFERENT bits'}.", "",
              "| round | blocked (`k_eg_factor` + `k_eg_subst`), us | `k_lba_solve`, us | ratio |", "|---|---|---|---|"]
    for i, (new, old) in enumerate(rounds):
        lines.append(f"| {i + 1} | {new:.0f} | {old:.0f} | {old / new:.1f} |")
    med = lambda v: float(np.median(v))
    below = med([r[0] for r in rounds]) < med([r[1] for r in rounds])
    lines += ["", f"Median: blocked {med([r[0] for r in rounds]):.0f} us, `k_lba_solve` {med([r[1] for r in rounds]):.0f} us: the blocked form is "
              + ("below the existing kernel." if below else "NOT below the existing kernel.") + "  `xfh_local_ba_device` is not switched to it here.", ""]
    if a.bench:
        lines += ["## The front end", "", "`bench.py --gpus 1 --steps 20 --warmup 5` with this library (a translation unit more, no front-end kernel touched): " + a.bench,
                  "", "The figure on record for the tree before it is the one `profiles/local_ba.md` closes with (31624 frames/s, 8.10 ms per step).  A run of the parent's library in "
                  "the same session was not possible: this tree's bindings ask every library for the new symbols.", ""]
    rig.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
