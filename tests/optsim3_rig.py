"""Seeded scenes for xfh_sim3_optimize_device and its restatements (tests/ref_optsim3.py, tests/ref_optsim3_literal.py): two keyframes that see
common points through a known similarity S12 (P3D1c = S12.map(P3D2c)), observations = the projections + noise, a perturbed start.  SCENES is the
table whose condition tests/test_optsim3_ref.py::test_rig_condition measures on the CPU and which the GPU tests compare under SIM3OPT_TOL;
run_host() runs problems through xfh_sim3_optimize_host, Sim3OptRig on the device with outputs and workspace between guard bytes."""
import ctypes as C
import functools

import numpy as np

import guarded
import ref_optsim3 as R
import ref_optsim3_literal as RL
import ref_poseopt as RP
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context

F, D = np.float32, np.float64
CAM = (517.3, 516.5, 318.6, 255.3)                                      # fx, fy, cx, cy (TUM1-like)
TH2 = 10.0                                                              # LoopClosing.cc:767
GUARD = 256


def _pose(rng, rot, tr):
    p = RP.oplus(np.r_[rng.uniform(-rot, rot, 3), rng.uniform(-tr, tr, 3)], [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
    return RP.to_tcw(p)


def _to_world(T, Pc):
    T = np.asarray(T, D).reshape(3, 4)
    return ((Pc - T[:, 3]) @ T[:, :3]).astype(F)                        # R^T (Pc - t)


def make(seed, n_pairs, n1, fix_scale=0, all_points=0, outliers=0, not_in_kf2=0, bad2=0, null1=0, null_assigned=0, behind=0, nan_z=0, noise=0.5,
         start=(0.01, 0.03, 0.02), pin=None, spare=4, out_px=(30, 90), w=(1.0, 1.0)):
    """-> a problem dict.  n_pairs good correspondences in KF2, then `outliers` more with a gross observation error, `not_in_kf2` more whose point is
    not in KF2 (an edge pair only with all_points), and keypoints that look matched but have no edge: bad2 (flag byte 0), null1 (point1 outside its
    range), null_assigned (assigned beyond nq), behind (z < 0 in camera 2), nan_z.  start = size of the perturbation (rotation, translation, log
    scale).  pin: keypoint numbers that carry a good pair whatever the seed.  w = (inv_sigma2_1, inv_sigma2_2), drawn from nothing: the scene is the same."""
    rng = np.random.RandomState(seed)
    fx, fy, cx, cy = CAM
    n_edge = n_pairs + outliers + not_in_kf2
    n_all = n_edge + bad2 + null1 + null_assigned + behind + nan_z
    assert n_all <= n1
    nq, M1, n2 = n_all + spare, n_all + spare, n_all + spare
    s_true = 1.0 if fix_scale else float(rng.uniform(0.85, 1.2))
    true = R.oplus(np.r_[rng.uniform(-0.1, 0.1, 3), rng.uniform(-0.3, 0.3, 3), 0.0], [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, s_true], 1)
    z = rng.uniform(2.5, 9.0, nq)
    u, v = rng.uniform(120, 520, nq), rng.uniform(100, 380, nq)
    P2c = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
    P1c = np.stack(R.smap(true, [P2c[:, 0], P2c[:, 1], P2c[:, 2]]), 1)
    T1w, T2w, Tmw = _pose(rng, 0.3, 1.0), _pose(rng, 0.3, 1.0), _pose(rng, 0.3, 1.0)
    # the slots
    if pin:
        pinned = np.array(sorted(pin))
        assert len(pinned) <= n_pairs and pinned[0] >= 0 and pinned[-1] < n1
        rest = rng.choice(np.setdiff1d(np.arange(n1), pinned), n_all - len(pinned), replace=False)
        slots = np.r_[pinned, rng.permutation(rest)]                     # the first n_pairs slots are the good pairs
    else:
        slots = rng.permutation(rng.choice(n1, n_all, replace=False))
    q = rng.permutation(nq)[:n_all]                                      # row in points2 of each slot
    m = rng.permutation(M1)[:n_all]                                      # row in points1
    k2 = rng.permutation(n2)[:n_all]                                     # keypoint in KF2
    kind = np.repeat(np.arange(8), [n_pairs, outliers, not_in_kf2, bad2, null1, null_assigned, behind, nan_z])
    if kind.size and (kind == 6).any():
        b = q[kind == 6]
        P2c[b] *= -1.0                                                   # behind camera 2 (P3D1c does not matter: no edge)
    points2 = np.zeros((nq, 3), F)
    points2[:] = _to_world(T2w, P2c)
    points1 = np.zeros((M1, 3), F)
    points1[m] = _to_world(T1w, P1c[q])
    points1[np.setdiff1d(np.arange(M1), m)] = rng.uniform(-3, 3, (M1 - n_all, 3))
    points2[q[kind == 7]] = np.nan
    assigned = np.full(n1, -1, np.int32)
    assigned[slots] = q
    assigned[slots[kind == 5]] = nq + rng.randint(0, 3, int((kind == 5).sum()))
    point1 = rng.randint(-3, 0, n1).astype(np.int32)
    point1[slots] = m
    point1[slots[kind == 4]] = np.where(rng.rand(int((kind == 4).sum())) < 0.5, -1, M1 + 2)
    flags2 = np.ones(nq, np.uint8)
    flags2[q[kind == 3]] = rng.choice([0, 2, 254], int((kind == 3).sum()))
    index2 = np.full(nq, -1, np.int32)
    index2[q] = k2
    index2[q[kind == 2]] = -1
    xy1, xy2 = rng.uniform(0, 640, (n1, 2)), rng.uniform(0, 640, (n2, 2))
    pu1, pv1 = fx * P1c[q, 0] / P1c[q, 2] + cx, fy * P1c[q, 1] / P1c[q, 2] + cy
    pu2, pv2 = fx * P2c[q, 0] / P2c[q, 2] + cx, fy * P2c[q, 1] / P2c[q, 2] + cy
    xy1[slots] = np.stack([pu1, pv1], 1) + rng.randn(n_all, 2) * noise
    xy2[k2] = np.stack([pu2, pv2], 1) + rng.randn(n_all, 2) * noise
    g = np.nonzero(kind == 1)[0]
    side = rng.rand(len(g)) < 0.5                                        # a gross error in one image only: bad in one direction
    off = rng.choice([-1, 1], (len(g), 2)) * rng.uniform(out_px[0], out_px[1], (len(g), 2))
    xy1[slots[g[side]]] += off[side]
    xy2[k2[g[~side]]] += off[~side]
    st = R.oplus(np.r_[rng.randn(3) * start[0], rng.randn(3) * start[1], rng.randn() * start[2]], true, fix_scale)
    return dict(T1w=T1w, xy_un1=np.nan_to_num(xy1).astype(F), point1=point1, points1=points1, assigned=assigned, points2=points2, flags2=flags2, index2=index2,
                xy_un2=np.nan_to_num(xy2).astype(F), T2w=T2w, S12=R.state_to(st), Tmw=Tmw, cam1=CAM, cam2=CAM, th2=TH2, fix_scale=fix_scale,
                all_points=all_points, inv_sigma2_1=float(F(w[0])), inv_sigma2_2=float(F(w[1])))


def edge_pins(n1):
    """the first keypoint, both sides of the first stride of 256 lanes, the last partial stride and the last keypoint"""
    return {k for k in (0, 255, 256, n1 - 257, n1 - 256, n1 - 1) if 0 <= k < n1}


# name -> arguments of make().  Between them: fix_scale 0 and 1; all_points 0 and 1 with points not in KF2 (their obs2 is the normalised pair); bad
# and NULL points on either side; z < 0 in camera 2 and a NaN z; 0 % outliers (n_more = 5) and 20 % (n_more = 10); n_corr - n_bad of exactly 9 and
# exactly 10; no pair; one pair; n1 of 1, 255, 256, 257 and 1024 / 1025, the two sides of the size at which the kernel instance changes, and
# XFH_GRID_MAX_N; pairs on the first and the last keypoint.  No scene has more than about 600 edges.  out100_w, out100_w_swap and out100_fix_w carry
# information weights (0.694444, 1.44), the swap, and the first again with a fixed scale: the rule's final_chi2 is 93.745 and 87.912 for the two orders
# (85.249 at (1, 1)), so weights exchanged between the two edge directions cannot pass.  The spread of the float64 forms on the three: state 8.7e-9,
# S12_out 0.125 and chi2 2.0 float32 steps, final_chi2 1.5e-10 -- under half of SIM3OPT_TOL, which test_spread_of_the_reference enforces.
SCENES = {
    "none": dict(seed=1, n_pairs=0, n1=40, bad2=3, null1=3, null_assigned=2, behind=2, nan_z=0),
    "one_n1": dict(seed=2, n_pairs=1, n1=1),
    "one": dict(seed=3, n_pairs=1, n1=40, pin={39}),
    "keep9": dict(seed=4, n_pairs=9, n1=64, outliers=3, out_px=(60, 90)),                          # n_corr - n_bad = 9: the early return
    "keep10": dict(seed=5, n_pairs=10, n1=64, outliers=3, out_px=(60, 90)),                        # = 10: round 2 runs
    "clean30": dict(seed=6, n_pairs=30, n1=255, pin=edge_pins(255)),                               # n_more = 5
    "clean30_fix": dict(seed=7, n_pairs=30, n1=256, fix_scale=1, pin=edge_pins(256)),
    "out100": dict(seed=8, n_pairs=80, n1=257, outliers=20, pin=edge_pins(257), bad2=4, null1=4, null_assigned=3, behind=3),
    "out100_fix": dict(seed=9, n_pairs=80, n1=300, outliers=20, fix_scale=1, start=(0.02, 0.05, 0.0)),
    "all_points": dict(seed=10, n_pairs=40, n1=300, outliers=8, not_in_kf2=12, all_points=1),   # twelve normalised-obs2 pairs
    "kf2_only": dict(seed=11, n_pairs=40, n1=300, outliers=8, not_in_kf2=12, all_points=0),             # the same without all_points: no edge
    "nan_z": dict(seed=16, n_pairs=30, n1=300, nan_z=2),                                           # a NaN z passes the z < 0 test: NaN sums, every trial fails
    "e1024": dict(seed=12, n_pairs=120, n1=1024, outliers=30, pin=edge_pins(1024) | {1023}, bad2=5, behind=5),
    "e1025": dict(seed=13, n_pairs=120, n1=1025, outliers=30, pin=edge_pins(1025) | {1023, 1024}, null1=5),
    "ws300": dict(seed=14, n_pairs=250, n1=3000, outliers=50, fix_scale=1, not_in_kf2=10, all_points=1),
    "keep9_ws": dict(seed=4, n_pairs=9, n1=64, outliers=3, out_px=(60, 90), fix_scale=1, all_points=1),   # the two neighbours of ws300 in WS_BATCH3
    "out100_ws": dict(seed=9, n_pairs=80, n1=300, outliers=20, fix_scale=1, all_points=1, not_in_kf2=5, start=(0.02, 0.05, 0.0)),
    "max": dict(seed=15, n_pairs=200, n1=16384, outliers=40, pin={0, 16383}),
    # information weights other than 1, different on the two sides (the workload's own are 1: octave 0); the swap has another final_chi2
    "out100_w": dict(seed=8, n_pairs=80, n1=257, outliers=20, pin=edge_pins(257), bad2=4, null1=4, null_assigned=3, behind=3, w=(0.694444, 1.44)),
    "out100_w_swap": dict(seed=8, n_pairs=80, n1=257, outliers=20, pin=edge_pins(257), bad2=4, null1=4, null_assigned=3, behind=3, w=(1.44, 0.694444)),
    "out100_fix_w": dict(seed=9, n_pairs=80, n1=300, outliers=20, fix_scale=1, start=(0.02, 0.05, 0.0), w=(0.694444, 1.44)),
}
BATCH3 = ("out100", "keep9", "clean30")                                 # B = 3: different pair counts, the middle one returns early
WS_BATCH3 = ("ws300", "keep9_ws", "out100_ws")                           # the same in the workspace instance (n1 = 3000)

# SIM3OPT_TOL: twice the largest spread of the float64 forms among themselves (the literal, the rule, the rule with exp / sin / cos / sqrt jittered by
# one double step under three seeds) that tests/test_optsim3_forms.py::test_spread_of_the_reference sees on SCENES and on 200 random small scenes:
# state 3.0e-7 of its largest entry, S12_out 4, Tcw 1, Ow 1 and chi2 6.5 float32 steps (at the magnitude of their block, and of max(chi2, th2)),
# final_chi2 7.7e-9 of max(final_chi2, th2); not below 1 float step and 1e-13 relative.  That test fails if it sees more than half of these
# constants.  Nothing from the device is in them; profiles/optimize_sim3.md has the table.  The numeric Jacobian is why a 1e-7 is there at all.
SIM3OPT_TOL = R.Tol(state=6e-7, s12=8, tcw=2, ow=2, chi2=13, final=1.6e-8)


def scene(name):
    return make(**SCENES[name])


def batch(problems):
    """problems padded to one (n1, M1, nq, n2): padding keypoints have no pair, padding rows are never named"""
    n1, M1 = max(len(p["assigned"]) for p in problems), max(len(p["points1"]) for p in problems)
    nq, n2 = max(len(p["points2"]) for p in problems), max(len(p["xy_un2"]) for p in problems)
    out = []
    for p in problems:
        o = dict(p)

        def pad(a, n, fill):
            a = np.asarray(a)
            r = np.full((n,) + a.shape[1:], fill, a.dtype)
            r[:len(a)] = a
            return r
        big = np.asarray(p["assigned"]) >= len(p["points2"])
        o["assigned"] = pad(np.where(big, nq + 1, p["assigned"]).astype(np.int32), n1, -1)
        o["point1"] = pad(np.where(np.asarray(p["point1"]) >= len(p["points1"]), M1 + 1, p["point1"]).astype(np.int32), n1, -1)
        o["xy_un1"], o["points1"], o["points2"] = pad(p["xy_un1"], n1, 0), pad(p["points1"], M1, 0), pad(p["points2"], nq, 0)
        o["flags2"], o["index2"], o["xy_un2"] = pad(p["flags2"], nq, 0), pad(p["index2"], nq, -1), pad(p["xy_un2"], n2, 0)
        out.append(o)
    return out


# ---- the float64 forms of a scene and their spread (tests/test_optsim3_forms.py, tests/test_optsim3_ref.py, tools/time_optsim3.py) ------------------
JITTER_SEEDS = (11, 12, 13)


def random_small(k):
    """scene k of the stream: 10 .. 25 good pairs on 64 keypoints, 0 / 2 / 4 outliers, both scale modes, every other pair of scenes with all_points
    and two points that are not in KF2"""
    ap = (k // 2) % 2
    return make(seed=1000 + k, n_pairs=10 + k % 16, n1=64, outliers=2 * (k % 3), fix_scale=k % 2, all_points=ap, not_in_kf2=2 * ap, bad2=k % 2, behind=(k // 4) % 2)


def problem_of(name):
    return scene(name) if isinstance(name, str) else random_small(name)


@functools.lru_cache(maxsize=None)
def host_of(name):
    """the library's host form (xfh_sim3_optimize_host) of the scene: one more float64 form, the kernel's own lines on one host thread"""
    return run_host([problem_of(name)])[0]


@functools.lru_cache(maxsize=None)
def forms_of(name):
    """-> [literal, rule, rule with three libm jitters] of a rig scene (a name) or of stream scene k (an int): the float64 forms, cached"""
    p = problem_of(name)
    return [RL.literal(p), R.rule(p)] + [R.rule(p, libm_jitter=s) for s in JITTER_SEEDS]


def spread(forms):
    """the largest distance between any two of the forms, per output"""
    worst = dict.fromkeys(R.Tol._fields, 0.0)
    for i in range(len(forms)):
        for j in range(i + 1, len(forms)):
            for k, v in R.distances(forms[i], forms[j], TH2).items():
                worst[k] = max(worst[k], v)
    return worst


def cam_struct(cam=CAM):
    c = capi.Camera()
    c.fx, c.fy, c.cx, c.cy = cam[:4]
    c.width, c.height = 640, 480
    return c


SIDE1 = (("T1w", F), ("xy_un1", F), ("point1", np.int32), ("points1", F))
SIDE2 = (("assigned", np.int32), ("points2", F), ("flags2", np.uint8), ("index2", np.int32), ("xy_un2", F), ("T2w", F))


def _inputs(problems, side1_shared):
    p0 = problems[0]
    dims = (len(p0["assigned"]), len(p0["points1"]), len(p0["points2"]), len(p0["xy_un2"]))
    assert all((len(p["assigned"]), len(p["points1"]), len(p["points2"]), len(p["xy_un2"])) == dims for p in problems), "use batch()"
    for k in ("th2", "fix_scale", "all_points", "inv_sigma2_1", "inv_sigma2_2"):
        assert all(p[k] == p0[k] for p in problems), k
    one = problems[:1] if side1_shared else problems
    arrays = [np.ascontiguousarray(np.stack([np.asarray(p[k], dt) for p in one])) for k, dt in SIDE1]
    arrays += [np.ascontiguousarray(np.stack([np.asarray(p[k], dt) for p in problems])) for k, dt in SIDE2]
    s12 = np.ascontiguousarray(np.stack([np.asarray(p["S12"], F) for p in problems]))
    tmw = None if p0.get("Tmw") is None else np.ascontiguousarray(np.stack([np.asarray(p["Tmw"], F) for p in problems]))
    return dims, arrays, s12, tmw


def _split(B, arrays, has_tmw):
    """dict of output arrays with a leading B -> one dict per problem (Tcw and Ow only where the call had a Tmw)"""
    return guarded.problems(arrays, B, [k for k in arrays if has_tmw or k not in ("Tcw", "Ow")])


def run_host(problems, side1_shared=False, L=None):
    """xfh_sim3_optimize_host on B problems -> per problem dict of outputs"""
    L = L or capi.lib()
    B = len(problems)
    (n1, M1, nq, n2), arrays, s12, tmw = _inputs(problems, side1_shared)
    p0 = problems[0]
    outs = Context.sim3_optimize_layout(B, n1).zeros()
    ws = np.zeros(int(L.xfh_sim3_optimize_workspace_bytes(n1, B)) + 16, np.uint8)
    wsp = (ws.ctypes.data + 15) & ~15
    c1, c2 = cam_struct(p0["cam1"]), cam_struct(p0["cam2"])
    rc = L.xfh_sim3_optimize_host(B, n1, M1, nq, n2, int(side1_shared), *[a.ctypes.data for a in arrays], s12.ctypes.data, 13,
                                  None if tmw is None else tmw.ctypes.data, C.byref(c1), C.byref(c2), p0["th2"], p0["fix_scale"], p0["all_points"],
                                  p0["inv_sigma2_1"], p0["inv_sigma2_2"], wsp, outs["assigned_out"].ctypes.data, outs["status"].ctypes.data,
                                  outs["chi2"].ctypes.data, outs["state"].ctypes.data, outs["S12_out"].ctypes.data, 13,
                                  None if tmw is None else outs["Tcw"].ctypes.data, None if tmw is None else outs["Ow"].ctypes.data,
                                  outs["header"].ctypes.data, outs["final_chi2"].ctypes.data)
    assert rc == 0, rc
    return _split(B, outs, tmw is not None)


class Sim3OptRig:
    """device buffers for B problems; run() -> per problem dict of outputs, the raw output bytes, guards checked; .workspace is the workspace as
    the last run left it"""

    def __init__(self, L):
        self.L = L
        self.ctx = Context(nfeatures=1, max_height=32, max_width=32)

    def close(self):
        self.ctx.close()

    def run(self, problems, side1_shared=False, fill=guarded.FILL, in_place=False, ws_fill=0x3C, s12_stride=13):
        """fill: the byte around and under the outputs and around the workspace; ws_fill: the byte the workspace holds before the call.  in_place:
        d_assigned_out = d_assigned and d_S12_out = d_S12."""
        L, B = self.L, len(problems)
        (n1, M1, nq, n2), arrays, s12, tmw = _inputs(problems, side1_shared)
        p0 = problems[0]
        if s12_stride != 13:                                             # the solver's layout: 13 floats inside a wider record
            wide = np.full((B, s12_stride), np.nan, F)
            wide[:, :13] = s12
            s12 = wide
        dev = [capi.DeviceBuffer(a.nbytes).upload(a) for a in arrays + [s12] + ([tmw] if tmw is not None else [])]
        lay = Context.sim3_optimize_layout(B, n1, GUARD)
        out = guarded.outputs(lay, fill)
        ws_bytes = int(L.xfh_sim3_optimize_workspace_bytes(n1, B))
        assert ws_bytes > 0 and ws_bytes % 16 == 0
        ws = guarded.Guarded(ws_bytes, GUARD, fill, inner=ws_fill)
        c1, c2 = cam_struct(p0["cam1"]), cam_struct(p0["cam2"])
        ptr = lambda k: out.ptr + lay[k]
        a_out = dev[4].ptr if in_place else ptr("assigned_out")
        s_out, s_out_stride = (dev[10].ptr, s12_stride) if in_place else (ptr("S12_out"), 13)
        rc = L.xfh_sim3_optimize_device(self.ctx.h, B, n1, M1, nq, n2, int(side1_shared), *[d.ptr for d in dev[:10]], dev[10].ptr, s12_stride,
                                        dev[11].ptr if tmw is not None else None, C.byref(c1), C.byref(c2), p0["th2"], p0["fix_scale"], p0["all_points"],
                                        p0["inv_sigma2_1"], p0["inv_sigma2_2"], ws.ptr, a_out, ptr("status"), ptr("chi2"), ptr("state"), s_out,
                                        s_out_stride, ptr("Tcw") if tmw is not None else None, ptr("Ow") if tmw is not None else None, ptr("header"),
                                        ptr("final_chi2"))
        assert rc == 0, rc
        self.ctx.synchronize()
        skip = (("assigned_out", "S12_out") if in_place else ()) + (() if tmw is not None else ("Tcw", "Ow"))
        raw = guarded.download(out, lay, fill, skip)
        self.workspace = ws.download()
        a = lay.parse(raw)
        if in_place:
            a["assigned_out"] = dev[4].download(np.int32, B * n1).reshape(B, n1)
            wide_after = dev[10].download(F, B * s12_stride).reshape(B, s12_stride)
            assert np.all(np.isnan(wide_after[:, 13:])), "the rest of the solver's record was written"
            a["S12_out"] = wide_after[:, :13].copy()
        for d in dev + [out, ws]:
            d.free()
        return _split(B, a, tmw is not None), raw[lay.used(skip)]
