"""Seeded scenes for xfh_pose_optimize_device and its restatements (tests/ref_poseopt.py): map points in front of a pinhole camera, observations =
their projection at the true pose + noise, a perturbed start pose.  SCENES and EDGE_SCENES are the tables the CPU test checks the 1e-9 condition of
and the GPU tests compare on exactly; MONO_SCENES (all-mono, ten or more edges) hold a condition on their outputs only and are compared within
MONO_TOL; PoseRig runs them on the device, outputs and workspace between guard bytes."""
import ctypes as C

import numpy as np

import guarded
import ref_poseopt as RP
from xfeatslam_amd import capi

F, D = np.float32, np.float64
CAM = (517.3, 516.5, 318.6, 255.3, 40.0)                                # fx, fy, cx, cy, bf (TUM1-like)
INV_SIGMA2 = 1.0
GUARD = 256


def make(seed, n_edges, nt, kind="mono", outliers=0.0, noise=0.7, start=(0.02, 0.05), beyond=0, identical=False, spare=5, pin=None, w=INV_SIGMA2):
    """-> dict(Tcw, xy_un, uright, assigned, points, nt, nq, w).  w: the information weight inv_sigma2 of every edge (nothing is drawn for it).  kind: mono (uright None), stereo, mixed (uright < 0 on half), mono_ur (an all-negative
    uright array).  start = (rotation [rad], translation [m]) size of the perturbation.  beyond = keypoints whose assigned entry is >= nq.
    identical: every edge sees the same map point.  pin: keypoint numbers that carry an edge whatever the seed (the others are drawn)."""
    rng = np.random.RandomState(seed)
    fx, fy, cx, cy, bf = CAM
    nq = n_edges + spare
    true = RP.oplus(np.r_[rng.uniform(-0.3, 0.3, 3), rng.uniform(-1, 1, 3)], [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
    z = rng.uniform(1.5, 9.0, nq)
    u, v = rng.uniform(20, 620, nq), rng.uniform(20, 460, nq)
    Xc = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
    if identical:
        Xc[:] = Xc[0]
    inv = RP.normalize([-true[0], -true[1], -true[2], true[3]])          # world = R^T (Xc - t)
    d = Xc - np.array(true[4:7])
    points = np.stack(RP.rotate(inv, [d[:, 0], d[:, 1], d[:, 2]]), 1).astype(F)
    if pin:
        pinned = np.array(sorted(pin))
        assert len(pinned) <= n_edges and pinned[0] >= 0 and pinned[-1] < nt
        rest = rng.choice(np.setdiff1d(np.arange(nt), pinned), n_edges + beyond - len(pinned), replace=False)
        slots = np.sort(np.r_[pinned, rest])
    else:
        slots = np.sort(rng.choice(nt, n_edges + beyond, replace=False))
    assigned = np.full(nt, -1, np.int32)
    which = rng.permutation(n_edges + beyond)
    if pin:                                                              # the pinned slots among those that get an edge, not an entry >= nq
        which = np.r_[which[np.isin(slots[which], pinned)], which[~np.isin(slots[which], pinned)]]
    pid = rng.permutation(nq)[:n_edges]
    assigned[slots[which[:n_edges]]] = pid
    assigned[slots[which[n_edges:]]] = nq + rng.randint(0, 3, beyond)
    xy = rng.uniform(0, 640, (nt, 2))
    ur = rng.uniform(0, 600, nt)
    k = slots[which[:n_edges]]
    pc, _, _ = RP.edge_error(true, RP.cam_of(CAM), points[pid].astype(D), np.zeros((n_edges, 3)), np.zeros(n_edges, bool), 1.0)
    pu, pv = fx * pc[0] / pc[2] + cx, fy * pc[1] / pc[2] + cy
    xy[k, 0], xy[k, 1] = pu + rng.randn(n_edges) * noise, pv + rng.randn(n_edges) * noise
    ur[k] = pu - bf / pc[2] + rng.randn(n_edges) * noise
    gross = k[rng.rand(n_edges) < outliers]
    xy[gross] += rng.choice([-1, 1], (len(gross), 2)) * rng.uniform(15, 80, (len(gross), 2))
    uright = None
    if kind == "stereo":
        uright = ur.astype(F)
    elif kind == "mixed":
        uright = np.where(rng.rand(nt) < 0.5, ur, -1.0).astype(F)
    elif kind == "mono_ur":
        uright = np.full(nt, -1.0, F)
    st = RP.oplus(np.r_[rng.randn(3) * start[0], rng.randn(3) * start[1]], true)
    return dict(Tcw=RP.to_tcw(st), xy_un=xy.astype(F), uright=uright, assigned=assigned, points=points, nt=nt, nq=nq, w=float(F(w)))


# name -> arguments of make().  The seeds were chosen so that tests/test_poseopt_ref.py::test_rig_condition holds: every decision of the literal
# form stays farther than 1e-9 (relative) from its decision point.  Edge counts 2, 3, 9, 10, 63, 64, 65, 257 and about 1000.  The four *_w scenes are
# n63_mono_far and far_stereo at inv_sigma2 = float32(0.694) and float32(1.44) (far_stereo_s153_w144: far_stereo's arguments with seed 153, because with
# seed 151 and this weight a round ends on rho == 0 exactly, which the 1e-9 condition excludes): literal and rule decide alike and differ by 0 float steps in pose and
# chi2 and by at most 3.8e-15 in final_chi2 (the exact comparison's bound is 1 step and 1e-9), the kernel's loop on the host equals the rule by bytes, and
# the smallest |rho| of the four is 2.3e-9 (n63_mono_far_w0694).  Every existing scene keeps w = 1.
SCENES = {
    "n2": dict(seed=1, n_edges=2, nt=40),
    "n3": dict(seed=100, n_edges=3, nt=40, kind="stereo"),
    "n9_mono": dict(seed=100, n_edges=9, nt=64, noise=3.0),
    "n9_mixed": dict(seed=101, n_edges=9, nt=64, kind="mixed"),
    "n10": dict(seed=100, n_edges=10, nt=64, kind="stereo"),
    "n63_mono_far": dict(seed=170, n_edges=63, nt=300, noise=1.0, outliers=0.2, start=(0.3, 0.8)),      # 40 iterations, edges that come back
    "n63_mono_lost": dict(seed=153, n_edges=63, nt=300, noise=1.0, outliers=0.2, start=(0.3, 0.8)),     # trials rejected outright; then no level-0 edge
    "n64_stereo": dict(seed=182, n_edges=64, nt=300, kind="stereo", outliers=0.2),                      # a round that ends on ten rejected trials
    "n65_mixed": dict(seed=277, n_edges=65, nt=257, kind="mixed", outliers=0.2, beyond=6),
    "n257": dict(seed=126, n_edges=257, nt=1025, kind="mixed", outliers=0.2),
    "n1000": dict(seed=9, n_edges=1000, nt=4096, kind="mixed", outliers=0.2, beyond=20),
    "far_stereo": dict(seed=151, n_edges=120, nt=500, kind="stereo", outliers=0.1, noise=1.0, start=(0.25, 0.6)),
    "identical": dict(seed=100, n_edges=12, nt=64, identical=True, kind="stereo"),                      # rank-deficient H: lambda keeps every pivot positive
    "big": dict(seed=14, n_edges=700, nt=5000, kind="mixed", outliers=0.2),                             # nt > 4096: the workspace instance
    # an information weight other than 1 (the workload's own is 1: octave 0): the two far starts, below and above 1
    "n63_mono_far_w0694": dict(seed=170, n_edges=63, nt=300, noise=1.0, outliers=0.2, start=(0.3, 0.8), w=0.694),
    "n63_mono_far_w144": dict(seed=170, n_edges=63, nt=300, noise=1.0, outliers=0.2, start=(0.3, 0.8), w=1.44),
    "far_stereo_w0694": dict(seed=151, n_edges=120, nt=500, kind="stereo", outliers=0.1, noise=1.0, start=(0.25, 0.6), w=0.694),
    "far_stereo_s153_w144": dict(seed=153, n_edges=120, nt=500, kind="stereo", outliers=0.1, noise=1.0, start=(0.25, 0.6), w=1.44),   # far_stereo's arguments under another seed: 151 ends a round on rho == 0 here
}
BATCH3 = ("n64_stereo", "n2", "n257")                                   # B = 3: different edge counts, the middle one refused at < 3

# All-mono scenes of ten or more edges that converge: what a monocular tracker has, and what the 1e-9 condition shuts out (the last round converges into
# rounding noise, where rho is noise / 1e-3 and the number of trials is chance).  Their condition is tests/test_poseopt_ref.py::test_mono_scene_condition:
# every classification farther than 1e-4 from its cut, every pivot farther than 1e-9 from 0, in both forms; they are compared through
# ref_poseopt.outputs_agree with MONO_TOL.  Both ways of being mono (uright None: "null"; an all-negative array: "neg"), 0 % and 20 % outliers, and nt
# in each of the three ranges that select a kernel instance (<= 1024, 1025 .. 4096, above), so that each instance meets a null uright.
MONO_SCENES = {
    "m100_null": dict(seed=1, n_edges=100, nt=400),
    "m100_neg_out": dict(seed=1, n_edges=100, nt=400, kind="mono_ur", outliers=0.2),
    "m200_null_out": dict(seed=1, n_edges=200, nt=1024, outliers=0.2, pin={0, 255, 256, 1023}),
    "m300_null": dict(seed=1, n_edges=300, nt=1025, pin={1024}),
    "m1000_neg_out": dict(seed=1, n_edges=1000, nt=4096, kind="mono_ur", outliers=0.2, pin={4095}),
    "m700_null_out": dict(seed=1, n_edges=700, nt=5000, outliers=0.2, pin={4096, 4999}),
    "m700_neg": dict(seed=1, n_edges=700, nt=5000, kind="mono_ur"),
    "m400_null_max": dict(seed=1, n_edges=400, nt=16384, pin={0, 16383}),
}
# The spread of the float64 forms among themselves on all-mono scenes (literal, rule, rule with three libm jitters; MONO_SCENES and 200 stream scenes),
# measured by tests/test_poseopt_ref.py::test_mono_spread_of_the_reference: twice the largest value seen there (pose 1 and chi2 53 float32 steps -- on
# a chi2 of 5e-4, where obs - projection cancels -- and final_chi2 9.8e-14 relative), not below 1 step and 1e-13.  That test fails if it sees more
# than half of these constants; profiles/pose_optimization.md has the table.  Nothing from the device is in them.
MONO_TOL = RP.Tol(pose=2, chi2=106, final=2e-13)


def edge_pins(nt):
    """the first keypoint, both sides of the first stride of 256 lanes, the last partial stride and the last keypoint, and both sides of the sizes at
    which the instance changes"""
    return {0, 255, 256, nt - 257, nt - 256, nt - 1} | {k for k in (1023, 1024, 4095, 4096) if k < nt}


# nt at the last size of k_pose_optimize<4>, the first and last of <16>, the first of the workspace instance and XFH_GRID_MAX_N, with edges at
# edge_pins(nt).  Stereo or mixed, so that the 1e-9 condition can hold (test_rig_condition) and the comparison is the exact one.
EDGE_SCENES = {
    "e1024": dict(seed=3, n_edges=200, nt=1024, kind="stereo", outliers=0.2, pin=edge_pins(1024)),
    "e1025": dict(seed=3, n_edges=257, nt=1025, kind="mixed", outliers=0.2, pin=edge_pins(1025)),
    "e4096": dict(seed=1, n_edges=300, nt=4096, kind="mixed", outliers=0.1, pin=edge_pins(4096)),
    "e4097": dict(seed=2, n_edges=300, nt=4097, kind="stereo", outliers=0.2, pin=edge_pins(4097)),
    "e16384": dict(seed=1, n_edges=400, nt=16384, kind="mixed", outliers=0.2, beyond=10, pin=edge_pins(16384)),
}
WS_BATCH3 = ("big", "m700_null_out", "n2")                              # B = 3 at nt = 5000: conditioned mixed, all-mono (neighbours in the workspace), refused
NULL_BATCH2 = ("m300_null", "m1000_neg_out")                            # B = 2 at nt = 4096, run with a null uright


def scene(name):
    for table in (SCENES, MONO_SCENES, EDGE_SCENES):
        if name in table:
            return make(**table[name])
    raise KeyError(name)


def batch(names, null_uright=False):
    """scenes padded to one (nt, nq): -> list of scenes with common shapes (padding keypoints have no edge, padding points are never named).
    null_uright: the scenes are all-mono and stay without a uright array (the call gets a null pointer)"""
    sc = [scene(n) for n in names]
    nt, nq = max(s["nt"] for s in sc), max(s["nq"] for s in sc)
    out = []
    for s in sc:
        a = np.full(nt, -1, np.int32); a[:s["nt"]] = np.where(s["assigned"] >= s["nq"], nq + 1, s["assigned"])
        xy = np.zeros((nt, 2), F); xy[:s["nt"]] = s["xy_un"]
        ur = np.full(nt, -1.0, F)
        if s["uright"] is not None:
            assert not null_uright or not (s["uright"] >= 0).any(), "a scene with stereo edges cannot go without uright"
            ur[:s["nt"]] = s["uright"]
        p = np.zeros((nq, 3), F); p[:s["nq"]] = s["points"]
        out.append(dict(Tcw=s["Tcw"], xy_un=xy, uright=None if null_uright else ur, assigned=a, points=p, nt=nt, nq=nq, w=s.get("w", INV_SIGMA2)))
    return out


def model(s, form=RP.rule):
    return form(s["Tcw"], CAM, s["xy_un"], s["uright"], s["assigned"], s["points"], s.get("w", INV_SIGMA2))


def cam_struct():
    c = capi.Camera()
    c.fx, c.fy, c.cx, c.cy, c.bf = CAM
    c.width, c.height = 640, 480
    return c


class PoseRig:
    """device buffers for B problems of (nt, nq); run() -> per problem dict of outputs, the raw output bytes, guards checked; .workspace is the
    workspace as the last run left it"""

    def __init__(self, L):
        from xfeatslam_amd.extractor import Context
        self.L = L
        self.ctx = Context(nfeatures=1, max_height=32, max_width=32)
        self.cam = cam_struct()

    def close(self):
        self.ctx.close()

    def run(self, scenes, fill=guarded.FILL, uright=True, in_place=False, ws_fill=0x3C):
        """fill: the byte around and under the outputs and around the workspace; ws_fill: the byte the workspace holds before the call.  Scenes
        whose uright is None (all of them, or none) give the call a null pointer."""
        L, B, nt, nq = self.L, len(scenes), scenes[0]["nt"], scenes[0]["nq"]
        assert all(s["nt"] == nt and s["nq"] == nq for s in scenes)
        assert len({s["uright"] is None for s in scenes}) == 1, "uright is one pointer for the whole call"
        assert len({s.get("w", INV_SIGMA2) for s in scenes}) == 1, "inv_sigma2 is one value for the whole call"
        has_ur = uright and scenes[0]["uright"] is not None
        ins = [np.stack([s["Tcw"] for s in scenes]).astype(F), np.stack([s["xy_un"] for s in scenes]).astype(F),
               np.stack([s["uright"] for s in scenes]).astype(F) if has_ur else None,
               np.stack([s["assigned"] for s in scenes]).astype(np.int32), np.stack([s["points"] for s in scenes]).astype(F)]
        dev = [None if a is None else capi.DeviceBuffer(a.nbytes).upload(a) for a in ins]
        lay = self.ctx.pose_optimize_layout(B, nt, GUARD)
        out = guarded.outputs(lay, fill)
        ws_bytes = int(L.xfh_pose_optimize_workspace_bytes(nt, B))      # exactly what the call may use, between two guards
        assert ws_bytes > 0 and ws_bytes % 16 == 0
        ws = guarded.Guarded(ws_bytes, GUARD, fill, inner=ws_fill)
        tcw_out = dev[0].ptr if in_place else out.ptr + lay["Tcw_out"]
        rc = L.xfh_pose_optimize_device(self.ctx.h, B, nt, nq, dev[0].ptr, C.byref(self.cam), dev[1].ptr, dev[2].ptr if has_ur else None, dev[3].ptr,
                                        dev[4].ptr, scenes[0].get("w", INV_SIGMA2), ws.ptr, tcw_out, *[out.ptr + lay[k] for k in lay.names[1:]])
        assert rc == 0, rc
        self.ctx.synchronize()
        skip = ("Tcw_out",) if in_place else ()
        raw = guarded.download(out, lay, fill, skip)
        self.workspace = ws.download()                                  # as the call left it: B strides of xfh_pose_optimize_workspace_bytes(nt, 1)
        a = lay.parse(raw)
        if in_place:
            a["Tcw_out"] = dev[0].download(F, B * 12).reshape(B, 12)
        for d in dev + [out, ws]:
            if d is not None:
                d.free()
        return guarded.problems(a, B), raw[lay.used(skip)]
