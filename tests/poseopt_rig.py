"""Seeded scenes for xfh_pose_optimize_device and its restatements (tests/ref_poseopt.py): map points in front of a pinhole camera, observations =
their projection at the true pose + noise, a perturbed start pose.  SCENES is the table the CPU test checks the condition of and the GPU tests
compare on; PoseRig runs them on the device between guard bytes."""
import ctypes as C

import numpy as np

import ref_poseopt as RP
from xfeatslam_amd import capi

F, D = np.float32, np.float64
CAM = (517.3, 516.5, 318.6, 255.3, 40.0)                                # fx, fy, cx, cy, bf (TUM1-like)
INV_SIGMA2 = 1.0
GUARD = 256


def make(seed, n_edges, nt, kind="mono", outliers=0.0, noise=0.7, start=(0.02, 0.05), beyond=0, identical=False, spare=5):
    """-> dict(Tcw, xy_un, uright, assigned, points, nt, nq).  kind: mono (uright None), stereo, mixed (uright < 0 on half), mono_ur (an all-negative
    uright array).  start = (rotation [rad], translation [m]) size of the perturbation.  beyond = keypoints whose assigned entry is >= nq.
    identical: every edge sees the same map point."""
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
    slots = np.sort(rng.choice(nt, n_edges + beyond, replace=False))
    assigned = np.full(nt, -1, np.int32)
    which = rng.permutation(n_edges + beyond)
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
    return dict(Tcw=RP.to_tcw(st), xy_un=xy.astype(F), uright=uright, assigned=assigned, points=points, nt=nt, nq=nq)


# name -> arguments of make().  The seeds were chosen so that tests/test_poseopt_ref.py::test_rig_condition holds: every decision of the literal
# form stays farther than 1e-9 (relative) from its decision point.  Edge counts 2, 3, 9, 10, 63, 64, 65, 257 and about 1000.
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
}
BATCH3 = ("n64_stereo", "n2", "n257")                                   # B = 3: different edge counts, the middle one refused at < 3


def scene(name):
    return make(**SCENES[name])


def batch(names):
    """scenes padded to one (nt, nq): -> list of scenes with common shapes (padding keypoints have no edge, padding points are never named)"""
    sc = [scene(n) for n in names]
    nt, nq = max(s["nt"] for s in sc), max(s["nq"] for s in sc)
    out = []
    for s in sc:
        a = np.full(nt, -1, np.int32); a[:s["nt"]] = np.where(s["assigned"] >= s["nq"], nq + 1, s["assigned"])
        xy = np.zeros((nt, 2), F); xy[:s["nt"]] = s["xy_un"]
        ur = np.full(nt, -1.0, F)
        if s["uright"] is not None:
            ur[:s["nt"]] = s["uright"]
        p = np.zeros((nq, 3), F); p[:s["nq"]] = s["points"]
        out.append(dict(Tcw=s["Tcw"], xy_un=xy, uright=ur, assigned=a, points=p, nt=nt, nq=nq))
    return out


def model(s, form=RP.rule):
    return form(s["Tcw"], CAM, s["xy_un"], s["uright"], s["assigned"], s["points"], INV_SIGMA2)


def cam_struct():
    c = capi.Camera()
    c.fx, c.fy, c.cx, c.cy, c.bf = CAM
    c.width, c.height = 640, 480
    return c


OUTS = (("Tcw_out", F, 12), ("outlier", np.uint8, None), ("chi2", F, None), ("header", np.int32, 8), ("final_chi2", D, 1))


class PoseRig:
    """device buffers for B problems of (nt, nq); run() -> per problem dict of outputs, the raw output bytes, guards checked"""

    def __init__(self, L):
        from xfeatslam_amd.extractor import Context
        self.L = L
        self.ctx = Context(nfeatures=1, max_height=32, max_width=32)
        self.cam = cam_struct()

    def close(self):
        self.ctx.close()

    def run(self, scenes, fill=0xA5, uright=True, in_place=False):
        L, B, nt, nq = self.L, len(scenes), scenes[0]["nt"], scenes[0]["nq"]
        assert all(s["nt"] == nt and s["nq"] == nq for s in scenes)
        has_ur = uright and scenes[0]["uright"] is not None
        ins = [np.stack([s["Tcw"] for s in scenes]).astype(F), np.stack([s["xy_un"] for s in scenes]).astype(F),
               np.stack([s["uright"] for s in scenes]).astype(F) if has_ur else None,
               np.stack([s["assigned"] for s in scenes]).astype(np.int32), np.stack([s["points"] for s in scenes]).astype(F)]
        dev = [None if a is None else capi.DeviceBuffer(a.nbytes).upload(a) for a in ins]
        al = lambda x: (x + 255) & ~255
        off, pos = {}, GUARD
        for name, dt, per in OUTS:
            off[name] = pos
            pos = al(pos + B * (per or nt) * np.dtype(dt).itemsize + GUARD)
        out = capi.DeviceBuffer(pos).upload(np.full(pos, fill, np.uint8))
        ws = capi.DeviceBuffer(max(16, int(L.xfh_pose_optimize_workspace_bytes(nt, B))))
        tcw_out = dev[0].ptr if in_place else out.ptr + off["Tcw_out"]
        rc = L.xfh_pose_optimize_device(self.ctx.h, B, nt, nq, dev[0].ptr, C.byref(self.cam), dev[1].ptr, dev[2].ptr if has_ur else None, dev[3].ptr,
                                        dev[4].ptr, INV_SIGMA2, ws.ptr, tcw_out, out.ptr + off["outlier"], out.ptr + off["chi2"], out.ptr + off["header"],
                                        out.ptr + off["final_chi2"])
        assert rc == 0, rc
        self.ctx.synchronize()
        raw = out.download(np.uint8, pos)
        written = np.zeros(pos, bool)
        res = [dict() for _ in range(B)]
        for name, dt, per in OUTS:
            n = per or nt
            size = B * n * np.dtype(dt).itemsize
            if name == "Tcw_out" and in_place:
                a = dev[0].download(F, B * 12)
            else:
                a = raw[off[name]:off[name] + size].view(dt)
                written[off[name]:off[name] + size] = True
            for b in range(B):
                res[b][name] = a[b * n:(b + 1) * n].copy() if name != "final_chi2" else float(a[b])
        assert np.all(raw[~written] == fill), "bytes outside the output arrays were written"
        for d in dev + [out, ws]:
            if d is not None:
                d.free()
        return res, raw[written].copy()
