"""The scenes of the triangulation tests (tests/test_triangulate_ref.py, tests/test_gpu_triangulate.py, tests/test_gpu_triangulate_cpp.py,
tools/time_triangulate.py) and one guarded run of xfh_triangulate_device.  main_scene() is the SearchForTriangulation scene of
tests/triangulation_rig.py (n1 = 301, n2 = 515, B = 3) with what the triangulation reads beside it: the poses its seeds drew, mvDepth under every
stereo keypoint and the camera centres.  small_scene() is a seeded keyframe with B neighbours of any size, built the same way, for the random
comparisons and the n1 = 65 case; planted() puts pairs with written-out causes into it.  No test lives here."""
import numpy as np

import guarded
import ref_triangulate as RG
import ref_triangulation as RT
import triangulation_rig as TR
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context

F = np.float32
GUARD = 4096
CAM = {k: TR.K[k] for k in ("fx", "fy", "cx", "cy", "bf")}
SCALE_FACTOR, NLEVELS = 1.2, 8
RATIO_FACTOR = float(F(1.5) * F(SCALE_FACTOR))
SCALE_LAST = float(F(SCALE_FACTOR) ** 7)
FAR_TH = 8.5                                # mThFarPoints of the main scene: its points lie 3.5 .. 9 m away, so the gate is met from both sides


def cam_struct(cam=CAM):
    c = capi.Camera()
    for k, v in cam.items():
        setattr(c, k, float(v))
    c.width, c.height = 640, 480
    return c


def main_params(**kw):
    return RG.params(CAM, **dict(dict(sigma2=1.0, ratio_factor=RATIO_FACTOR, scale_last=SCALE_LAST, far_th=FAR_TH), **kw))


def pose(R, t):
    """X_c = R X_w + t -> (Tcw[12], Ow[3]) in float32; the centre from the float64 pose, rounded once"""
    return np.concatenate([R, t[:, None]], 1).astype(F).reshape(12), (-R.T @ t).astype(F)


def depth_of(k):
    """mvDepth of an RGB-D keyframe from its mvuRight: z = bf / (x - uright) where there is one, else -1"""
    ur = k["ur"]
    with np.errstate(all="ignore"):
        z = F(CAM["bf"]) / (k["xy"][:, 0] - ur)
    return np.where(ur >= 0, z, F(-1)).astype(F)


def fundamental(R, t):
    """F12 and the epipole as tests/triangulation_rig.py computes them"""
    Km = np.array([[CAM["fx"], 0, CAM["cx"]], [0, CAM["fy"], CAM["cy"]], [0, 0, 1.0]])
    R12, t12 = R.T, -R.T @ t
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    F12 = (np.linalg.inv(Km.T) @ tx @ R12 @ np.linalg.inv(Km)).astype(F).reshape(9)
    with np.errstate(all="ignore"):
        ep = np.array([CAM["fx"] * t[0] / t[2] + CAM["cx"], CAM["fy"] * t[1] / t[2] + CAM["cy"]]).astype(F)
    return F12, ep


class Scn:
    """k1, k2[B], F12[B], ep[B]; dist(b) = the DescriptorDistance table both forms of the search read"""

    def dists(self, O=None):
        if getattr(self, "_d", None) is None:
            self._d = [O.distance_i32(self.k1["desc"], k["desc"]) if O is not None else RG.numpy_dist(self.k1["desc"], k["desc"]) for k in self.k2]
        return self._d


def main_scene(seed=7100):
    s = TR.Scene(seed)
    o = Scn()
    I, z0 = np.eye(3), np.zeros(3)
    T1, O1 = pose(I, z0)
    o.k1 = dict(s.k1, depth=np.where(s.k1["ur"] >= 0, s.X[:, 2].astype(F), F(-1)).astype(F), Tcw=T1, Ow=O1)
    o.k2, o.F12, o.ep = [], s.F12, s.ep
    for b, k in enumerate(s.k2):
        rng = np.random.RandomState(seed + 1 + b)                          # the pose TR.neighbour drew first from this seed
        R = TR.rot(*rng.uniform(-0.04, 0.04, 3))
        t = np.array([rng.uniform(0.25, 0.4), rng.uniform(-0.05, 0.05), rng.uniform(0.9, 1.3)])
        assert np.array_equal(fundamental(R, t)[0], s.F12[b])
        T2, O2 = pose(R, t)
        o.k2.append(dict(k, depth=depth_of(k), Tcw=T2, Ow=O2))
    return o


def small_scene(seed, n1=12, n2=14, B=3):
    """a keyframe at the origin and B neighbours: sideways, forward and mixed motion, pixel noise from 0.2 to 4 px, points from 2 to 80 m, a third
    of the keypoints stereo, two vocabulary nodes"""
    rng = np.random.RandomState(seed)
    o = Scn()
    X = np.stack([rng.uniform(-1.5, 1.5, n1), rng.uniform(-1.0, 1.0, n1), rng.uniform(2.0, 9.0, n1)], 1)
    far = rng.rand(n1) < 0.2
    X[far] *= rng.uniform(4, 10, (int(far.sum()), 1))
    xy = TR.project(X).astype(F)
    T1, O1 = pose(np.eye(3), np.zeros(3))
    ur = TR.uright_of(rng, xy, X[:, 2], 0.4)
    o.k1 = dict(node_of=rng.randint(0, 2, n1).astype(np.uint32), xy=xy, ur=ur, has=(rng.rand(n1) < 0.1).astype(np.uint8), desc=TR.unit_rows(rng, n1),
                depth=np.where(ur >= 0, X[:, 2].astype(F), F(-1)).astype(F), Tcw=T1, Ow=O1)
    o.k2, o.F12, o.ep = [], [], []
    for b in range(B):
        R = TR.rot(*rng.uniform(-0.05, 0.05, 3))
        t = np.array([rng.uniform(-0.6, 0.6), rng.uniform(-0.1, 0.1), rng.uniform(-0.2, 0.8)])
        t[0] += 0.25 * np.sign(t[0])
        Fm, ep = fundamental(R, t)
        xy2 = np.stack([rng.uniform(10, 630, n2), rng.uniform(10, 470, n2)], 1)
        z2 = rng.uniform(2.0, 9.0, n2)
        desc = TR.unit_rows(rng, n2)
        node_of = rng.randint(0, 2, n2).astype(np.uint32)
        seen = rng.permutation(n1)[:min(n2, int(0.75 * n1))]
        for i, k in zip(seen, rng.permutation(n2)):
            X2 = R @ X[i] + t
            if X2[2] < 0.5:
                continue
            xy2[k] = TR.project(X2[None])[0] + rng.uniform(-1, 1, 2) * rng.choice([0.2, 0.2, 0.2, 1.5, 4.0])
            z2[k] = X2[2]
            row = o.k1["desc"][i].astype(np.float64) + 0.03 * rng.randn(64)
            desc[k] = (row / np.linalg.norm(row)).astype(F)
            node_of[k] = o.k1["node_of"][i]
        xy2 = xy2.astype(F)
        ur2 = TR.uright_of(rng, xy2, z2, 0.4)
        T2, O2 = pose(R, t)
        k2 = dict(node_of=node_of, xy=xy2, ur=ur2, has=(rng.rand(n2) < 0.1).astype(np.uint8), desc=desc, Tcw=T2, Ow=O2)
        k2["depth"] = depth_of(k2)
        o.k2.append(k2); o.F12.append(Fm); o.ep.append(ep)
    return o


def planted_params():
    """mfScaleFactor = 5 / 6: the scale gate is [0.8, 1.25], which the neighbour's forward motion crosses for the nearest points;
    mvLevelSigma2[0] = 25: the gates are 12 and 14 px wide, so that the point KF1 unprojects at 50 m passes them in KF2"""
    return RG.params(CAM, sigma2=25.0, ratio_factor=1.25, scale_last=SCALE_LAST)


def planted(seed=4252, n1=65, n2=65):
    """B = 2, n1 = n2 = 65 with match12 written directly (i -> a permutation at neighbour 0) and causes planted into single pairs:
    pair 0: KF1 stereo with depth 0 and a ray parallel to its partner's -> the stereo branch, STEREO_NO_DEPTH
    pair 1: a NaN x in KF2 (mono): cosRays is NaN, no branch is taken -> LOW_PARALLAX; pair 2: a NaN uright in KF1: not stereo
    pair 3: KF1 stereo at 50 m (its stereo cosine then lies 1.2e-6 below 1), its partner's ray parallel -> unprojected from KF1, ACCEPTED at neighbour 0.  Neighbour 1 is neighbour 0 again with
            its centre Ow2 REPLACED by that point and only pairs 3 and 8 matched -> dist2 == 0, ZERO_DIST
    pairs 4, 5: two keypoints of KF1 matched to the same keypoint of KF2;  pair 6: the rays meet behind both cameras -> BEHIND1
    pair 7: a point between the two cameras, the neighbour standing in front of KF1 and seeing its mirror image -> BEHIND2
    pair 9: as pair 3 but at 10 m: exact in KF1, tens of pixels off in KF2 -> REPROJ2
    every seventh pair from 14 on is 40 px off in KF2 -> REPROJ1 / REPROJ2
    -> (scene, match12[2][n1]); its parameters are planted_params()"""
    o = small_scene(seed, n1, n2, 1)
    k1, k2 = o.k1, o.k2[0]
    perm = np.random.RandomState(seed).permutation(n2)
    m = np.full((2, n1), -1, np.int32)
    R, t = k2["Tcw"].reshape(3, 4)[:, :3].astype(np.float64), k2["Tcw"].reshape(3, 4)[:, 3].astype(np.float64)
    assert t[2] < -0.1, "the seed must put the neighbour in front of KF1"
    X = np.stack([(k1["xy"][:, 0] - CAM["cx"]) / CAM["fx"], (k1["xy"][:, 1] - CAM["cy"]) / CAM["fy"], np.ones(n1)], 1)
    for i in range(n1):                                                    # every keypoint of KF1 seen again: its own point at 2 .. 9 m
        z = {0: 1e7, 3: 1e7, 9: 1e7, 6: -5.0, 7: -t[2] / 2}.get(i, 2.0 + 7.0 * ((i * 37) % 65) / 65.0)          # (pairs 0, 3, 9: KF2's ray is parallel to KF1's)
        k = int(perm[i])
        X2 = R @ (X[i] * z) + t
        k2["xy"][k] = (TR.project(X2[None])[0] + (0.0 if i < 14 else [0.3 * np.sin(i), 40.0 * (i % 7 == 0)])).astype(F)
        if i in (6, 7):
            k1["ur"][i] = k2["ur"][k] = F(-1)
        if k1["ur"][i] >= 0:
            k1["ur"][i] = F(k1["xy"][i, 0]) - F(CAM["bf"]) / F(z); k1["depth"][i] = F(z)
        if k2["ur"][k] >= 0:
            k2["ur"][k] = k2["xy"][k, 0] - F(CAM["bf"]) / F(X2[2]); k2["depth"][k] = F(X2[2])
        m[0, i] = k
    for i, zi in ((0, 50.0), (3, 50.0), (9, 10.0)):                                                # KF1 measures 50 m there: unprojected, the point reprojects some pixels off in KF2
        k1["ur"][i] = F(k1["xy"][i, 0]) - F(CAM["bf"]) / F(zi); k1["depth"][i] = F(zi); k2["ur"][perm[i]] = F(-1)
    k1["depth"][0] = F(0)
    k2["ur"][perm[1]] = F(-1); k2["xy"][perm[1], 0] = np.nan
    k1["ur"][2] = np.nan
    m[0, 5] = m[0, 4]
    r = RG.pair_rule(planted_params(), RG.obs(k1, 3), RG.obs(k2, int(m[0, 3])))
    assert r["kind"] == 1 and r["status"] == RG.ACCEPTED
    o.k2.append(dict(k2, Ow=r["x3D"].copy())); o.F12.append(o.F12[0]); o.ep.append(o.ep[0])
    m[1, 3], m[1, 8] = m[0, 3], m[0, 8]
    return o, m


# ---- hand-made pairs with written-out answers: K = (512, 512, 320, 240), bf = 40, KF1 at the origin -------------------------------------------------
HCAM = dict(fx=512.0, fy=512.0, cx=320.0, cy=240.0, bf=40.0)
I34 = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F)


def handmade():
    """-> list of (name, o1, o2, kwargs of params, want) with want = dict(status, kind and, where it is exact, x3D)"""
    kp = lambda x, y, ur=-1.0, depth=-1.0, T=I34, Ow=(0, 0, 0), raw=None: dict(x=F(x), y=F(y), xr=F(x if raw is None else raw[0]), yr=F(y if raw is None else raw[1]),
                                                                             ur=F(ur), depth=F(depth), T=np.asarray(T, F), Ow=np.asarray(Ow, F))
    T2 = np.array([1, 0, 0, -1, 0, 1, 0, 0, 0, 0, 1, 0], F)                # the neighbour one metre to the right: Ow2 = (1, 0, 0)
    c = []
    # the point (0.5, 0, 4): x1 = 320 + 512 * 0.5 / 4 = 384, x2 = 320 - 64 = 256: every number a power of two, the answer exact in any arithmetic
    c.append(("two views, exact", kp(384, 240), kp(256, 240, T=T2, Ow=(1, 0, 0)), {}, dict(status=RG.ACCEPTED, kind=0, x3D=(0.5, 0, 4), tol=1)))
    c.append(("far gate", kp(384, 240), kp(256, 240, T=T2, Ow=(1, 0, 0)), dict(far_th=4.0), dict(status=RG.FAR, kind=0)))
    c.append(("y off by 3 px in KF2: 1.5 px in each view", kp(384, 240), kp(256, 243, T=T2, Ow=(1, 0, 0)), {}, dict(status=RG.ACCEPTED, kind=0)))
    c.append(("y off by 8 px", kp(384, 240), kp(256, 248, T=T2, Ow=(1, 0, 0)), {}, dict(status=RG.REPROJ1, kind=0)))
    # disparity of the wrong sign: the rays meet behind both cameras
    c.append(("behind", kp(256, 240), kp(384, 240, T=T2, Ow=(1, 0, 0)), {}, dict(status=RG.BEHIND1, kind=0)))
    # identical rays, no stereo: cosRays = 1
    c.append(("no parallax", kp(384, 240), kp(384, 240, T=T2, Ow=(1, 0, 0)), {}, dict(status=RG.LOW_PARALLAX, kind=0)))
    # KF1 stereo, depth 4 (uright = 384 - 40 / 4), the partner on the same ray direction: unprojected from the RAW key (400, 240) -> (0.625, 0, 4)
    c.append(("stereo of KF1, raw key", kp(384, 240, 374, 4, raw=(400, 240)), kp(384, 240, T=T2, Ow=(1, 0, 0)), {}, dict(status=RG.REPROJ1, kind=1, x3D=(0.625, 0, 4), tol=0)))
    c.append(("stereo of KF1", kp(384, 240, 374, 4), kp(256, 240, T=T2, Ow=(1, 0, 0)), dict(sigma2=1e6), dict(status=RG.ACCEPTED, kind=0)))
    c.append(("stereo of KF1 at no parallax", kp(384, 240, 374, 4), kp(384, 240, T=T2, Ow=(1, 0, 0)), dict(sigma2=1e9), dict(status=RG.ACCEPTED, kind=1, x3D=(0.5, 0, 4), tol=0)))
    c.append(("stereo of KF2 at no parallax", kp(384, 240), kp(384, 240, 374, 4, T=T2, Ow=(1, 0, 0)), dict(sigma2=1e9), dict(status=RG.ACCEPTED, kind=2, x3D=(1.5, 0, 4), tol=0)))
    c.append(("both stereo: only KF1's cosine is computed", kp(384, 240, 374, 4), kp(384, 240, 383, 40, T=T2, Ow=(1, 0, 0)), dict(sigma2=1e9),
              dict(status=RG.ACCEPTED, kind=1, x3D=(0.5, 0, 4), tol=0)))
    c.append(("stereo without depth", kp(384, 240, 374, 0), kp(384, 240, T=T2, Ow=(1, 0, 0)), {}, dict(status=RG.STEREO_NO_DEPTH, kind=1)))
    c.append(("scale: the neighbour four times nearer", kp(320, 240), kp(320 - 512, 240, T=np.array([1, 0, 0, -1, 0, 1, 0, 0, 0, 0, 1, -3], F), Ow=(1, 0, 3)), dict(sigma2=1e9),
              dict(status=RG.SCALE, kind=0)))
    c.append(("zero distance: Ow2 named as the point", kp(384, 240, 374, 4), kp(384, 240, T=T2, Ow=(0.5, 0, 4)), dict(sigma2=1e9), dict(status=RG.ZERO_DIST, kind=1)))
    # column 2 of A is exactly zero (poses may hold anything): xn1 = (2^-6, 0, 1), xn2 = (2^-4, 0, 1), T[0][2] = xn[0] -> x3Dh = (0, 0, 1, 0)
    Ta = np.array([1, 0, 2.0 ** -6, 0, 0, 1, 0, 0, 0, 0, 1, 0], F); Tb = np.array([1, 0, 2.0 ** -4, -0.5, 0, 1, 0, 0.125, 0, 0, 1, 0], F)
    c.append(("w == 0", kp(328, 240, T=Ta), kp(352, 240, T=Tb, Ow=(0.5, -0.125, 0)), {}, dict(status=RG.DEGENERATE, kind=0)))
    c.append(("NaN key in KF2", kp(384, 240), kp(np.nan, 240, T=T2, Ow=(1, 0, 0)), {}, dict(status=RG.LOW_PARALLAX, kind=0)))
    c.append(("NaN pose column: the point is NaN and passes every gate", kp(384, 240, 374, 4, Ow=(np.nan, 0, 0)), kp(384, 240, T=T2, Ow=(1, 0, 0)), {},
              dict(status=RG.ACCEPTED, kind=1)))
    c.append(("inertial: 0.9997 is low parallax only there", kp(320, 240), kp(320 - 12.5, 240, T=np.array([1, 0, 0, -0.0977, 0, 1, 0, 0, 0, 0, 1, 0], F), Ow=(0.0977, 0, 0)),
              dict(inertial=True), dict(status=RG.LOW_PARALLAX, kind=0)))
    return c


class TriangRig:
    """one guarded run of xfh_triangulate_device"""

    def __init__(self, L):
        self.L, self.ctx = L, Context(nfeatures=1, max_height=32, max_width=32)
        self.bufs = []

    def close(self):
        self.free()
        self.ctx.close()

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []

    def dev(self, a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        b = capi.DeviceBuffer(max(a.nbytes, 16)).upload(a)
        self.bufs.append(b)
        return b.ptr

    def side(self, ks):
        return [self.dev(a) for a in Context._triang_side(ks, len(ks))]

    def run(self, cam, side1, k2s, match12, P, claim=True, d_match12=None):
        """side1: ONE keyframe (shared) or B of them.  P: RG.params.  -> (parsed outputs, raw bytes)"""
        B, n1, n2 = len(k2s), len(side1[0]["xy"]), len(k2s[0]["xy"])
        shared = len(side1) == 1
        lay = Context.triangulate_layout(B, n1, GUARD)
        out = guarded.outputs(lay)
        dm = d_match12 if d_match12 is not None else self.dev(np.ascontiguousarray(match12, np.int32))
        self.ctx.triangulate_device(B, n1, n2, shared, cam, self.side(side1), self.side(k2s), dm, out.ptr, sigma2=P["sigma2"], ratio_factor=P["ratio_factor"],
                                    scale_last=P["scale_last"], far_th=P["far_th"], inertial=P["inertial"], claim=claim, guard=GUARD)
        self.ctx.synchronize()
        raw = guarded.download(out, lay, skip=() if claim else Context.TRIANG_CLAIM_OUT)
        out.free(); self.free()
        return Context.triangulate_parse(raw, lay, B, n1, claim), raw


def assert_equals_rule(got, want, claim=True):
    """integers equal, floats by bits"""
    for k in ("status", "kind", "header") + (("winner", "new_idx1", "new_b", "new_idx2") if claim else ()):
        assert np.array_equal(got[k], want[k]), (k, np.argwhere(np.asarray(got[k]) != np.asarray(want[k]))[:8])
    for k in ("xyz",) + (("new_xyz", "new_normal", "new_dist") if claim else ()):
        g, w = np.ascontiguousarray(got[k], F).view(np.int32), np.ascontiguousarray(want[k], F).view(np.int32)
        assert np.array_equal(g, w), (k, np.argwhere(g != w)[:8], RG.ulps(got[k], want[k]).max())
    if claim:
        assert got["n_new"] == want["n_new"]
