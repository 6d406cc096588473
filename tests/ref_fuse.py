"""numpy fp32 restatement of the search of ORBmatcher::Fuse (src/ORBmatcher.cc:1333-1523, the SE3 form; :1525-1640, the Sim3 form) as
include/xfeat_hip.h states it: one query at a time, written from the reference's lines (test infrastructure, no GPU; shares no code
with the library).

  predict_level   MapPoint::PredictScale (src/MapPoint.cc:514-529) DIRECTLY: ceilf(logf(ratio) / logf(scale_factor)) with the logf and
                  ceilf of this process's libm through ctypes (numpy has its own float log), then the clamp of :523-526.  It does not
                  know the library's threshold table: the table is tested against this expression.
  project         :1383-1429: x3Dc from a row-major 3x4 [R|t], the depth test on zc, invz = 1.0f / zc, Pinhole::project,
                  KeyFrame::IsInImage (KeyFrame.cc:750-753), the distance range, the 60 degree test in double, the level, the radius
  search          :1431-1497 per query: KeyFrame::GetFeaturesInArea (ref_window.features_in_area), the level window :1454, the
                  chi-square gates :1457-1481, DescriptorDistance with the oracle's best2_csr, bestDist <= TH_LOW
  scene           the seeded inputs of the tests: normals, distances and flags for world points

Every fp32 expression is evaluated in np.float32 in the written order (numpy never contracts a multiply and an add).
"""
import ctypes
import ctypes.util

import numpy as np

import ref_window as RW

F = np.float32
D = np.float64
INACTIVE, BEHIND, OUT_OF_IMAGE, OUT_OF_RANGE, BAD_ANGLE, NO_CANDIDATES, REJECTED, FUSED = range(8)
VISIBLE = NO_CANDIDATES                                     # what the projection stage calls a point that reaches the search
TH_LOW = 100
INT_MAX = 0x7fffffff

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = ctypes.c_float; _libm.logf.argtypes = [ctypes.c_float]
_libm.ceilf.restype = ctypes.c_float; _libm.ceilf.argtypes = [ctypes.c_float]


def logf(x):
    return F(_libm.logf(ctypes.c_float(float(F(x)))))


def predict_level(ratio, scale_factor, nlevels):
    """MapPoint.cc:522-526 with the float overloads; where (int) of the quotient is undefined (NaN, +-Inf) the contract's answers"""
    with np.errstate(all="ignore"):
        q = F(_libm.ceilf(ctypes.c_float(float(logf(ratio) / logf(scale_factor)))))
    if np.isnan(q):
        return 0
    if q < 0:
        return 0
    if q >= nlevels:
        return nlevels - 1
    return int(q)


def scale_factors(scale_factor, nlevels):
    """mvScaleFactor (XFextractor.cc:80-96): a running fp32 product"""
    sf = np.ones(nlevels, F)
    for i in range(1, nlevels):
        sf[i] = F(sf[i - 1] * F(scale_factor))
    return sf


def project(T, Ow, cam, bounds, th, scale_factor, nlevels, xyz, normals, dist):
    """-> u, v, ur, r (fp32 arrays), level (int32), status (BEHIND .. BAD_ANGLE or VISIBLE).  BEHIND: u = v = ur = 0; every culled point
    has level -1 and r = 0.  dist[i] = (min_distance, max_distance, predict_distance)."""
    T = np.asarray(T, F).reshape(12); Ow = np.asarray(Ow, F).reshape(3)
    p = np.asarray(xyz, F).reshape(-1, 3); nr = np.asarray(normals, F).reshape(-1, 3); dd = np.asarray(dist, F).reshape(-1, 3)
    n = len(p)
    fx, fy, cx, cy, bf = (F(cam[k]) for k in ("fx", "fy", "cx", "cy", "bf"))
    mnx, mny, mxx, mxy = (F(b) for b in bounds)
    sf = scale_factors(scale_factor, nlevels)
    u = np.zeros(n, F); v = np.zeros(n, F); ur = np.zeros(n, F); r = np.zeros(n, F)
    level = np.full(n, -1, np.int32); st = np.zeros(n, np.uint8)
    with np.errstate(all="ignore"):
        for i in range(n):
            X, Y, Z = p[i]
            xc = ((T[0] * X + T[1] * Y) + T[2] * Z) + T[3]
            yc = ((T[4] * X + T[5] * Y) + T[6] * Z) + T[7]
            zc = ((T[8] * X + T[9] * Y) + T[10] * Z) + T[11]
            if zc < F(0):                                                                    # :1387
                st[i] = BEHIND
                continue
            invz = F(1) / zc                                                                 # :1393
            u[i] = (fx * xc) / zc + cx; v[i] = (fy * yc) / zc + cy                           # Pinhole.cpp:45-46
            ur[i] = u[i] - bf * invz                                                         # :1404
            if not (u[i] >= mnx and u[i] < mxx and v[i] >= mny and v[i] < mxy):              # KeyFrame.cc:752
                st[i] = OUT_OF_IMAGE
                continue
            po = p[i] - Ow
            d3 = np.sqrt((po[0] * po[0] + po[1] * po[1]) + po[2] * po[2], dtype=F)
            if d3 < dd[i, 0] or d3 > dd[i, 1]:                                               # :1412
                st[i] = OUT_OF_RANGE
                continue
            dot = (po[0] * nr[i, 0] + po[1] * nr[i, 1]) + po[2] * nr[i, 2]
            if D(dot) < D(0.5) * D(d3):                                                      # :1420
                st[i] = BAD_ANGLE
                continue
            level[i] = predict_level(dd[i, 2] / d3, scale_factor, nlevels)                   # :1426
            r[i] = F(th) * sf[level[i]]                                                      # :1429
            st[i] = VISIBLE
    return u, v, ur, r, level, st


def chi2_skips(u, v, ur, xk, yk, urk):
    """:1457-1481 with kpLevel = 0 and mvInvLevelSigma2[0] = 1.0f; arrays over the candidates"""
    with np.errstate(all="ignore"):
        ex = F(u) - xk; ey = F(v) - yk
        er = F(ur) - urk
        stereo = urk >= 0
        e2s = (ex * ex + ey * ey) + er * er
        e2m = ex * ex + ey * ey
        return np.where(stereo, e2s.astype(D) > 7.8, e2m.astype(D) > 5.99)


def search(O, status_in, level, u, v, r, ur, qdesc, grid, x, y, bounds, tg, uright=None, chi2=True, init_dist=256, th_low=TH_LOW):
    """the loop over the queries.  status_in[q] == VISIBLE: the query reaches the search; anything else is kept.  O: the oracle module."""
    nq, nt = len(qdesc), len(tg)
    x = np.asarray(x, F); y = np.asarray(y, F)
    urk_all = np.full(nt, -1, F) if uright is None else np.asarray(uright, F)
    status = np.asarray(status_in, np.uint8).copy()
    best_idx = np.full(nq, -1, np.int32); best = np.full(nq, init_dist, np.int32)
    n_window = np.zeros(nq, np.int32); n_tested = np.zeros(nq, np.int32)
    n_fused = 0
    for q in range(nq):
        if status[q] != VISIBLE:
            continue
        c = RW.features_in_area(grid, x, y, u[q], v[q], r[q], bounds)                         # :1431
        n_window[q] = len(c)
        if len(c) == 0:                                                                      # :1433
            status[q] = NO_CANDIDATES
            continue
        if level[q] > 1:                                                                     # :1454, kpLevel = 0
            c = c[:0]
        elif chi2:
            c = c[~chi2_skips(u[q], v[q], ur[q], x[c], y[c], urk_all[c])]
        n_tested[q] = len(c)
        if len(c):
            bi, bd, _, _ = (int(a[0]) for a in O.best2_csr(qdesc[q:q + 1], tg, np.array([0, len(c)], np.int32), c, init_dist))
            best_idx[q] = bi; best[q] = bd
        if best_idx[q] >= 0 and best[q] <= th_low:                                           # :1497
            status[q] = FUSED; n_fused += 1
        else:
            status[q] = REJECTED
    return dict(status=status, best_idx=best_idx, best_dist=best, n_window=n_window, n_tested=n_tested, n_fused=n_fused)


def camera_centre(T):
    """Ow = -R^T t of a row-major 3x4 pose, in float64 and rounded once"""
    T = np.asarray(T, D).reshape(3, 4)
    return (-T[:, :3].T @ T[:, 3]).astype(F)


def scene(seed, xy_last, cam, T, ratio_max=None, inactive=0.1, kf=None):
    """the seeded map points of the tests: the last frame's keypoints back-projected at a seeded depth of 1.9 .. 2.3 m (its camera frame
    is the world frame; 3 % behind the camera, 3 % pushed out of the image; with kf, see below), normals towards the camera centre of pose T, 6 % of
    them turned past 60 degrees; predict_distance = ratio * dist3D with the ratio spread over 0.8 .. 2.1 (levels 0 .. 4 at scale
    factor 1.2) and, where ratio_max is given, every 16th query ON a threshold or its successor; min / max distance = 0.8f / 1.2f
    times a range around it, 4 % of them excluding the point; flags with about 10 % inactive
    -> xyz[n][3], normals[n][3], dist[n][3], flags[n]"""
    rng0 = np.random.RandomState(seed)
    xy = np.asarray(xy_last, F).reshape(-1, 2)
    z = rng0.uniform(1.9, 2.3, len(xy)).astype(F)
    z[rng0.rand(len(xy)) < 0.03] *= F(-1)
    p = np.stack([(xy[:, 0] - F(cam["cx"])) / F(cam["fx"]) * z, (xy[:, 1] - F(cam["cy"])) / F(cam["fy"]) * z, z], 1).astype(F)
    if kf is not None:
        # kf = (x, y, uright) of the keyframe: a point that projects within 3 pixels of a stereo keypoint is moved along its ray to that
        # keypoint's depth bf / (x - uright) (where that lies in 1 .. 60 m; 95 % of them), so that the stereo chi-square gate has candidates it keeps
        kx, ky, kur = (np.asarray(a, D) for a in kf)
        Td = np.asarray(T, D).reshape(3, 4)
        pc = p.astype(D) @ Td[:, :3].T + Td[:, 3]
        with np.errstate(all="ignore"):
            pu = float(cam["fx"]) * pc[:, 0] / pc[:, 2] + float(cam["cx"]); pv = float(cam["fy"]) * pc[:, 1] / pc[:, 2] + float(cam["cy"])
        take = rng0.rand(len(xy)) < 0.95
        for i in np.nonzero(take & (z > 0))[0]:
            e2 = (kx - pu[i]) ** 2 + (ky - pv[i]) ** 2
            k = int(e2.argmin())
            if e2[k] < 9.0 and kur[k] >= 0:
                zk = float(cam["bf"]) / (kx[k] - kur[k])
                if 1.0 < zk < 60.0:
                    p[i] = (p[i].astype(D) * (zk / float(z[i]))).astype(F)
    p[rng0.rand(len(xy)) < 0.03, 0] *= F(3)
    astray = rng0.rand(len(xy)) < 0.15                                   # off its keypoint by about 10 .. 80 pixels: windows without members
    p[astray, 1] += (rng0.uniform(0.02, 0.15, len(xy)).astype(F) * p[:, 2])[astray]
    Ow = camera_centre(T)
    rng = np.random.RandomState(seed + 11)
    n = len(p)
    po = p - np.asarray(Ow, F)
    with np.errstate(all="ignore"):
        d3 = np.sqrt((po[:, 0] * po[:, 0] + po[:, 1] * po[:, 1]) + po[:, 2] * po[:, 2], dtype=F)
    nr = po / np.maximum(d3, F(1e-6))[:, None]
    tilt = rng.uniform(0.0, 0.9, n)                                      # radians; beyond 60 degrees (1.047) for the turned ones
    turned = rng.rand(n) < 0.06
    tilt[turned] = rng.uniform(1.0, 1.5, int(turned.sum()))
    axis = np.cross(nr, rng.randn(n, 3)); axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    nr = (nr * np.cos(tilt)[:, None] + np.cross(axis, nr) * np.sin(tilt)[:, None]).astype(F)
    ratio = np.exp(rng.uniform(np.log(0.8), np.log(2.1), n)).astype(F)
    ratio[rng.rand(n) < 0.6] = F(1.1)                                   # most points at level 1, where the search is live
    ratio[rng.rand(n) < 0.3] = F(0.95)                                  # and at level 0
    ratio[astray] = F(0.95)                                              # (level 0: the smallest window)
    pd = (ratio * d3).astype(F)
    if ratio_max is not None and len(ratio_max):
        # predict_distance whose fp32 quotient by dist3D IS the threshold (or its successor) where such a value exists
        for j in range(0, n, 16):
            t = F(ratio_max[(j // 16) % min(len(ratio_max), 3)])
            if (j // 16) % 2:
                t = np.nextafter(t, F(np.inf))
            for cand in (F(t * d3[j]), np.nextafter(F(t * d3[j]), F(np.inf)), np.nextafter(F(t * d3[j]), F(0))):
                if F(cand / d3[j]) == t:
                    pd[j] = cand
                    break
    lo = (F(0.8) * (pd * F(0.4))).astype(F); hi = (F(1.2) * pd).astype(F)
    far = rng.rand(n) < 0.04
    hi[far] = (d3[far] * F(0.9)).astype(F)                                # the point lies beyond the range
    dist = np.stack([lo, hi, pd], 1).astype(F)
    flags = (rng.rand(n) >= inactive).astype(np.uint8)
    return p, nr, dist, flags


def coords_with_e2(target, u=100.0, v=100.0):
    """keypoint coordinates (x_k, y_k) near (u, v) for which the fp32 expression (u - x_k)^2 + (v - y_k)^2 is EXACTLY `target`
    (u, v in [64, 128): their differences with neighbours on the 2^-17 grid are exact)"""
    target = F(target); step = F(2.0 ** -17)
    ex = (np.floor(np.sqrt(D(target) - 0.001) / D(step)) + np.arange(0, 64))[:, None].astype(F) * step
    ey = np.arange(0, 6000)[None, :].astype(F) * step
    e2 = (ex * ex + ey * ey).astype(F)
    i, j = np.nonzero(e2 == target)
    assert len(i), target
    xk, yk = F(F(u) - ex[i[0], 0]), F(F(v) - ey[0, j[0]])
    assert F(u) - xk == ex[i[0], 0] and F(v) - yk == ey[0, j[0]]
    return xk, yk


# ---- hand-made cases: a camera with fx = fy = 1, cx = cy = 0 and the identity pose project (X, Y, 1) to (u, v) = (X, Y) exactly, ur = u - 40
UNIT_CAM = dict(fx=F(1), fy=F(1), cx=F(0), cy=F(0), k1=F(0), k2=F(0), p1=F(0), p2=F(0), k3=F(0), bf=F(40), width=640, height=480)
B640 = (0.0, 0.0, 640.0, 480.0)
I34 = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F)


def line_descriptors(values):
    """descriptors on one axis: DescriptorDistance(a, b) = (int)(512 * (a - b)^2) in fp32"""
    d = np.zeros((len(values), 64), F)
    d[:, 0] = values
    return d


def below_and_above(t):
    """the two neighbouring floats a < t < b of a double t that is no float"""
    a = F(t)
    if float(a) > t:
        a = np.nextafter(a, F(0))
    return a, np.nextafter(a, F(np.inf))


def tiny(cands, queries, th=3.0, chi2=True, init_dist=256, scale_factor=1.2, nlevels=8):
    """cands: (x, y, uright, descriptor value) per keypoint; queries: (u, v, descriptor value, ratio) -- the query sits at (u, v, 1)
    with the normal along its viewing ray and predict_distance = ratio * dist3D -> the inputs of one problem as a dict"""
    c = np.asarray(cands, D).reshape(-1, 4); q = np.asarray(queries, D).reshape(-1, 4)
    xyz = np.stack([q[:, 0], q[:, 1], np.ones(len(q))], 1).astype(F)
    d3 = np.sqrt((xyz[:, 0] * xyz[:, 0] + xyz[:, 1] * xyz[:, 1]) + xyz[:, 2] * xyz[:, 2], dtype=F)
    dist = np.stack([np.zeros(len(q), F), np.full(len(q), np.inf, F), (q[:, 3].astype(F) * d3).astype(F)], 1)
    return dict(xyz=xyz, normals=xyz.copy(), dist=dist, qdesc=line_descriptors(q[:, 2]), flags=np.ones(len(q), np.uint8), T=I34, Ow=np.zeros(3, F),
                cam=UNIT_CAM, bounds=B640, th=th, scale_factor=scale_factor, nlevels=nlevels, x=c[:, 0].astype(F), y=c[:, 1].astype(F),
                uright=c[:, 2].astype(F), tg=line_descriptors(c[:, 3]), chi2=chi2, init_dist=init_dist)


def run_case(O, k):
    """the restatement on the inputs of tiny() (or any dict of that shape) -> the result dict of search() plus level and proj"""
    u, v, ur, r, level, st = project(k["T"], k["Ow"], k["cam"], k["bounds"], k["th"], k["scale_factor"], k["nlevels"], k["xyz"], k["normals"], k["dist"])
    st = np.where(k["flags"] & 1, st, INACTIVE).astype(np.uint8)
    m = search(O, st, level, u, v, r, ur, k["qdesc"], RW.build(k["x"], k["y"], k["bounds"]), k["x"], k["y"], k["bounds"], k["tg"], uright=k["uright"],
               chi2=k["chi2"], init_dist=k["init_dist"])
    act = (k["flags"] & 1) != 0
    m["level"] = np.where(act, level, -1).astype(np.int32)
    m["proj"] = np.where(act[:, None], np.stack([u, v, ur], 1), F(0)).astype(F)
    return m


def handmade():
    """(name, inputs, expected) of the boundary cases tests/test_fuse_ref.py writes out; expected: dict of lists per output"""
    cases = []
    a599, b599 = below_and_above(5.99); a78, b78 = below_and_above(7.8)
    # e2 one ulp either side of 5.99 (monocular: uright = -1) and of 7.8 (stereo: uright = 60 = ur, er = 0); the skipped one is the nearer descriptor
    for name, (lo, hi), urk in (("chi2 mono 5.99", (a599, b599), -1.0), ("chi2 stereo 7.8", (a78, b78), 60.0)):
        (x0, y0), (x1, y1) = coords_with_e2(lo), coords_with_e2(hi)
        k = tiny([(x0, y0, urk, 0.3), (x1, y1, urk, 0.0)], [(100, 100, 0.0, 1.0)])
        cases.append((name, k, dict(status=[FUSED], best_idx=[0], best_dist=[46], n_window=[2], n_tested=[1], level=[0])))
        k = tiny([(x0, y0, urk, 0.3), (x1, y1, urk, 0.0)], [(100, 100, 0.0, 1.0)], chi2=False)
        cases.append((name + " off", k, dict(status=[FUSED], best_idx=[1], best_dist=[0], n_window=[2], n_tested=[2], level=[0])))
    # uright = 0 is a stereo keypoint (0 >= 0): er = 60, skipped; -1 is monocular; 59 is stereo with er = 1
    k = tiny([(100, 100, 0.0, 0.0), (101, 100, -1.0, 0.1), (100, 101, 59.0, 0.3)], [(100, 100, 0.0, 1.0)])
    cases.append(("uright -1 / 0 / positive", k, dict(status=[FUSED], best_idx=[1], best_dist=[5], n_window=[3], n_tested=[2], level=[0])))
    # two equal descriptors: slot 1 lies in grid column 9 (x = 94.5), slot 0 in column 10 (x = 95.5): slot 1 is visited first and keeps the tie
    k = tiny([(95.5, 100, -1.0, 0.1), (94.5, 100, -1.0, 0.1)], [(95, 100, 0.0, 1.0)])
    cases.append(("tie goes to the first visited", k, dict(status=[FUSED], best_idx=[1], best_dist=[5], n_window=[2], n_tested=[2], level=[0])))
    # best exactly TH_LOW and one above
    k = tiny([(100, 100, -1.0, 0.4425)], [(100, 100, 0.0, 1.0)])
    cases.append(("best 100", k, dict(status=[FUSED], best_idx=[0], best_dist=[100], n_window=[1], n_tested=[1], level=[0])))
    k = tiny([(100, 100, -1.0, 0.4445)], [(100, 100, 0.0, 1.0)])
    cases.append(("best 101", k, dict(status=[REJECTED], best_idx=[0], best_dist=[101], n_window=[1], n_tested=[1], level=[0])))
    # a best of 300: no candidate under 256 in the SE3 form, a candidate (still rejected) with INT_MAX
    k = tiny([(100, 100, -1.0, 0.766)], [(100, 100, 0.0, 1.0)])
    cases.append(("best 300 init 256", k, dict(status=[REJECTED], best_idx=[-1], best_dist=[256], n_window=[1], n_tested=[1], level=[0])))
    k = tiny([(100, 100, -1.0, 0.766)], [(100, 100, 0.0, 1.0)], chi2=False, init_dist=INT_MAX)
    cases.append(("best 300 init INT_MAX", k, dict(status=[REJECTED], best_idx=[0], best_dist=[300], n_window=[1], n_tested=[1], level=[0])))
    # levels: 1 widens the radius to 1.2f * th (x = 103.5 is inside 3.6, outside 3); 2 and above test no candidate but count the window
    k = tiny([(103.5, 100, -1.0, 0.0)], [(100, 100, 0.0, 1.0), (100, 100, 0.0, 1.1), (100, 100, 0.0, 1.3), (100, 100, 0.0, 100.0)], chi2=False)
    cases.append(("levels 0 1 2 7", k, dict(status=[NO_CANDIDATES, FUSED, REJECTED, REJECTED], best_idx=[-1, 0, -1, -1], best_dist=[256, 0, 256, 256],
                                            n_window=[0, 1, 1, 1], n_tested=[0, 1, 0, 0], level=[0, 1, 2, 7])))
    return cases


def query_descriptors(seed, u, v, x, y, tg, own):
    """the map points' descriptors.  The synthetic weights' descriptors of ONE scene point in two frames are several hundred apart
    (tests/test_fuse_ref.py prints the figures), so with the last frame's own rows nothing would come under TH_LOW = 100.  A map point's
    descriptor is the most distinctive of its observations (MapPoint::ComputeDistinctiveDescriptors), and a point worth fusing HAS been
    observed near the spot: a query whose projection (u, v) has a keyframe keypoint within 2.4 pixels takes that keypoint's row plus
    seeded noise of four strengths (DescriptorDistance about 0, 13, 50 and 160, the third twice as often); one in seven takes instead the row of a keypoint
    inside the 2.9 pixel square but beyond the mono chi-square bound, so that the gate changes its answer; the others keep `own`."""
    rng = np.random.RandomState(seed + 23)
    q = np.array(own, F, copy=True)
    x = np.asarray(x, D); y = np.asarray(y, D)
    for i in range(len(q)):
        pick, sigma, other = rng.rand(), (0.0, 0.02, 0.04, 0.04, 0.07)[rng.randint(5)], rng.rand(64 + 1)
        if not (np.isfinite(u[i]) and np.isfinite(v[i])):
            continue
        dx = x - D(u[i]); dy = y - D(v[i]); e2 = dx * dx + dy * dy
        k = -1
        if pick < 1 / 7:
            c = np.nonzero((np.abs(dx) < 2.9) & (np.abs(dy) < 2.9) & (e2 > 6.5))[0]
            if len(c):
                k, sigma = int(c[int(other[64] * len(c))]), 0.0
        if k < 0 and e2.min() < 2.4 * 2.4:
            k = int(e2.argmin())
        if k >= 0:
            row = np.asarray(tg[k], D) + sigma * (other[:64] - 0.5) * np.sqrt(12.0)
            q[i] = (row / np.linalg.norm(row)).astype(F)
    return q
