"""Restatement of the triangulation half of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:434-710, conventional Pinhole
keyframes) with GeometricTools::Triangulate (src/GeometricTools.cc:47-66), KeyFrame::UnprojectStereo (src/KeyFrame.cc:755-772) and
MapPoint::UpdateNormalAndDepth for two observations (src/MapPoint.cc:426-494), in two forms:

  literal()   the loop over the neighbours as the reference runs it: SearchForTriangulation per neighbour (ref_triangulation.literal) with has1
              updated as points are created, every float operation a numpy fp32 scalar operation, cos(2 * atan2(mb / 2, depth)) with numpy's
              float32 functions, and the null vector from LAPACK's float32 SVD of the float32 A (lapack_null_vector).  That SVD is LAPACK's,
              NOT Eigen's JacobiSVD: the reference's own rounding cannot be had here, LAPACK's float32 error stands in for it.
  rule()      the contract of xfh_triangulate_device (include/xfeat_hip.h): one snapshot search for all neighbours (ref_triangulation.order_free),
              the per-pair rule with the cosine identity and the fp64 one-sided Jacobi null vector, the first accepted neighbour wins, the compact
              list in creation order.  pair_rule() is that per-pair rule alone, operation for operation what triangulate_math.h computes.

A keyframe is a dict(xy, xy_raw (optional), ur (or None), depth, Tcw [12], Ow [3]) beside the search's node_of / has / desc.  P = params(...).
No test lives here."""
import numpy as np

import ref_triangulation as RT

F, D = np.float32, np.float64
(NO_MATCH, LOW_PARALLAX, STEREO_NO_DEPTH, DEGENERATE, BEHIND1, BEHIND2, REPROJ1, REPROJ2, ZERO_DIST, FAR, SCALE, ACCEPTED, SUPERSEDED) = range(13)
NAMES = ("NO_MATCH", "LOW_PARALLAX", "STEREO_NO_DEPTH", "DEGENERATE", "BEHIND1", "BEHIND2", "REPROJ1", "REPROJ2", "ZERO_DIST", "FAR", "SCALE", "ACCEPTED",
         "SUPERSEDED")
MAX_SWEEPS, TOL = 30, D(1e-15)
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def params(cam, sigma2=1.0, ratio_factor=1.8, scale_last=1.0, far_th=0.0, inertial=False):
    """cam: dict(fx, fy, cx, cy, bf).  invfx, invfy, mb in float as Frame computes them"""
    p = {k: F(cam[k]) for k in ("fx", "fy", "cx", "cy", "bf")}
    with np.errstate(all="ignore"):
        p.update(invfx=F(1) / p["fx"], invfy=F(1) / p["fy"], mb=p["bf"] / p["fx"])
    p.update(sigma2=F(sigma2), ratio_factor=F(ratio_factor), scale_last=F(scale_last), far_th=F(far_th), inertial=bool(inertial))
    return p


def obs(k, i):
    """keypoint i of keyframe k -> what the rule reads"""
    raw = k.get("xy_raw")
    st = k.get("ur") is not None
    return dict(x=F(k["xy"][i][0]), y=F(k["xy"][i][1]), xr=F((k["xy"] if raw is None else raw)[i][0]), yr=F((k["xy"] if raw is None else raw)[i][1]),
                ur=F(k["ur"][i]) if st else F(-1), depth=F(k["depth"][i]) if st else F(-1), T=np.asarray(k["Tcw"], F).reshape(12), Ow=np.asarray(k["Ow"], F).reshape(3))


def dot3(a0, a1, a2, b0, b1, b2):
    return F(F(F(a0 * b0) + F(a1 * b1)) + F(a2 * b2))


def cos_identity(mb, depth):
    h, z = D(F(mb / F(2))), D(depth)
    return F((z * z - h * h) / (z * z + h * h))


def cos_libm(mb, depth):
    return F(np.cos(F(2) * np.arctan2(F(mb / F(2)), F(depth))))


def jacobi_null_vector(A):
    """the rule's fp64 null vector of the float32 4x4 A -> (x[4] float64, sweeps run)"""
    U = [[D(A[r][c]) for c in range(4)] for r in range(4)]
    V = [[D(1.0 if r == c else 0.0) for c in range(4)] for r in range(4)]
    col2 = lambda p, q: ((U[0][p] * U[0][q] + U[1][p] * U[1][q]) + U[2][p] * U[2][q]) + U[3][p] * U[3][q]
    sweeps = 0
    for _ in range(MAX_SWEEPS):
        sweeps += 1
        rot = 0
        for p, q in PAIRS:
            alpha, beta, gamma = col2(p, p), col2(q, q), col2(p, q)
            if not (np.abs(gamma) > TOL * np.sqrt(alpha * beta)):
                continue
            zeta = (beta - alpha) / (D(2.0) * gamma)
            t = (D(-1.0) if zeta < 0 else D(1.0)) / (np.abs(zeta) + np.sqrt(D(1.0) + zeta * zeta))
            c = D(1.0) / np.sqrt(D(1.0) + t * t)
            s = c * t
            for r in range(4):
                up, uq, vp, vq = U[r][p], U[r][q], V[r][p], V[r][q]
                U[r][p] = c * up - s * uq; U[r][q] = s * up + c * uq
                V[r][p] = c * vp - s * vq; V[r][q] = s * vp + c * vq
            rot += 1
        if rot == 0:
            break
    best, x = col2(0, 0), [V[r][0] for r in range(4)]
    for c in range(1, 4):
        n = col2(c, c)
        if n < best:
            best, x = n, [V[r][c] for r in range(4)]
    return np.array(x, D), sweeps


def lapack_null_vector(A, dtype=F):
    """V's last column from LAPACK's SVD of A in `dtype`.  float32 (the literal form) goes through scipy.linalg.svd, which calls sgesdd, a SVD
    carried out in float32; numpy.linalg.svd of a float32 matrix computes in double and rounds the result, which is the rule itself again and
    would measure nothing.  float64: numpy's dgesdd"""
    if dtype == F:
        import scipy.linalg
        return scipy.linalg.svd(np.asarray(A, F), lapack_driver="gesdd", check_finite=False)[2][3]
    return np.linalg.svd(np.asarray(A, dtype))[2][3]


def matrix_A(P, o1, o2):
    xn1 = (F(F(o1["x"] - P["cx"]) / P["fx"]), F(F(o1["y"] - P["cy"]) / P["fy"]))
    xn2 = (F(F(o2["x"] - P["cx"]) / P["fx"]), F(F(o2["y"] - P["cy"]) / P["fy"]))
    T1, T2 = o1["T"], o2["T"]
    A = np.zeros((4, 4), F)
    for c in range(4):
        A[0][c] = F(xn1[0] * T1[8 + c]) - T1[c]; A[1][c] = F(xn1[1] * T1[8 + c]) - T1[4 + c]
        A[2][c] = F(xn2[0] * T2[8 + c]) - T2[c]; A[3][c] = F(xn2[1] * T2[8 + c]) - T2[4 + c]
    return xn1, xn2, A


def unproject_stereo(P, o):
    z = o["depth"]
    if not (z > 0):
        return None
    x = F(F(F(o["xr"] - P["cx"]) * z) * P["invfx"]); y = F(F(F(o["yr"] - P["cy"]) * z) * P["invfy"])
    R = o["T"]
    return np.array([F(F(F(F(R[k] * x) + F(R[4 + k] * y)) + F(R[8 + k] * z)) + o["Ow"][k]) for k in range(3)], F)


def view_gate(P, o, stereo, X):
    """0 pass, 1 behind, 2 reprojection"""
    T = o["T"]
    z = F(dot3(T[8], T[9], T[10], X[0], X[1], X[2]) + T[11])
    if z <= 0:
        return 1
    x = F(dot3(T[0], T[1], T[2], X[0], X[1], X[2]) + T[3]); y = F(dot3(T[4], T[5], T[6], X[0], X[1], X[2]) + T[7])
    if not stereo:
        ex = F(F(F(F(P["fx"] * x) / z) + P["cx"]) - o["x"]); ey = F(F(F(F(P["fy"] * y) / z) + P["cy"]) - o["y"])
        return 2 if D(F(F(ex * ex) + F(ey * ey))) > D(5.991) * D(P["sigma2"]) else 0
    invz = F(D(1.0) / D(z))
    u = F(F(F(P["fx"] * x) * invz) + P["cx"]); ur = F(u - F(P["bf"] * invz)); v = F(F(F(P["fy"] * y) * invz) + P["cy"])
    ex, ey, er = F(u - o["x"]), F(v - o["y"]), F(ur - o["ur"])
    return 2 if D(F(F(F(ex * ex) + F(ey * ey)) + F(er * er))) > D(7.8) * D(P["sigma2"]) else 0


def dists(o1, o2, X):
    a = [F(X[k] - o1["Ow"][k]) for k in range(3)]; b = [F(X[k] - o2["Ow"][k]) for k in range(3)]
    return a, b, F(np.sqrt(dot3(*a, *a))), F(np.sqrt(dot3(*b, *b)))


def gates(P, o1, o2, st1, st2, X):
    """:612-691 on a 3-D point -> status"""
    with np.errstate(all="ignore"):
        g1 = view_gate(P, o1, st1, X)
        if g1 == 1:
            return BEHIND1
        T2 = o2["T"]
        if F(dot3(T2[8], T2[9], T2[10], X[0], X[1], X[2]) + T2[11]) <= 0:
            return BEHIND2
        if g1 == 2:
            return REPROJ1
        if view_gate(P, o2, st2, X) == 2:
            return REPROJ2
        _, _, d1, d2 = dists(o1, o2, X)
        if d1 == 0 or d2 == 0:
            return ZERO_DIST
        if P["far_th"] > 0 and (d1 >= P["far_th"] or d2 >= P["far_th"]):
            return FAR
        ratio = F(d2 / d1)
        if F(ratio * P["ratio_factor"]) < F(1) or ratio > F(F(1) * P["ratio_factor"]):
            return SCALE
        return ACCEPTED


def normal_depth(X, Ow1, Ow2, scale_last):
    with np.errstate(all="ignore"):
        a, b, na, nb = dists(dict(Ow=Ow1), dict(Ow=Ow2), X)
        normal = np.array([F(F(F(F(0) + F(a[k] / na)) + F(b[k] / nb)) / F(2)) for k in range(3)], F)
        mx = F(na * F(1)); mn = F(mx / F(scale_last))
        return normal, np.array([F(F(0.8) * mn), F(F(1.2) * mx), mx], F)


def pair_rule(P, o1, o2, form="rule"):
    """one matched pair -> dict(status, kind, x3D, x3Dh, and what the decisions compared: cosRays, cos1, cos2, st1, st2, A (when step 4 ran))"""
    with np.errstate(all="ignore"):
        st1, st2 = bool(o1["ur"] >= 0), bool(o2["ur"] >= 0)
        xn1, xn2, A = matrix_A(P, o1, o2)
        T1, T2 = o1["T"], o2["T"]
        r1 = [F(F(F(T1[k] * xn1[0]) + F(T1[4 + k] * xn1[1])) + F(T1[8 + k] * F(1))) for k in range(3)]
        r2 = [F(F(F(T2[k] * xn2[0]) + F(T2[4 + k] * xn2[1])) + F(T2[8 + k] * F(1))) for k in range(3)]
        n1, n2 = F(np.sqrt(dot3(*r1, *r1))), F(np.sqrt(dot3(*r2, *r2)))
        cosRays = F(dot3(*r1, *r2) / F(n1 * n2))
        cosf = cos_identity if form == "rule" else cos_libm
        cos1 = cos2 = F(cosRays + F(1))
        if st1:
            cos1 = cosf(P["mb"], o1["depth"])
        elif st2:
            cos2 = cosf(P["mb"], o2["depth"])
        cosStereo = cos2 if cos2 < cos1 else cos1
        o = dict(status=NO_MATCH, kind=0, x3D=np.zeros(3, F), x3Dh=np.zeros(4, D), cosRays=cosRays, cos1=cos1, cos2=cos2, st1=st1, st2=st2, A=None, sweeps=0)
        if cosRays < cosStereo and cosRays > 0 and (st1 or st2 or D(cosRays) < (0.9996 if P["inertial"] else 0.9998)):
            o["A"] = A
            if form == "rule":
                o["x3Dh"], o["sweeps"] = jacobi_null_vector(A)
            else:
                o["x3Dh"] = lapack_null_vector(A, F).astype(D)
            h = o["x3Dh"].astype(F)
            if h[3] == 0:
                o["status"] = DEGENERATE
                return o
            X = np.array([F(h[0] / h[3]), F(h[1] / h[3]), F(h[2] / h[3])], F)
        elif st1 and cos1 < cos2:
            o["kind"] = 1
            X = unproject_stereo(P, o1)
        elif st2 and cos2 < cos1:
            o["kind"] = 2
            X = unproject_stereo(P, o2)
        else:
            o["status"] = LOW_PARALLAX
            return o
        if X is None:
            o["status"] = STEREO_NO_DEPTH
            return o
        o["x3D"] = X
        o["status"] = gates(P, o1, o2, st1, st2, X)
        return o


def numpy_dist(desc1, desc2):
    """a stand-in table of DescriptorDistance for scenes that never reach the library's search: (int)(512 |a - b|^2), both forms read the same table"""
    d = np.asarray(desc1, D)[:, None, :] - np.asarray(desc2, D)[None, :, :]
    return (512.0 * (d * d).sum(-1)).astype(np.int32)


def header_of(status, kind, winner_b):
    """the eight ints of one problem from the snapshot statuses; winner_b: (is new, is superseded) per keypoint"""
    new, sup = winner_b
    m = status != NO_MATCH
    return np.array([m.sum(), (m & (status != LOW_PARALLAX) & (kind == 0)).sum(), (kind != 0).sum(), (status == ACCEPTED).sum(), new.sum(), (new & (kind != 0)).sum(),
                     sup.sum(), 0], np.int32)


def rule_from_matches(P, k1, k2s, match12, claim=True, side1=None):
    """the contract from match12 [B][n1] on: per-pair rule, claim, headers, compact list.  side1: B keyframes (own side-1 blocks, no claim)"""
    B, n1 = len(k2s), len(k1["xy"])
    st = np.zeros((B, n1), np.uint8); kd = np.zeros((B, n1), np.uint8); xyz = np.zeros((B, n1, 3), F)
    info = {}
    for b in range(B):
        ka = k1 if side1 is None else side1[b]
        n2 = len(k2s[b]["xy"])
        for i in range(n1):
            m = int(match12[b][i])
            if m < 0 or m >= n2:
                continue
            r = pair_rule(P, obs(ka, i), obs(k2s[b], m))
            st[b, i], kd[b, i], xyz[b, i] = r["status"], r["kind"], r["x3D"]
            info[(b, i)] = r
    out = dict(kind=kd, xyz=xyz, info=info, snapshot=st.copy())
    acc = st == ACCEPTED
    if claim:
        winner = np.where(acc.any(0), acc.argmax(0), -1).astype(np.int32)
    hdr = np.zeros((B, 8), np.int32)
    lst = []
    for b in range(B):
        new = (winner == b) if claim else acc[b]
        sup = ((st[b] != NO_MATCH) & (winner >= 0) & (winner < b)) if claim else np.zeros(n1, bool)
        hdr[b] = header_of(st[b], kd[b], (new, sup))
        if claim:
            lst += [(i, b) for i in np.nonzero(new)[0]]
    out["header"] = hdr
    if claim:
        for b in range(B):
            st[b][(st[b] != NO_MATCH) & (winner >= 0) & (winner < b)] = SUPERSEDED
        n_new = len(lst)
        o = dict(winner=winner, n_new=n_new, new_idx1=np.full(n1, -1, np.int32), new_b=np.full(n1, -1, np.int32), new_idx2=np.full(n1, -1, np.int32),
                 new_xyz=np.zeros((n1, 3), F), new_normal=np.zeros((n1, 3), F), new_dist=np.zeros((n1, 3), F))
        for j, (i, b) in enumerate(lst):
            o["new_idx1"][j], o["new_b"][j], o["new_idx2"][j], o["new_xyz"][j] = i, b, match12[b][i], xyz[b, i]
            o["new_normal"][j], o["new_dist"][j] = normal_depth(xyz[b, i], np.asarray(k1["Ow"], F), np.asarray(k2s[b]["Ow"], F), P["scale_last"])
        out.update(o)
    out["status"] = st
    return out


def snapshot_matches(dist, k1, k2s, F12, ep, **kw):
    """match12 [B][n1] of ONE batched search: every neighbour against the same has1"""
    return np.stack([RT.order_free(dist[b], k1, k2s[b], F12[b], ep[b], **kw)["match12"] for b in range(len(k2s))])


def rule(P, dist, k1, k2s, F12, ep, **kw):
    return rule_from_matches(P, k1, k2s, snapshot_matches(dist, k1, k2s, F12, ep, **kw))


def literal(P, dist, k1, k2s, F12, ep, **kw):
    """:434-710: per neighbour the search on the CURRENT has1, then the loop over vMatchedIndices; a created point sets has1[idx1]
    -> dict(status [B][n1] (NO_MATCH where the pair was never searched), kind, xyz, created: list of (idx1, b, idx2, x3D, normal, dist))"""
    B, n1 = len(k2s), len(k1["xy"])
    k1 = dict(k1, has=np.array(k1["has"], np.uint8).copy())
    st = np.zeros((B, n1), np.uint8); kd = np.zeros((B, n1), np.uint8); xyz = np.zeros((B, n1, 3), F)
    created = []
    for b in range(B):
        pairs = RT.literal(dist[b], k1, k2s[b], F12[b], ep[b], **kw)["pairs"]
        for idx1, idx2 in pairs:
            r = pair_rule(P, obs(k1, idx1), obs(k2s[b], idx2), form="literal")
            st[b, idx1], kd[b, idx1], xyz[b, idx1] = r["status"], r["kind"], r["x3D"]
            if r["status"] != ACCEPTED:
                continue                                                   # every `continue` of :586-691
            nrm, dst = normal_depth(r["x3D"], np.asarray(k1["Ow"], F), np.asarray(k2s[b]["Ow"], F), P["scale_last"])
            created.append((idx1, b, idx2, r["x3D"], nrm, dst))
            k1["has"][idx1] = 1                                           # mpCurrentKeyFrame->AddMapPoint(pMP, idx1)
    return dict(status=st, kind=kd, xyz=xyz, created=created)


def ulps(a, b):
    """distance in float32 steps between two arrays (equal NaNs and equal infinities are 0)"""
    a, b = np.asarray(a, F).ravel(), np.asarray(b, F).ravel()
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia); ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.where(np.isnan(a) & np.isnan(b), 0, np.abs(ia - ib))
