"""Optimizer::PoseOptimization (reference src/Optimizer.cc:814-1114, conventional camera, Pinhole) restated in float64, twice:

  literal(...)  a transcription with the objects the reference has: edges with a level, a robust kernel and a stored _error, an optimizer with
                computeActiveErrors / activeRobustChi2 / buildSystem over the level-0 edges in insertion order, a vertex with push / pop, the
                Levenberg solve() line by line, and the classification loop that reads a stale _error for inliers.
  rule(...)     what k_pose_optimize does: the state machine of xfeatslam_amd/csrc/poseopt_math.h driven by passes over all keypoints, with H, b and
                the chi2 sums folded in the kernel's order (lane l of 256 adds keypoints l, l + 256, ...; xor butterfly 32 .. 1 over 64 lanes;
                four waves in order).

  rule(..., libm_jitter=seed)  the rule with every sqrt / sin / cos result moved by up to one double ulp: the device's libm is not the host's.

Both use the same per-edge arithmetic (the lines of poseopt_math.h, operation by operation), so they differ in summation order and in
bookkeeping only.  Every decision also records how far it was from its decision point (`margins`), which is what the rig's condition is.
same_decisions() compares two results with their trajectories, outputs_agree() their outputs alone."""
import collections
import math

import numpy as np

D, F = np.float64, np.float32
CHI2_MONO, CHI2_STEREO = F(5.991), F(7.815)
DELTA_MONO, DELTA_STEREO = float(F(math.sqrt(5.991))), float(F(math.sqrt(7.815)))
DBL_MAX = float(np.finfo(D).max)
THREADS = 256
H_KEYS = ("n_initial", "n_bad", "ret", "rounds", "iterations", "trials", "rejected", "ldlt_failures")


def _cut(thr):
    """the double at which (float)chi2 > thr changes: half way between thr and the next float"""
    return (float(thr) + float(np.nextafter(thr, F(np.inf)))) / 2.0


CUT_MONO, CUT_STEREO = _cut(CHI2_MONO), _cut(CHI2_STEREO)

_JITTER = None                                                          # a RandomState while rule(..., libm_jitter=seed) runs


def _libm(v):
    """a sqrt / sin / cos result (a float or an array): as the host's libm gave it, or -- under rule(..., libm_jitter=seed) -- moved by -1, 0 or +1
    double ulp, which is how another libm may answer"""
    if _JITTER is None:
        return v
    k = _JITTER.randint(-1, 2, np.shape(v))
    with np.errstate(all="ignore"):
        r = np.where(k < 0, np.nextafter(v, -np.inf), np.where(k > 0, np.nextafter(v, np.inf), v))
    return r if np.ndim(v) else float(r)


# ---- the pose: SE3Quat as [qx, qy, qz, qw, tx, ty, tz] of Python floats ----------------------------------------------------------------------
def normalize(q):
    if q[3] < 0.0:
        q = [-q[0], -q[1], -q[2], -q[3]]
    n = _libm(math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]))
    return [q[0] / n, q[1] / n, q[2] / n, q[3] / n]


def quat_from_matrix(R):
    t = (R[0] + R[4]) + R[8]
    q = [0.0] * 4
    if t > 0.0:
        t = _libm(math.sqrt(t + 1.0))
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (R[7] - R[5]) * t, (R[2] - R[6]) * t, (R[3] - R[1]) * t
    else:
        i = 0
        if R[4] > R[0]:
            i = 1
        if R[8] > R[4 * i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = _libm(math.sqrt(((R[4 * i] - R[4 * j]) - R[4 * k]) + 1.0))
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[3 * k + j] - R[3 * j + k]) * t
        q[j] = (R[3 * j + i] + R[3 * i + j]) * t
        q[k] = (R[3 * k + i] + R[3 * i + k]) * t
    return q


def matrix_from_quat(q):
    tx, ty, tz = 2.0 * q[0], 2.0 * q[1], 2.0 * q[2]
    twx, twy, twz = tx * q[3], ty * q[3], tz * q[3]
    txx, txy, txz, tyy, tyz, tzz = tx * q[0], ty * q[0], tz * q[0], ty * q[1], tz * q[1], tz * q[2]
    return [1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1.0 - (txx + tyy)]


def from_tcw(T):
    T = [float(v) for v in np.asarray(T, F).reshape(12)]
    q = normalize(quat_from_matrix([T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]]))
    return q + [T[3], T[7], T[11]]


def to_tcw(p):
    R = matrix_from_quat(p[:4])
    return np.array([R[0], R[1], R[2], p[4], R[3], R[4], R[5], p[5], R[6], R[7], R[8], p[6]], D).astype(F)


def rotate(q, v):
    """q * v; v may be three arrays"""
    ux, uy, uz = 2.0 * (q[1] * v[2] - q[2] * v[1]), 2.0 * (q[2] * v[0] - q[0] * v[2]), 2.0 * (q[0] * v[1] - q[1] * v[0])
    return [(v[0] + q[3] * ux) + (q[1] * uz - q[2] * uy), (v[1] + q[3] * uy) + (q[2] * ux - q[0] * uz), (v[2] + q[3] * uz) + (q[0] * uy - q[1] * ux)]


def oplus(u, p):
    """SE3Quat::exp(u) * p"""
    u = [float(v) for v in u]
    wx, wy, wz = u[0], u[1], u[2]
    theta = _libm(math.sqrt((wx * wx + wy * wy) + wz * wz))
    O = [0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0]
    O2 = [(O[3 * r] * O[c] + O[3 * r + 1] * O[3 + c]) + O[3 * r + 2] * O[6 + c] for r in range(3) for c in range(3)]
    I = [1.0 if k % 4 == 0 else 0.0 for k in range(9)]
    if theta < 0.00001:
        R = [(I[k] + O[k]) + O2[k] for k in range(9)]
        V = list(R)
    else:
        s, c, t2 = _libm(math.sin(theta)), _libm(math.cos(theta)), theta * theta
        a, b, d = s / theta, (1.0 - c) / t2, (theta - s) / (t2 * theta)
        R = [(I[k] + a * O[k]) + b * O2[k] for k in range(9)]
        V = [(I[k] + b * O[k]) + d * O2[k] for k in range(9)]
    eq = quat_from_matrix(R)
    et = [(V[3 * r] * u[3] + V[3 * r + 1] * u[4]) + V[3 * r + 2] * u[5] for r in range(3)]
    eq = normalize(eq)
    rt = rotate(eq, p[4:7])
    a, b = eq, p[:4]
    q = [((a[3] * b[0] + a[0] * b[3]) + a[1] * b[2]) - a[2] * b[1],
         ((a[3] * b[1] + a[1] * b[3]) + a[2] * b[0]) - a[0] * b[2],
         ((a[3] * b[2] + a[2] * b[3]) + a[0] * b[1]) - a[1] * b[0],
         ((a[3] * b[3] - a[0] * b[0]) - a[1] * b[1]) - a[2] * b[2]]
    return normalize(q) + [et[0] + rt[0], et[1] + rt[1], et[2] + rt[2]]


# ---- the edges, vectorised over any number of them (scalars work too) ---------------------------------------------------------------------------
def cam_of(cam):
    """(fx, fy, cx, cy, bf) as the doubles of the floats the library is given"""
    return tuple(float(F(v)) for v in cam)


def edge_error(p, cam, X, obs, stereo, w):
    """-> pc [3], e [3], chi2: computeError + chi2() at pose p.  X, obs: (n, 3) float64; stereo: (n,) bool"""
    fx, fy, cx, cy, bf = cam
    with np.errstate(all="ignore"):
        r = rotate(p[:4], [X[..., 0], X[..., 1], X[..., 2]])
        pc = [r[0] + p[4], r[1] + p[5], r[2] + p[6]]
        m0 = obs[..., 0] - (fx * pc[0] / pc[2] + cx)
        m1 = obs[..., 1] - (fy * pc[1] / pc[2] + cy)
        invz = np.asarray(1.0 / pc[2]).astype(F).astype(D)
        u = pc[0] * invz * fx + cx
        s0 = obs[..., 0] - u
        s1 = obs[..., 1] - (pc[1] * invz * fy + cy)
        s2 = obs[..., 2] - (u - bf * invz)
        e = [np.where(stereo, s0, m0), np.where(stereo, s1, m1), np.where(stereo, s2, 0.0)]
        c2 = e[0] * (w * e[0]) + e[1] * (w * e[1])
        chi2 = np.where(stereo, c2 + e[2] * (w * e[2]), c2)
    return pc, e, chi2


def edge_jacobian(cam, pc, stereo):
    """-> 18 arrays, the 3x6 Jacobian row-major (third row zero for mono)"""
    fx, fy, cx, cy, bf = cam
    x, y, z = pc
    with np.errstate(all="ignore"):
        a, c, b, d = fx / z, -fx * x / (z * z), fy / z, -fy * y / (z * z)
        zero = np.zeros_like(np.asarray(x, D))
        M = [-(c * y), -(a * z - c * x), -(-a * y), -a, zero, -c, -(d * y - b * z), -(-d * x), -(b * x), zero, -b, -d] + [zero] * 6
        invz = 1.0 / z
        i2 = invz * invz
        S = [x * y * i2 * fx, -(1.0 + (x * x * i2)) * fx, y * invz * fx, -invz * fx, zero, x * i2 * fx,
             (1.0 + y * y * i2) * fy, -x * y * i2 * fy, -x * invz * fy, zero, -invz * fy, y * i2 * fy]
        S += [S[0] - bf * y * i2, S[1] + bf * x * i2, S[2], S[3], zero, S[5] - bf * i2]
        return [np.where(stereo, S[k], M[k]) for k in range(18)]


def huber(chi2, stereo):
    delta = np.where(stereo, DELTA_STEREO, DELTA_MONO)
    dsqr = delta * delta
    with np.errstate(all="ignore"):
        sq = _libm(np.sqrt(chi2))
        inl = chi2 <= dsqr
        return np.where(inl, chi2, 2.0 * sq * delta - dsqr), np.where(inl, 1.0, delta / sq)


def shares(J, e, stereo, w, rho1):
    """one edge's share of the 28 sums (the chi2 entry left 0): (n, 28)"""
    ww = rho1 * w
    out = []
    with np.errstate(all="ignore"):
        for i in range(6):
            for j in range(i, 6):
                c = J[i] * (ww * J[j]) + J[6 + i] * (ww * J[6 + j])
                out.append(np.where(stereo, c + J[12 + i] * (ww * J[12 + j]), c))
        for i in range(6):
            c = J[i] * (w * e[0]) + J[6 + i] * (w * e[1])
            c = np.where(stereo, c + J[12 + i] * (w * e[2]), c)
            out.append(-(rho1 * c))
        out.append(np.zeros_like(out[0]))
    return np.stack([np.asarray(o, D) for o in out], -1)


def ldlt_solve(H21, lam, b, x):
    """-> ok, x (the old x when not ok), pivots seen"""
    A = [[0.0] * 6 for _ in range(6)]
    n = 0
    for i in range(6):
        for j in range(i, 6):
            A[i][j] = A[j][i] = float(H21[n])
            n += 1
    for i in range(6):
        A[i][i] = A[i][i] + lam
    d, piv = [0.0] * 6, []
    for j in range(6):
        dj = A[j][j]
        for k in range(j):
            dj = dj - A[j][k] * A[j][k] * d[k]
        piv.append((dj, abs(A[j][j])))
        if not dj > 0.0:
            return False, list(x), piv
        d[j] = dj
        for i in range(j + 1, 6):
            s = A[i][j]
            for k in range(j):
                s = s - A[i][k] * A[j][k] * d[k]
            A[i][j] = s / dj
    y = [0.0] * 6
    for i in range(6):
        s = float(b[i])
        for k in range(i):
            s = s - A[i][k] * y[k]
        y[i] = s
    y = [y[i] / d[i] for i in range(6)]
    xo = [0.0] * 6
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s = s - A[k][i] * xo[k]
        xo[i] = s
    return True, xo, piv


def edges_of(xy_un, uright, assigned, points):
    """-> idx (keypoints with an edge), X (n, 3), obs (n, 3), stereo (n,)"""
    assigned = np.asarray(assigned, np.int32)
    nq = len(points)
    idx = np.nonzero((assigned >= 0) & (assigned < nq))[0]
    X = np.asarray(points, F)[assigned[idx]].astype(D).reshape(-1, 3)
    ur = np.full(len(assigned), -1.0, F) if uright is None else np.asarray(uright, F)
    obs = np.concatenate([np.asarray(xy_un, F)[idx].reshape(-1, 2), ur[idx, None]], 1).astype(D)
    return idx, X, obs, ~(ur[idx] < 0)


class Trace:
    def __init__(self):
        self.events, self.reasons, self.history, self.margins = [], [], [], dict(classify=np.inf, rho=np.inf, stop=np.inf, pivot=np.inf)

    def margin(self, key, v):
        if v == v:
            self.margins[key] = min(self.margins[key], float(v))


def _levenberg_step(S, tempChi, tr):
    """lines 129-166 of optimization_algorithm_levenberg.cpp on a dict-like state; -> 'trial' | 'stop:<reason>' | 'ok', accepted"""
    rho = S["currentChi"] - tempChi
    scale = 0.0
    for j in range(6):
        scale += S["x"][j] * (S["lam"] * S["x"][j] + S["b"][j])
    scale += 1e-3
    with np.errstate(all="ignore"):
        rho = float(D(rho) / D(scale))
    tr.margin("rho", abs(rho))
    accepted = rho > 0.0 and math.isfinite(tempChi)
    if accepted:
        t = 2.0 * rho - 1.0
        alpha = 1.0 - t * t * t
        alpha = 2.0 / 3.0 if 2.0 / 3.0 < alpha else alpha
        f = alpha if 1.0 / 3.0 < alpha else 1.0 / 3.0
        S["lam"] *= f
        S["ni"] = 2.0
        S["currentChi"] = tempChi
    else:
        S["lam"] *= S["ni"]
        S["ni"] *= 2.0
    S["qmax"] += 1
    if rho < 0.0 and S["qmax"] < 10:
        return "trial", accepted
    if S["qmax"] == 10 or rho == 0.0:
        return "stop:qmax" if S["qmax"] == 10 else "stop:rho0", accepted
    ini, cur = S["iniChi"], S["currentChi"]
    if ini == ini and cur == cur and ini != 0.0:
        tr.margin("stop", abs((ini - cur) * 1e3 - ini) / abs(ini))
    if (ini - cur) * 1e3 < ini:
        S["nbad"] += 1
    else:
        S["nbad"] = 0
    if S["nbad"] >= 3:
        return "stop:three", accepted
    return "ok", accepted


def _lambda_init(H21):
    m, n = 0.0, 0
    for j in range(6):
        a = abs(float(H21[n]))
        m = m if a < m else a
        n += 6 - j
    return 1e-5 * m


def _classify(chi2, stereo, tr):
    cf = F(chi2)
    cut = CUT_STEREO if stereo else CUT_MONO
    tr.margin("classify", abs(float(chi2) - cut) / cut)
    return bool(cf > (CHI2_STEREO if stereo else CHI2_MONO)), cf


def _result(nt, Tcw_out, outlier, chi2, hdr, final, tr):
    return dict(Tcw_out=np.asarray(Tcw_out, F).reshape(12), outlier=outlier, chi2=chi2, header=np.array(hdr, np.int32), final_chi2=float(final),
                events=tr.events, reasons=tr.reasons, history=tr.history, margins=tr.margins)


# ---- the literal form ------------------------------------------------------------------------------------------------------------------------
class _Edge:
    """one g2o edge: its keypoint, kind, level, whether it still has its robust kernel, and _error / the camera-frame point as last computed"""

    def __init__(self, i, k, stereo):
        self.i, self.k, self.stereo, self.level, self.robust, self.error, self.pc = i, k, bool(stereo), 0, True, None, None


def literal(Tcw, cam, xy_un, uright, assigned, points, inv_sigma2, stale=True):
    """stale=False: every edge computes its error afresh before it is classified -- NOT the reference; it shows where the stale rule matters"""
    cam, w = cam_of(cam), float(F(inv_sigma2))
    nt = len(assigned)
    tr = Trace()
    outlier, chi2_out = np.zeros(nt, np.uint8), np.zeros(nt, F)
    idx, X, obs, st = edges_of(xy_un, uright, assigned, points)
    edges = [_Edge(i, int(k), st[i]) for i, k in enumerate(idx)]
    hdr = [len(edges), 0, 0, 0, 0, 0, 0, 0]
    if len(edges) < 3:
        return _result(nt, Tcw, outlier, chi2_out, hdr, 0.0, tr)
    estimate = None
    S = dict(x=[0.0] * 6, currentChi=0.0)

    def compute_errors(es):                                               # computeError() of each edge in the list (evaluated together, stored per edge)
        ii = [e.i for e in es]
        pc, er, _ = edge_error(estimate, cam, X[ii], obs[ii], st[ii], w)
        for n, e in enumerate(es):
            e.error = (float(er[0][n]), float(er[1][n]), float(er[2][n]))
            e.pc = (float(pc[0][n]), float(pc[1][n]), float(pc[2][n]))

    def chi2(e):
        c = e.error[0] * (w * e.error[0]) + e.error[1] * (w * e.error[1])
        return c + e.error[2] * (w * e.error[2]) if e.stereo else c

    def rho_of(es):                                                       # robustify(chi2) where the edge has a kernel, else (chi2, 1)
        c = np.array([chi2(e) for e in es], D)
        r0, r1 = huber(c, np.array([e.stereo for e in es]))
        has = np.array([e.robust for e in es])
        return np.where(has, r0, c), np.where(has, r1, 1.0)

    def robust_chi2(es):
        s = 0.0
        for v in rho_of(es)[0].tolist():
            s += v
        return s

    nbad = 0
    for it in range(4):
        estimate = from_tcw(Tcw)                                          # pFrame->GetPose(): the input, every round
        active = [e for e in edges if e.level == 0]                       # initializeOptimization(0)
        reason = "noactive"
        for i in range(10 if active else 0):                              # optimize(10)
            compute_errors(active)
            S["currentChi"] = robust_chi2(active)
            S["iniChi"] = S["currentChi"]
            acc = np.zeros(28, D)                                         # buildSystem: the edges in insertion order
            pcs, ers = np.array([e.pc for e in active], D), np.array([e.error for e in active], D)
            sta = np.array([e.stereo for e in active])
            sh = shares(edge_jacobian(cam, [pcs[:, 0], pcs[:, 1], pcs[:, 2]], sta), [ers[:, 0], ers[:, 1], ers[:, 2]], sta, w, rho_of(active)[1])
            for row in sh:
                acc = acc + row
            S["H"], S["b"] = acc[:21].copy(), acc[21:27].copy()
            if i == 0:
                S["lam"], S["ni"], S["nbad"] = _lambda_init(S["H"]), 2.0, 0
            S["qmax"] = 0
            hdr[4] += 1
            tr.events.append(("build", it, i))
            while True:
                backup = list(estimate)                                   # push()
                ok, S["x"], piv = ldlt_solve(S["H"], S["lam"], S["b"], S["x"])
                for dj, ajj in piv:
                    if ajj > 0:
                        tr.margin("pivot", abs(dj) / ajj)
                estimate = oplus(S["x"], estimate)
                hdr[5] += 1
                hdr[7] += 0 if ok else 1
                compute_errors(active)
                tempChi = robust_chi2(active) if ok else DBL_MAX
                step, accepted = _levenberg_step(S, tempChi, tr)
                if not accepted:
                    estimate = backup                                     # pop(): the edges keep the errors of the rejected estimate
                    hdr[6] += 1
                tr.events.append(("trial", it, i, S["qmax"], accepted, ok))
                if step != "trial":
                    break
            if step.startswith("stop"):
                reason = step[5:]
                break
            reason = "iterations"
        tr.reasons.append(reason)
        nbad = 0
        for e in edges:                                                   # (the mono and the stereo loop differ in the threshold only)
            if outlier[e.k] or not stale:
                compute_errors([e])
            o, cf = _classify(chi2(e), e.stereo, tr)
            outlier[e.k], chi2_out[e.k], e.level = o, cf, 1 if o else 0
            nbad += o
            if it == 2:
                e.robust = False
        tr.history.append(outlier.copy())
        hdr[1], hdr[2] = nbad, len(edges) - nbad
        hdr[3] += 1
        if len(edges) < 10:
            break
    return _result(nt, to_tcw(estimate), outlier, chi2_out, hdr, S["currentChi"], tr)


# ---- the kernel's rule -------------------------------------------------------------------------------------------------------------------------
def fold(per_keypoint):
    """(nt, m) shares per keypoint slot (zero rows where nothing is added) -> (m,) in the kernel's order"""
    nt, m = per_keypoint.shape
    ept = -(-nt // THREADS)
    a = np.zeros((ept * THREADS, m), D)
    a[:nt] = per_keypoint
    a = a.reshape(ept, THREADS, m)
    acc = np.zeros((THREADS, m), D)
    with np.errstate(all="ignore"):
        for j in range(ept):
            acc = acc + a[j]
        v = acc.reshape(THREADS // 64, 64, m)
        lane = np.arange(64)
        for s in (32, 16, 8, 4, 2, 1):
            v = v + v[:, lane ^ s]
        return ((v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0]


def rule(Tcw, cam, xy_un, uright, assigned, points, inv_sigma2, libm_jitter=None):
    """libm_jitter=seed: every sqrt, sin and cos result is moved by -1, 0 or +1 double ulp from a stream seeded with it.  That is how the device may
    differ from this form: its fold is this one, only its libm is not the host's."""
    global _JITTER
    _JITTER = None if libm_jitter is None else np.random.RandomState(libm_jitter)
    try:
        return _rule(Tcw, cam, xy_un, uright, assigned, points, inv_sigma2)
    finally:
        _JITTER = None


def _rule(Tcw, cam, xy_un, uright, assigned, points, inv_sigma2):
    cam, w = cam_of(cam), float(F(inv_sigma2))
    nt = len(assigned)
    tr = Trace()
    outlier, chi2_out = np.zeros(nt, np.uint8), np.zeros(nt, F)
    idx, X, obs, st = edges_of(xy_un, uright, assigned, points)
    n = len(idx)
    hdr = [n, 0, 0, 0, 0, 0, 0, 0]
    if n < 3:
        return _result(nt, Tcw, outlier, chi2_out, hdr, 0.0, tr)
    out = np.zeros(n, bool)
    last = np.zeros(n, D)
    S = dict(x=[0.0] * 6, currentChi=0.0)
    inp = from_tcw(Tcw)
    est = inp

    def pass_(p, build, robust):
        nonlocal last
        act = ~out
        pc, e, c = edge_error(p, cam, X, obs, st, w)
        last = np.where(act, c, last)
        r0, r1 = huber(c, st) if robust else (c, np.ones(n, D))
        sh = shares(edge_jacobian(cam, pc, st), e, st, w, r1) if build else np.zeros((n, 28), D)
        sh[:, 27] = r0
        per = np.zeros((nt, 28), D)
        per[idx[act]] = sh[act]
        return fold(per)

    for rnd in range(4):
        est = inp
        robust = rnd < 3
        reason = "noactive"
        for i in range(10 if n - hdr[1] > 0 else 0):
            sums = pass_(est, True, robust)
            S["H"], S["b"], S["currentChi"] = sums[:21].copy(), sums[21:27].copy(), float(sums[27])
            S["iniChi"] = S["currentChi"]
            if i == 0:
                S["lam"], S["ni"], S["nbad"] = _lambda_init(S["H"]), 2.0, 0
            S["qmax"] = 0
            hdr[4] += 1
            tr.events.append(("build", rnd, i))
            while True:
                backup = est
                ok, S["x"], piv = ldlt_solve(S["H"], S["lam"], S["b"], S["x"])
                for dj, ajj in piv:
                    if ajj > 0:
                        tr.margin("pivot", abs(dj) / ajj)
                est = oplus(S["x"], est)
                hdr[5] += 1
                hdr[7] += 0 if ok else 1
                chi = float(pass_(est, False, robust)[27])
                step, accepted = _levenberg_step(S, chi if ok else DBL_MAX, tr)
                if not accepted:
                    est = backup
                    hdr[6] += 1
                tr.events.append(("trial", rnd, i, S["qmax"], accepted, ok))
                if step != "trial":
                    break
            if step.startswith("stop"):
                reason = step[5:]
                break
            reason = "iterations"
        tr.reasons.append(reason)
        _, _, fresh = edge_error(est, cam, X, obs, st, w)
        c = np.where(out, fresh, last)
        for i in range(n):
            out[i], chi2_out[idx[i]] = _classify(c[i], st[i], tr)
        outlier[idx] = out
        tr.history.append(outlier.copy())
        hdr[1], hdr[2] = int(out.sum()), n - int(out.sum())
        hdr[3] += 1
        if n < 10:
            break
    return _result(nt, to_tcw(est), outlier, chi2_out, hdr, S["currentChi"], tr)


def same_decisions(a, b):
    """names of what differs between two results in decisions: flags, the header, the accept / reject sequence, the reasons"""
    bad = [k for k in ("outlier", "header") if not np.array_equal(a[k], b[k])]
    return bad + [k for k in ("events", "reasons") if a[k] != b[k]]


Tol = collections.namedtuple("Tol", "pose chi2 final")                   # float32 steps, float32 steps, relative


def header_in_bounds(h):
    """header[4:8] within what the loop's limits allow, whatever the trajectory: iterations <= 40, iterations <= trials <= 400, rejected and
    ldlt_failures <= trials"""
    return bool(0 <= h[4] <= 40 and h[4] <= h[5] <= 400 and 0 <= h[6] <= h[5] and 0 <= h[7] <= h[5])


def outputs_agree(a, b, tol):
    """what differs between two results in their OUTPUTS, as a list of strings; nothing about the trajectory (events, reasons, header[4:8] beyond
    their static bounds): where a rho lies in rounding noise two correct evaluations take different numbers of trials to the same answer"""
    bad = []
    if not np.array_equal(a["outlier"], b["outlier"]):
        k = np.nonzero(np.asarray(a["outlier"]) != np.asarray(b["outlier"]))[0]
        bad.append(f"outlier differs at {len(k)} keypoints, first {k[:8].tolist()}")
    ha, hb = np.asarray(a["header"]), np.asarray(b["header"])
    if not np.array_equal(ha[:4], hb[:4]):
        bad.append(f"header[0:4] {ha[:4].tolist()} != {hb[:4].tolist()}")
    for tag, h in (("first", ha), ("second", hb)):
        if not header_in_bounds(h):
            bad.append(f"header[4:8] of the {tag} out of bounds: {h[4:].tolist()}")
    ut, uc = ulps(a["Tcw_out"], b["Tcw_out"]), ulps(a["chi2"], b["chi2"])
    if not ut.max() <= tol.pose:
        bad.append(f"Tcw_out {int(ut.max())} float steps apart at entry {int(ut.argmax())} (allowed {tol.pose})")
    if not uc.max() <= tol.chi2:
        bad.append(f"chi2 {int(uc.max())} float steps apart at keypoint {int(uc.argmax())} (allowed {tol.chi2})")
    rel = final_rel(a, b)
    if not rel <= tol.final:
        bad.append(f"final_chi2 {a['final_chi2']:.17g} and {b['final_chi2']:.17g}: {rel:.2e} relative (allowed {tol.final:.1e})")
    return bad


def final_rel(a, b):
    fa, fb = float(a["final_chi2"]), float(b["final_chi2"])
    return 0.0 if fa == fb else abs(fa - fb) / max(abs(fa), abs(fb))


def ulps(a, b):
    """distance in float32 steps, elementwise"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)
