"""Optimizer::OptimizeSim3 (reference src/Optimizer.cc:2100-2381, Pinhole cameras) restated in float64 as k_sim3_optimize computes it: the lines of
xfeatslam_amd/csrc/optsim3_math.h operation by operation -- the g2o::Sim3 state with its exponential, product and inverse, the two projection edges
with g2o's central-difference Jacobian, the Levenberg state machine of 7 unknowns over two rounds -- driven by passes over all keypoints, with H, b
and the robust chi2 folded in the kernel's order (lane l of 256 adds its keypoints l, l + 256, .. with e12 before e21; the xor butterfly 32 .. 1 over
64 lanes; four waves in order).  tests/ref_optsim3_literal.py is the transcription with the reference's objects.

  rule(p)                   p = a problem dict as tests/optsim3_rig.py makes it -> a result dict
  rule(p, libm_jitter=seed) every exp / sin / cos / sqrt result moved by up to one double step: the device's libm is not the host's.

A result also records what the rig's condition needs: the chi2 every classification read (cls1, cls2), the least |pivot| of every factorisation
and the accept / reject sequence.  outputs_agree() compares two results by the comparison rules of the GPU tests: decisions equal, numbers within a
tolerance, nothing about the trajectory beyond its static bounds."""
import collections
import math

import numpy as np

import ref_poseopt as RP

D, F = np.float64, np.float32
DELTA = 1e-9
SCALAR = 1.0 / (2 * DELTA)
DBL_MAX = RP.DBL_MAX
THREADS = 256
NO_EDGE, BAD_FIRST, BAD_FINAL, INLIER = range(4)
EDGE, IN_KF2 = 1, 2
H_KEYS = ("n_corr", "n_in_kf2", "n_out_kf2", "n_bad", "n_bad_out_kf2", "n_more", "ret", "rounds", "iterations", "trials", "rejected", "ldlt_failures")
_libm = RP._libm


# ---- g2o::Sim3 as [qx, qy, qz, qw, tx, ty, tz, s] of Python floats ---------------------------------------------------------------------------------
def state_from(S13):
    S = [float(v) for v in np.asarray(S13, F).reshape(13)]
    return RP.quat_from_matrix(S[:9]) + S[9:13]


def state_to(st):
    return np.array(RP.matrix_from_quat(st[:4]) + list(st[4:8]), D).astype(F)


def smap(S, X):
    """s * (r * X) + t; X may be three arrays"""
    r = RP.rotate(S[:4], X)
    return [S[7] * r[0] + S[4], S[7] * r[1] + S[5], S[7] * r[2] + S[6]]


def inverse(S):
    q = [-S[0], -S[1], -S[2], S[3]]
    m = -1.0 / S[7]
    return q + RP.rotate(q, [m * S[4], m * S[5], m * S[6]]) + [1.0 / S[7]]


def mul(A, B):
    a, b = A[:4], B[:4]
    rt = RP.rotate(a, B[4:7])
    q = [((a[3] * b[0] + a[0] * b[3]) + a[1] * b[2]) - a[2] * b[1],
         ((a[3] * b[1] + a[1] * b[3]) + a[2] * b[0]) - a[0] * b[2],
         ((a[3] * b[2] + a[2] * b[3]) + a[0] * b[1]) - a[1] * b[0],
         ((a[3] * b[3] - a[0] * b[0]) - a[1] * b[1]) - a[2] * b[2]]
    return q + [A[7] * rt[0] + A[4], A[7] * rt[1] + A[5], A[7] * rt[2] + A[6], A[7] * B[7]]


def exp7(u):
    """Sim3(Vector7d), sim3.h:70-142"""
    u = [float(v) for v in u]
    wx, wy, wz, sigma = u[0], u[1], u[2], u[6]
    theta = _libm(math.sqrt((wx * wx + wy * wy) + wz * wz))
    O = [0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0]
    O2 = [(O[3 * r] * O[c] + O[3 * r + 1] * O[3 + c]) + O[3 * r + 2] * O[6 + c] for r in range(3) for c in range(3)]
    I = [1.0 if k % 4 == 0 else 0.0 for k in range(9)]
    s, eps = _libm(math.exp(sigma)), 0.00001
    small = theta < eps
    if abs(sigma) < eps:
        C = 1.0
        if small:
            A, B = 1.0 / 2.0, 1.0 / 6.0
        else:
            theta2 = theta * theta
            A = (1.0 - _libm(math.cos(theta))) / theta2
            B = (theta - _libm(math.sin(theta))) / (theta2 * theta)
    else:
        C = (s - 1.0) / sigma
        if small:
            sigma2 = sigma * sigma
            A = ((sigma - 1.0) * s + 1.0) / sigma2
            B = ((0.5 * sigma2 - sigma + 1.0) * s) / (sigma2 * sigma)
        else:
            a, b, theta2, sigma2 = s * _libm(math.sin(theta)), s * _libm(math.cos(theta)), theta * theta, sigma * sigma
            c = theta2 + sigma2
            A = (a * sigma + (1.0 - b) * theta) / (theta * c)
            B = (C - ((b - 1.0) * sigma + a * theta) / c) * 1.0 / theta2
    if small:
        R = [(I[k] + O[k]) + O2[k] for k in range(9)]
    else:
        ra, rb = _libm(math.sin(theta)) / theta, (1.0 - _libm(math.cos(theta))) / (theta * theta)
        R = [(I[k] + ra * O[k]) + rb * O2[k] for k in range(9)]
    W = [(A * O[k] + B * O2[k]) + C * I[k] for k in range(9)]
    return RP.quat_from_matrix(R) + [(W[3 * r] * u[3] + W[3 * r + 1] * u[4]) + W[3 * r + 2] * u[5] for r in range(3)] + [s]


def oplus(u, est, fix_scale):
    u = [float(v) for v in u]
    if fix_scale:
        u[6] = 0.0
    return mul(exp7(u), est)


def perturbed(est, fix_scale):
    """-> pert[14], pinv[14]: exp(+delta e_d) * est at 2 d, exp(-delta e_d) * est at 2 d + 1, and their inverses"""
    pert = []
    for d in range(7):
        for v in (DELTA, -DELTA):
            u = [0.0] * 7
            u[d] = v
            pert.append(oplus(u, est, fix_scale))
    return pert, [inverse(p) for p in pert]


# ---- the edges, vectorised over any number of them (scalars work too) ---------------------------------------------------------------------------
def edge_error(T, cam, X, obs, w):
    """-> [e0, e1], chi2 of obs - project(T.map(X))"""
    with np.errstate(all="ignore"):
        p = smap(T, X)
        e0 = obs[0] - (cam[0] * p[0] / p[2] + cam[2])
        e1 = obs[1] - (cam[1] * p[1] / p[2] + cam[3])
        return [e0, e1], e0 * (w * e0) + e1 * (w * e1)


def edge_jacobian(pert, cam, X, obs):
    """the central difference of base_binary_edge.hpp:130-205 -> 14 entries, [2][7] row-major"""
    J = [None] * 14
    with np.errstate(all="ignore"):
        for d in range(7):
            ep, _ = edge_error(pert[2 * d], cam, X, obs, 1.0)
            em, _ = edge_error(pert[2 * d + 1], cam, X, obs, 1.0)
            J[d], J[7 + d] = SCALAR * (ep[0] - em[0]), SCALAR * (ep[1] - em[1])
    return J


def huber(chi2, delta):
    dsqr = delta * delta
    with np.errstate(all="ignore"):
        sq = _libm(np.sqrt(chi2))
        inl = chi2 <= dsqr
        return np.where(inl, chi2, 2.0 * sq * delta - dsqr), np.where(inl, 1.0, delta / sq)


def shares(J, e, w, rho1, rho0):
    """one edge's share of the 36 sums: (n, 36)"""
    ww = rho1 * w
    out = []
    with np.errstate(all="ignore"):
        for i in range(7):
            for j in range(i, 7):
                out.append(J[i] * (ww * J[j]) + J[7 + i] * (ww * J[7 + j]))
        for i in range(7):
            out.append(-(rho1 * (J[i] * (w * e[0]) + J[7 + i] * (w * e[1]))))
        out.append(rho0)
    return np.stack([np.broadcast_to(np.asarray(o, D), np.shape(rho0)) for o in out], -1)


def ldlt_solve(H, lam, b, x, N=7):
    """-> ok, x (the old x when not ok), the pivots seen"""
    A = [[0.0] * N for _ in range(N)]
    n = 0
    for i in range(N):
        for j in range(i, N):
            A[i][j] = A[j][i] = float(H[n])
            n += 1
    for i in range(N):
        A[i][i] = A[i][i] + lam
    d, piv = [0.0] * N, []
    for j in range(N):
        dj = A[j][j]
        for k in range(j):
            dj = dj - A[j][k] * A[j][k] * d[k]
        piv.append(dj)
        if not dj > 0.0:
            return False, list(x), piv
        d[j] = dj
        for i in range(j + 1, N):
            s = A[i][j]
            for k in range(j):
                s = s - A[i][k] * A[j][k] * d[k]
            A[i][j] = s / dj
    y = [0.0] * N
    for i in range(N):
        s = float(b[i])
        for k in range(i):
            s = s - A[i][k] * y[k]
        y[i] = s
    y = [y[i] / d[i] for i in range(N)]
    xo = [0.0] * N
    for i in range(N - 1, -1, -1):
        s = y[i]
        for k in range(i + 1, N):
            s = s - A[k][i] * xo[k]
        xo[i] = s
    return True, xo, piv


def fold(sh12, sh21):
    """(n1, m) shares of e12 and of e21 per keypoint (zero rows where nothing is added) -> (m,) in the kernel's order"""
    n1, m = sh12.shape
    ept = -(-n1 // THREADS)
    a = np.zeros((ept * THREADS, 2, m), D)
    a[:n1, 0], a[:n1, 1] = sh12, sh21
    a = a.reshape(ept, THREADS, 2, m)
    acc = np.zeros((THREADS, m), D)
    with np.errstate(all="ignore"):
        for j in range(ept):
            acc = acc + a[j, :, 0]
            acc = acc + a[j, :, 1]
        v = acc.reshape(THREADS // 64, 64, m)
        lane = np.arange(64)
        for s in (32, 16, 8, 4, 2, 1):
            v = v + v[:, lane ^ s]
        return ((v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0]


# ---- the pairs (:2167-2304) -------------------------------------------------------------------------------------------------------------------------
def pairs_of(p):
    """-> st (n1,) state words, P1, P2 (n1, 3) float32 camera-frame points, o1, o2 (n1, 2) float32 observations (rows without an edge hold zeros)"""
    n1, M1, nq, n2 = len(p["assigned"]), len(p["points1"]), len(p["points2"]), len(p["xy_un2"])
    asg, pt1, idx2 = np.asarray(p["assigned"], np.int64), np.asarray(p["point1"], np.int64), np.asarray(p["index2"], np.int64)
    ok = (asg >= 0) & (asg < nq)
    q = np.where(ok, asg, 0)
    ok &= (np.asarray(p["flags2"], np.uint8)[q] & 1) != 0
    ok &= (pt1 >= 0) & (pt1 < M1)
    m = np.where(ok, pt1, 0)
    i2 = idx2[q]
    in2 = (i2 >= 0) & (i2 < n2)
    ok &= in2 | bool(p["all_points"])
    T1, T2 = np.asarray(p["T1w"], F).reshape(3, 4), np.asarray(p["T2w"], F).reshape(3, 4)
    X1, X2 = np.asarray(p["points1"], F)[m], np.asarray(p["points2"], F)[q]
    with np.errstate(all="ignore"):
        P1 = np.stack([((T1[r, 0] * X1[:, 0] + T1[r, 1] * X1[:, 1]) + T1[r, 2] * X1[:, 2]) + T1[r, 3] for r in range(3)], 1).astype(F)
        P2 = np.stack([((T2[r, 0] * X2[:, 0] + T2[r, 1] * X2[:, 1]) + T2[r, 2] * X2[:, 2]) + T2[r, 3] for r in range(3)], 1).astype(F)
        ok &= ~(P2[:, 2] < 0)
        invz = F(1) / P2[:, 2]
        norm = np.stack([P2[:, 0] * invz, P2[:, 1] * invz], 1).astype(F)
    o1 = np.asarray(p["xy_un1"], F).reshape(n1, 2)
    o2 = np.where(in2[:, None], np.asarray(p["xy_un2"], F).reshape(n2, 2)[np.where(in2, i2, 0)], norm).astype(F)
    st = np.where(ok, EDGE | np.where(in2, IN_KF2, 0), 0).astype(np.int32)
    z = ~ok
    P1, P2, o1, o2 = P1.copy(), P2.copy(), o1.copy(), o2.copy()
    P1[z], P2[z], o1[z], o2[z] = 0, 0, 0, 0
    return st, P1, P2, o1, o2


def compose(est, Tmw):
    """gScw = gS12 * Sim3(Rmw, tmw, 1) -> Tcw [R | t / s], Ow = -R^T (t / s), rounded once"""
    T = [float(v) for v in np.asarray(Tmw, F).reshape(12)]
    m = RP.quat_from_matrix([T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]]) + [T[3], T[7], T[11], 1.0]
    c = mul(est, m)
    R = RP.matrix_from_quat(c[:4])
    ts = [c[4] / c[7], c[5] / c[7], c[6] / c[7]]
    Tcw = np.array([R[0], R[1], R[2], ts[0], R[3], R[4], R[5], ts[1], R[6], R[7], R[8], ts[2]], D).astype(F)
    Ow = np.array([-((R[r] * ts[0] + R[3 + r] * ts[1]) + R[6 + r] * ts[2]) for r in range(3)], D).astype(F)
    return Tcw, Ow


def lambda_init(H):
    m, n = 0.0, 0
    for j in range(7):
        a = abs(float(H[n]))
        m = m if a < m else a
        n += 7 - j
    return 1e-5 * m


def levenberg_step(S, tempChi):
    """optimization_algorithm_levenberg.cpp:129-166 on a dict; -> 'trial' | 'stop' | 'ok', accepted, rho"""
    rho = S["currentChi"] - tempChi
    scale = 0.0
    for j in range(7):
        scale += S["x"][j] * (S["lam"] * S["x"][j] + S["b"][j])
    scale += 1e-3
    with np.errstate(all="ignore"):
        rho = float(D(rho) / D(scale))
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
        return "trial", accepted, rho
    if S["qmax"] == 10 or rho == 0.0:
        return "stop", accepted, rho
    if (S["iniChi"] - S["currentChi"]) * 1e3 < S["iniChi"]:
        S["nbad"] += 1
    else:
        S["nbad"] = 0
    return ("stop" if S["nbad"] >= 3 else "ok"), accepted, rho


def cam_of(cam):
    return [float(F(v)) for v in cam[:4]]


def result(p, est, st, bad1, bad2, last, hdr, final, cls1, cls2, events, min_pivot):
    edge = (st & EDGE) != 0
    asg = np.asarray(p["assigned"], np.int32)
    status = np.where(~edge, NO_EDGE, np.where(bad1, BAD_FIRST, np.where(bad2, BAD_FINAL, INLIER))).astype(np.uint8)
    with np.errstate(all="ignore"):
        chi2 = np.where(edge[:, None], last, 0.0).astype(F)
    r = dict(assigned_out=np.where(bad1 | bad2, -1, asg).astype(np.int32), status=status, chi2=chi2, state=np.array(est, D), S12_out=state_to(est),
             header=np.array(hdr + [0] * (16 - len(hdr)), np.int32), final_chi2=float(final), cls1=cls1, cls2=cls2, events=events, min_pivot=min_pivot)
    if p.get("Tmw") is not None:
        r["Tcw"], r["Ow"] = compose(est, p["Tmw"])
    return r


def rule(p, libm_jitter=None, stale=True):
    """stale=False: classification 1 computes fresh errors at the estimate instead of reading what the last computeActiveErrors left -- NOT the
    reference's behaviour, only a test's handle on the stale-error rule"""
    RP._JITTER = None if libm_jitter is None else np.random.RandomState(libm_jitter)
    try:
        return _rule(p, stale)
    finally:
        RP._JITTER = None


def _rule(p, stale):
    cam1, cam2 = cam_of(p["cam1"]), cam_of(p["cam2"])
    w1, w2, th2 = float(F(p["inv_sigma2_1"])), float(F(p["inv_sigma2_2"])), float(F(p["th2"]))
    delta, fix = float(F(math.sqrt(F(p["th2"])))), int(p["fix_scale"])
    st, P1, P2, o1, o2 = pairs_of(p)
    n1 = len(st)
    X1, X2 = [P1[:, k].astype(D) for k in range(3)], [P2[:, k].astype(D) for k in range(3)]
    b1, b2 = [o1[:, k].astype(D) for k in range(2)], [o2[:, k].astype(D) for k in range(2)]
    edge, in2 = (st & EDGE) != 0, (st & IN_KF2) != 0
    n_corr, n_out = int(edge.sum()), int((edge & ~in2).sum())
    hdr = [n_corr, n_corr - n_out, n_out, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    bad1, bad2 = np.zeros(n1, bool), np.zeros(n1, bool)
    last = np.zeros((n1, 2), D)
    cls1, cls2 = np.full((n1, 2), np.nan), np.full((n1, 2), np.nan)
    S = dict(x=[0.0] * 7, currentChi=0.0)
    inp = state_from(p["S12"])
    est, events, piv_min = inp, [], np.inf

    def pass_(T, build, robust):
        nonlocal last
        act = edge & ~bad1
        Ti = inverse(T)
        e12, c12 = edge_error(T, cam1, X2, b1, w1)
        e21, c21 = edge_error(Ti, cam2, X1, b2, w2)
        last = np.where(act[:, None], np.stack([c12, c21], 1), last)
        r12, r21 = (huber(c12, delta), huber(c21, delta)) if robust else ((c12, np.ones(n1, D)), (c21, np.ones(n1, D)))
        if build:
            pert, pinv = perturbed(T, fix)
            s12 = shares(edge_jacobian(pert, cam1, X2, b1), e12, w1, r12[1], r12[0])
            s21 = shares(edge_jacobian(pinv, cam2, X1, b2), e21, w2, r21[1], r21[0])
        else:
            s12, s21 = np.zeros((n1, 36), D), np.zeros((n1, 36), D)
            s12[:, 35], s21[:, 35] = r12[0], r21[0]
        s12[~act], s21[~act] = 0.0, 0.0
        return fold(s12, s21)

    for rnd in range(2):
        iters = 5 if rnd == 0 else hdr[5]
        robust = rnd == 0
        for i in range(iters if n_corr > 0 else 0):
            sums = pass_(est, True, robust)
            S["H"], S["b"], S["currentChi"] = sums[:28].copy(), sums[28:35].copy(), float(sums[35])
            S["iniChi"] = S["currentChi"]
            if i == 0:
                S["lam"], S["ni"], S["nbad"] = lambda_init(S["H"]), 2.0, 0
            S["qmax"] = 0
            hdr[8] += 1
            while True:
                backup = est
                ok, S["x"], piv = ldlt_solve(S["H"], S["lam"], S["b"], S["x"])
                piv_min = min([piv_min] + [abs(v) for v in piv if v == v])
                est = oplus(S["x"], est, fix)
                hdr[9] += 1
                hdr[11] += 0 if ok else 1
                chi = float(pass_(est, False, robust)[35])
                step, accepted, rho = levenberg_step(S, chi if ok else DBL_MAX)
                if not accepted:
                    est = backup
                    hdr[10] += 1
                events.append((rnd, i, S["qmax"], accepted, ok))
                if step != "trial":
                    break
            if step == "stop":
                break
        hdr[7] += 1
        act = edge & ~bad1
        if rnd == 0:
            if not stale:
                _, c12 = edge_error(est, cam1, X2, b1, w1)
                _, c21 = edge_error(inverse(est), cam2, X1, b2, w2)
                last = np.where(act[:, None], np.stack([c12, c21], 1), last)
            cls1[act] = last[act]
            with np.errstate(all="ignore"):
                bad1 = act & ((last[:, 0] > th2) | (last[:, 1] > th2))
            hdr[3], hdr[4] = int(bad1.sum()), int((bad1 & ~in2).sum())
            hdr[5] = 10 if hdr[3] > 0 else 5
            if n_corr - hdr[3] < 10:
                est = inp
                break
        else:
            _, c12 = edge_error(est, cam1, X2, b1, w1)
            _, c21 = edge_error(inverse(est), cam2, X1, b2, w2)
            last = np.where(act[:, None], np.stack([c12, c21], 1), last)
            cls2[act] = last[act]
            with np.errstate(all="ignore"):
                bad2 = act & ((last[:, 0] > th2) | (last[:, 1] > th2))
            hdr[6] = (n_corr - hdr[3]) - int(bad2.sum())
    return result(p, est, st, bad1, bad2, last, hdr, S["currentChi"], cls1, cls2, events, piv_min)


# ---- comparisons ---------------------------------------------------------------------------------------------------------------------------------
# state: relative to its largest entry; s12, tcw, ow: float32 steps at the magnitude of their block (block_steps); chi2: float32 steps at
# max(chi2, th2) (chi2_steps); final: relative to max(final_chi2, th2)
Tol = collections.namedtuple("Tol", "state s12 tcw ow chi2 final")
DECISIONS = ("status", "assigned_out")


def same_decisions(a, b):
    """names of what differs between two results in decisions: pair status, assigned_out, header[0:8]"""
    bad = [k for k in DECISIONS if not np.array_equal(a[k], b[k])]
    return bad + (["header[0:8]"] if not np.array_equal(np.asarray(a["header"])[:8], np.asarray(b["header"])[:8]) else [])


def header_in_bounds(h):
    """header[8:12] within what the loop's limits allow, whatever the trajectory: iterations <= 15, iterations <= trials <= 150, rejected and
    factorisation failures <= trials; header[12:16] zero"""
    return bool(0 <= h[8] <= 15 and h[8] <= h[9] <= 150 and 0 <= h[10] <= h[9] and 0 <= h[11] <= h[9] and not np.any(np.asarray(h[12:16])))


def state_rel(a, b):
    a, b = np.asarray(a, D), np.asarray(b, D)
    if not np.array_equal(np.isnan(a), np.isnan(b)):
        return np.inf
    a, b = np.nan_to_num(a), np.nan_to_num(b)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(a)), np.max(np.abs(b)), 1e-300))


def final_rel(a, b, th2=10.0):
    """relative to max(|a|, |b|, th2): a final chi2 far below th2 (one pair, which seven unknowns fit exactly) is cancellation noise"""
    fa, fb = float(a["final_chi2"]), float(b["final_chi2"])
    if fa != fa or fb != fb:
        return 0.0 if (fa != fa and fb != fb) else np.inf
    return 0.0 if fa == fb else abs(fa - fb) / max(abs(fa), abs(fb), th2)


S12_BLOCKS = (slice(0, 9), slice(9, 12), slice(12, 13))                     # R, t, s
TCW_BLOCKS = ([0, 1, 2, 4, 5, 6, 8, 9, 10], [3, 7, 11])                   # R, t / s


def block_steps(a, b, blocks, floor=0.0):
    """the largest |a - b| of each block in float32 steps AT THE BLOCK'S LARGEST MAGNITUDE (not below `floor`): an entry of a rotation matrix near
    zero, or a chi2 that is cancellation noise, has float steps of its own that say nothing about the matrix or about the test against th2"""
    a, b = np.asarray(a, D).reshape(-1), np.asarray(b, D).reshape(-1)
    worst = 0.0
    for blk in blocks:
        x, y = a[blk], b[blk]
        if not np.array_equal(np.isnan(x), np.isnan(y)):
            return np.inf
        x, y = np.nan_to_num(x, posinf=3e38, neginf=-3e38), np.nan_to_num(y, posinf=3e38, neginf=-3e38)
        if x.size == 0:
            continue
        mag = F(min(max(np.max(np.abs(x)), np.max(np.abs(y)), floor, 1e-30), 3e38))
        worst = max(worst, float(np.max(np.abs(x - y)) / float(np.spacing(mag))))
    return worst


def chi2_steps(a, b, th2):
    """per pair and direction: |a - b| in float32 steps at max(|a|, |b|, th2) -- below th2 the steps of th2, which is what the classification sees"""
    a, b = np.asarray(a, D).reshape(-1), np.asarray(b, D).reshape(-1)
    if not np.array_equal(np.isnan(a), np.isnan(b)):
        return np.inf
    a, b = np.nan_to_num(a, posinf=3e38, neginf=-3e38), np.nan_to_num(b, posinf=3e38, neginf=-3e38)
    if a.size == 0:
        return 0.0
    mag = np.minimum(np.maximum(np.maximum(np.abs(a), np.abs(b)), th2), 3e38).astype(F)
    return float(np.max(np.abs(a - b) / np.spacing(mag).astype(D)))


def distances(a, b, th2=10.0):
    """the measured distance between two results in each output the tolerance names"""
    d = dict(state=state_rel(a["state"], b["state"]), s12=block_steps(a["S12_out"], b["S12_out"], S12_BLOCKS), chi2=chi2_steps(a["chi2"], b["chi2"], th2),
             final=final_rel(a, b, th2), tcw=0.0, ow=0.0)
    if "Tcw" in a and "Tcw" in b:
        d["tcw"], d["ow"] = block_steps(a["Tcw"], b["Tcw"], TCW_BLOCKS), block_steps(a["Ow"], b["Ow"], (slice(0, 3),))
    return d


def outputs_agree(a, b, tol):
    """what differs between two results under the comparison rules, as a list of strings: the decisions must be equal, the numbers within tol,
    and the trajectory counts only within their static bounds"""
    bad = [f"{k} differs" for k in same_decisions(a, b)]
    for tag, r in (("first", a), ("second", b)):
        if not header_in_bounds(np.asarray(r["header"])):
            bad.append(f"header[8:16] of the {tag} out of bounds: {np.asarray(r['header'])[8:].tolist()}")
    d = distances(a, b)
    for k in Tol._fields:
        if not d[k] <= getattr(tol, k):
            bad.append(f"{k}: {d[k]} apart (allowed {getattr(tol, k)})")
    return bad
