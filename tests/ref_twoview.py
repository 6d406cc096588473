"""TwoViewReconstruction::Reconstruct for the Pinhole camera, restated in numpy from the contract of xfh_two_view_device (include/xfeat_hip.h):
the "rule" form, which follows the orders and the fp64 Jacobi the header fixes and which the library (xfeatslam_amd/csrc/twoview_math.h, host and
device) must equal by bits.  Vectorised over the iterations / matches, never over the terms of one sum: every float operation is one numpy
operation on float32 (or, where the header names a double, float64) operands, so each is rounded exactly as the C++ line it restates."""
from __future__ import annotations

import numpy as np

F = np.float32
D = np.float64
(TOO_FEW, BOTH_ZERO, H_DEGENERATE, F_NO_WINNER, H_GATES, LOW_PARALLAX, OK_H, OK_F) = range(8)
STATUS_NAMES = ("TOO_FEW", "BOTH_ZERO", "H_DEGENERATE", "F_NO_WINNER", "H_GATES", "LOW_PARALLAX", "OK_H", "OK_F")
MODEL_H, MODEL_F = 1, 2
HEADER_INTS, FLOATS, LANES = 24, 48, 256
HEADER = ("N", "status", "model", "win_h", "win_f") + tuple(f"ngood{h}" for h in range(8)) + ("chosen", "inliers_h", "inliers_f", "n_tri", "n_hyp",
                                                                                             "n_matches_out")
F_SH, F_SF, F_RH, F_H21, F_F21, F_T21, F_COS = 0, 1, 2, 3, 12, 21, 33
DEFAULT_COS = float(np.cos(1.0 * np.pi / 180.0))


def inv_d(x):
    """(float)(1.0 / (double)x)"""
    with np.errstate(all="ignore"):
        return (1.0 / np.asarray(x, F).astype(D)).astype(F)


# ---- the minimal sets ------------------------------------------------------------------------------------------------------------------------
def draw_index(draw: int, rand_max: int, d: int) -> int:
    v = (float(draw) / (float(rand_max) + 1.0)) * float(d)
    return 0 if not v >= 0.0 else (d - 1 if v >= float(d) else int(v))


def set_of_iteration(draws8, rand_max: int, N: int):
    """the shrinking vAvailableIndices loop (TwoViewReconstruction.cc:83-98), transcribed with the vector itself"""
    avail = list(range(N))
    out = []
    for j in range(8):
        r = draw_index(int(draws8[j]), rand_max, len(avail))
        out.append(avail[r])
        avail[r] = avail[-1]
        avail.pop()
    return out


# ---- sums -----------------------------------------------------------------------------------------------------------------------------------
def lane_sum(terms):
    """the rule's sum over the last axis: 256 lanes, lane l adds the terms l, l + 256, .. in order to 0.0f; then s[l] += s[l + h], h = 128 .. 1"""
    t = np.asarray(terms, F)
    lead, n = t.shape[:-1], t.shape[-1]
    k = max(1, -(-n // LANES))
    pad = np.zeros(lead + (k * LANES,), F)
    pad[..., :n] = t
    pad = pad.reshape(lead + (k, LANES))
    with np.errstate(all="ignore"):
        acc = np.zeros(lead + (LANES,), F)
        if n:
            for r in range(k):
                row = pad[..., r, :]
                live = (np.arange(LANES) + r * LANES) < n                 # a lane adds only the terms it has
                acc = np.where(live, acc + row, acc)
        h = LANES // 2
        while h >= 1:
            acc = acc[..., :h] + acc[..., h:2 * h]
            h //= 2
    return acc[..., 0]


def normalize(xy):
    """(meanX, meanY, sX, sY) of one frame"""
    xy = np.asarray(xy, F)
    n = F(len(xy))
    out = np.zeros(4, F)
    with np.errstate(all="ignore"):
        for d in range(2):
            mean = F(lane_sum(xy[:, d]) / n)
            dev = F(lane_sum(np.abs(xy[:, d] - mean)) / n)
            out[d], out[2 + d] = mean, inv_d(dev)
    return out


def normalized(nrm, xy):
    return np.stack([(xy[..., 0] - nrm[0]) * nrm[2], (xy[..., 1] - nrm[1]) * nrm[3]], -1).astype(F)


# ---- the fp64 one-sided Jacobi, vectorised over a batch of matrices -----------------------------------------------------------------------------
def _coldot(a, b):
    s = a[:, 0] * b[:, 0]
    for r in range(1, a.shape[1]):
        s = s + a[:, r] * b[:, r]
    return s


def jacobi(A):
    """A [K][M][N] -> (U = A V with orthogonal columns, V), each matrix exactly as tv_jacobi / triang_null_vector iterate it"""
    U = np.array(A, D)
    K, M, N = U.shape
    V = np.tile(np.eye(N), (K, 1, 1))
    with np.errstate(all="ignore"):
        for _ in range(30):
            any_rot = False
            for p in range(N - 1):
                for q in range(p + 1, N):
                    up, uq = U[:, :, p].copy(), U[:, :, q].copy()
                    alpha, beta, gamma = _coldot(up, up), _coldot(uq, uq), _coldot(up, uq)
                    rot = np.abs(gamma) > 1e-15 * np.sqrt(alpha * beta)
                    if not rot.any():
                        continue
                    any_rot = True
                    zeta = (beta - alpha) / (2.0 * gamma)
                    t = np.where(zeta < 0.0, -1.0, 1.0) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                    c = 1.0 / np.sqrt(1.0 + t * t)
                    s = c * t
                    c, s, r = c[:, None], s[:, None], rot[:, None]
                    U[:, :, p] = np.where(r, c * up - s * uq, up)
                    U[:, :, q] = np.where(r, s * up + c * uq, uq)
                    vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                    V[:, :, p] = np.where(r, c * vp - s * vq, vp)
                    V[:, :, q] = np.where(r, s * vp + c * vq, vq)
            if not any_rot:
                break
    return U, V


def min_col(U):
    """index of the column of least squared norm, the first on a tie (a NaN never replaces)"""
    K, M, N = U.shape
    bn = _coldot(U[:, :, 0], U[:, :, 0])
    best = np.zeros(K, np.int64)
    for c in range(1, N):
        n = _coldot(U[:, :, c], U[:, :, c])
        m = n < bn
        bn, best = np.where(m, n, bn), np.where(m, c, best)
    return best


def null_vector(A):
    U, V = jacobi(A)
    k = min_col(U)
    return V[np.arange(len(k)), :, k]


def order3(U):
    n2 = [float(_coldot(U[None, :, c], U[None, :, c])[0]) for c in range(3)]
    o = [0, 1, 2]
    for a in range(1, 3):
        b = a
        while b > 0 and n2[o[b]] > n2[o[b - 1]]:
            o[b], o[b - 1] = o[b - 1], o[b]
            b -= 1
    return o, n2


def design_h(p1, p2):
    """p1, p2 [K][8][2] normalised -> the 16 x 9 matrices of ComputeH21, float32"""
    p1, p2 = np.asarray(p1, F), np.asarray(p2, F)
    K = len(p1)
    A = np.zeros((K, 16, 9), F)
    u1, v1, u2, v2 = p1[..., 0], p1[..., 1], p2[..., 0], p2[..., 1]
    one = np.ones_like(u1)
    with np.errstate(all="ignore"):
        A[:, 0::2, 3], A[:, 0::2, 4], A[:, 0::2, 5] = -u1, -v1, -one
        A[:, 0::2, 6], A[:, 0::2, 7], A[:, 0::2, 8] = v2 * u1, v2 * v1, v2
        A[:, 1::2, 0], A[:, 1::2, 1], A[:, 1::2, 2] = u1, v1, one
        A[:, 1::2, 6], A[:, 1::2, 7], A[:, 1::2, 8] = (-u2) * u1, (-u2) * v1, -u2
    return A


def design_f(p1, p2):
    """the 8 x 9 matrices of ComputeF21"""
    p1, p2 = np.asarray(p1, F), np.asarray(p2, F)
    u1, v1, u2, v2 = p1[..., 0], p1[..., 1], p2[..., 0], p2[..., 1]
    with np.errstate(all="ignore"):
        return np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones_like(u1)], -1).astype(F)


def fit_h(p1, p2):
    """p1, p2 [K][8][2] normalised -> Hn [K][9]"""
    return null_vector(design_h(p1, p2)).astype(F)


def fit_f(p1, p2):
    A = design_f(p1, p2)
    K = len(A)
    with np.errstate(all="ignore"):
        f = null_vector(A).astype(F)
        U, V = jacobi(f.reshape(K, 3, 3))
        out = np.zeros((K, 9), F)
        for k in range(K):
            o, _ = order3(U[k])
            for r in range(3):
                for c in range(3):
                    out[k, r * 3 + c] = F(U[k, r, o[0]] * V[k, c, o[0]] + U[k, r, o[1]] * V[k, c, o[1]])
    return out


def times_T(X, nrm):
    """X [K][9] times T(nrm)"""
    tx, ty = (-nrm[0]) * nrm[2], (-nrm[1]) * nrm[3]
    M = np.zeros_like(X)
    for r in range(3):
        M[:, r * 3] = X[:, r * 3] * nrm[2]
        M[:, r * 3 + 1] = X[:, r * 3 + 1] * nrm[3]
        M[:, r * 3 + 2] = (X[:, r * 3] * tx + X[:, r * 3 + 1] * ty) + X[:, r * 3 + 2]
    return M


def det3(A):
    A = [A[..., k] for k in range(9)]
    return (A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6])) + A[2] * (A[3] * A[7] - A[4] * A[6])


def inv3(Am):
    A = [Am[..., k] for k in range(9)]
    i = F(1.0) / det3(Am)
    return np.stack([(A[4] * A[8] - A[5] * A[7]) * i, (A[2] * A[7] - A[1] * A[8]) * i, (A[1] * A[5] - A[2] * A[4]) * i,
                     (A[5] * A[6] - A[3] * A[8]) * i, (A[0] * A[8] - A[2] * A[6]) * i, (A[2] * A[3] - A[0] * A[5]) * i,
                     (A[3] * A[7] - A[4] * A[6]) * i, (A[1] * A[6] - A[0] * A[7]) * i, (A[0] * A[4] - A[1] * A[3]) * i], -1).astype(F)


def compose_h(Hn, nrm1, nrm2):
    with np.errstate(all="ignore"):
        M = times_T(np.asarray(Hn, F), nrm1)
        ix, iy = F(1.0) / nrm2[2], F(1.0) / nrm2[3]
        out = np.zeros((len(M), 18), F)
        for c in range(3):
            out[:, c] = ix * M[:, c] + nrm2[0] * M[:, 6 + c]
            out[:, 3 + c] = iy * M[:, 3 + c] + nrm2[1] * M[:, 6 + c]
            out[:, 6 + c] = M[:, 6 + c]
        out[:, 9:] = inv3(out[:, :9])
    return out


def compose_f(Fn, nrm1, nrm2):
    with np.errstate(all="ignore"):
        M = times_T(np.asarray(Fn, F), nrm1)
        tx, ty = (-nrm2[0]) * nrm2[2], (-nrm2[1]) * nrm2[3]
        out = np.zeros((len(M), 18), F)
        for c in range(3):
            out[:, c] = nrm2[2] * M[:, c]
            out[:, 3 + c] = nrm2[3] * M[:, 3 + c]
            out[:, 6 + c] = (tx * M[:, c] + ty * M[:, 3 + c]) + M[:, 6 + c]
    return out


# ---- scores ---------------------------------------------------------------------------------------------------------------------------------
def inv_sigma2(sigma):
    return inv_d(F(sigma) * F(sigma))


def score_terms(model, M, sigma, u1, v1, u2, v2):
    """M [K][18], the coordinates [N] -> chi [K][N][2], inlier [K][N], share of the score [K][N]"""
    M = np.asarray(M, F)
    m = [M[:, k, None] for k in range(M.shape[1])]
    is2 = inv_sigma2(sigma)
    with np.errstate(all="ignore"):
        if model == MODEL_H:
            g = m[9:]
            w2 = inv_d((g[6] * u2 + g[7] * v2) + g[8])
            a, b = ((g[0] * u2 + g[1] * v2) + g[2]) * w2, ((g[3] * u2 + g[4] * v2) + g[5]) * w2
            chi1 = ((u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)) * is2
            w1 = inv_d((m[6] * u1 + m[7] * v1) + m[8])
            c, d = ((m[0] * u1 + m[1] * v1) + m[2]) * w1, ((m[3] * u1 + m[4] * v1) + m[5]) * w1
            chi2 = ((u2 - c) * (u2 - c) + (v2 - d) * (v2 - d)) * is2
            th = ts = F(5.991)
        else:
            a2, b2, c2 = (m[0] * u1 + m[1] * v1) + m[2], (m[3] * u1 + m[4] * v1) + m[5], (m[6] * u1 + m[7] * v1) + m[8]
            num2 = (a2 * u2 + b2 * v2) + c2
            chi1 = ((num2 * num2) / (a2 * a2 + b2 * b2)) * is2
            a1, b1, c1 = (m[0] * u2 + m[3] * v2) + m[6], (m[1] * u2 + m[4] * v2) + m[7], (m[2] * u2 + m[5] * v2) + m[8]
            num1 = (a1 * u1 + b1 * v1) + c1
            chi2 = ((num1 * num1) / (a1 * a1 + b1 * b1)) * is2
            th, ts = F(3.841), F(5.991)
        o1, o2 = chi1 > th, chi2 > th
        term = np.where(o1, F(0), ts - chi1) + np.where(o2, F(0), ts - chi2)
    return np.stack([chi1, chi2], -1).astype(F), ~o1 & ~o2, term.astype(F)


def argmax(score):
    w, s = -1, F(0)
    for it, v in enumerate(score):
        if v > s:
            s, w = v, it
    return w, F(s)


# ---- motion hypotheses --------------------------------------------------------------------------------------------------------------------------
def svd3(A9, rank2):
    U, V = jacobi(np.asarray(A9, F).reshape(1, 3, 3))
    U, V = U[0], V[0]
    o, n2 = order3(U)
    u, v, w = np.zeros((3, 3), D), np.zeros((3, 3), F), np.zeros(3, F)
    with np.errstate(all="ignore"):
        for k in range(3):
            wk = np.sqrt(D(n2[o[k]]))
            w[k] = F(wk)
            u[:, k] = U[:, o[k]] / wk
            v[:, k] = V[:, o[k]].astype(F)
        if rank2:
            u[0, 2] = u[1, 0] * u[2, 1] - u[2, 0] * u[1, 1]
            u[1, 2] = u[2, 0] * u[0, 1] - u[0, 0] * u[2, 1]
            u[2, 2] = u[0, 0] * u[1, 1] - u[1, 0] * u[0, 1]
    return u.astype(F), v, w


def times_K(X, cam):
    fx, fy, cx, cy = cam
    G = np.zeros(9, F)
    for r in range(3):
        G[r * 3], G[r * 3 + 1] = X[r * 3] * fx, X[r * 3 + 1] * fy
        G[r * 3 + 2] = (X[r * 3] * cx + X[r * 3 + 1] * cy) + X[r * 3 + 2]
    return G


def unit3(t):
    n = np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
    return np.array([t[0] / n, t[1] / n, t[2] / n], F)


def motions_f(F21, cam):
    cam = [F(c) for c in cam]
    fx, fy, cx, cy = cam
    Rt = np.zeros((4, 12), F)
    with np.errstate(all="ignore"):
        G = times_K(np.asarray(F21, F), cam)
        E = np.zeros(9, F)
        for c in range(3):
            E[c], E[3 + c], E[6 + c] = fx * G[c], fy * G[3 + c], (cx * G[c] + cy * G[3 + c]) + G[6 + c]
        U, V, _ = svd3(E, True)
        t = unit3(U[:, 2])
        R1, R2 = np.zeros(9, F), np.zeros(9, F)
        for r in range(3):
            for c in range(3):
                R1[r * 3 + c] = (U[r, 1] * V[c, 0] - U[r, 0] * V[c, 1]) + U[r, 2] * V[c, 2]
                R2[r * 3 + c] = (U[r, 0] * V[c, 1] - U[r, 1] * V[c, 0]) + U[r, 2] * V[c, 2]
        if det3(R1) < 0:
            R1 = -R1
        if det3(R2) < 0:
            R2 = -R2
        for h in range(4):
            Rt[h].reshape(3, 4)[:, :3] = (R2 if h & 1 else R1).reshape(3, 3)
            Rt[h].reshape(3, 4)[:, 3] = t if h < 2 else -t
    return Rt


def motions_h(H21, cam):
    """-> Rt [8][12], or None when the singular values are too close"""
    cam = [F(c) for c in cam]
    fx, fy, cx, cy = cam
    with np.errstate(all="ignore"):
        G = times_K(np.asarray(H21, F), cam)
        ifx, ify = F(1.0) / fx, F(1.0) / fy
        icx, icy = (-cx) * ifx, (-cy) * ify
        A = np.zeros(9, F)
        for c in range(3):
            A[c], A[3 + c], A[6 + c] = ifx * G[c] + icx * G[6 + c], ify * G[3 + c] + icy * G[6 + c], G[6 + c]
        U, V, w = svd3(A, False)
        s = F(det3(U.reshape(9)) * det3(V.reshape(9)))
        d1, d2, d3 = w
        if D(d1 / d2) < 1.00001 or D(d2 / d3) < 1.00001:
            return None
        aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
        aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
        x1, x3 = [aux1, aux1, -aux1, -aux1], [aux3, -aux3, aux3, -aux3]
        root = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3))
        ast, ct = root / ((d1 + d3) * d2), (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
        asp, cp = root / ((d1 - d3) * d2), (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
        sgn = [F(1), F(-1), F(-1), F(1)]
        Rt = np.zeros((8, 12), F)
        for h in range(8):
            i, second = h & 3, h >= 4
            sn = sgn[i] * (asp if second else ast)
            X = np.zeros((3, 3), F)
            for r in range(3):
                if not second:
                    X[r, 0], X[r, 1], X[r, 2] = U[r, 0] * ct + U[r, 2] * sn, U[r, 1], U[r, 2] * ct - U[r, 0] * sn
                else:
                    X[r, 0], X[r, 1], X[r, 2] = U[r, 0] * cp + U[r, 2] * sn, -U[r, 1], U[r, 0] * sn - U[r, 2] * cp
            if not second:
                tp0, tp2 = x1[i] * (d1 - d3), (-x3[i]) * (d1 - d3)
            else:
                tp0, tp2 = x1[i] * (d1 + d3), x3[i] * (d1 + d3)
            t = unit3(np.array([U[r, 0] * tp0 + U[r, 2] * tp2 for r in range(3)], F))
            for r in range(3):
                for c in range(3):
                    Rt[h, r * 4 + c] = s * ((X[r, 0] * V[c, 0] + X[r, 1] * V[c, 1]) + X[r, 2] * V[c, 2])
                Rt[h, r * 4 + 3] = t[r]
    return Rt


# ---- CheckRT ----------------------------------------------------------------------------------------------------------------------------------
def th2_of(sigma):
    return F(4.0 * D(F(sigma) * F(sigma)))


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def check_rt(cam, Rt, sigma, x1, y1, x2, y2, null=None):
    """one hypothesis, the pairs [n] -> verdict [n] (0 not counted, 1 counted, 2 counted and good), cos [n], p [n][3].  null: another null vector
    of the 4 x 4 matrices than the rule's (the literal form passes a float32 SVD)"""
    fx, fy, cx, cy = [F(c) for c in cam]
    Rt = np.asarray(Rt, F)
    x1, y1, x2, y2 = [np.asarray(a, F) for a in (x1, y1, x2, y2)]
    n = len(x1)
    if n == 0:
        return np.zeros(0, np.uint8), np.zeros(0, F), np.zeros((0, 3), F)
    z, o = F(0), F(1)
    with np.errstate(all="ignore"):
        P1 = np.array([[fx, z, cx, z], [z, fy, cy, z], [z, z, o, z]], F)
        P2 = np.stack([fx * Rt[0:4] + cx * Rt[8:12], fy * Rt[4:8] + cy * Rt[8:12], Rt[8:12]]).astype(F)
        A = np.zeros((n, 4, 4), F)
        A[:, 0] = x1[:, None] * P1[2][None] - P1[0][None]
        A[:, 1] = y1[:, None] * P1[2][None] - P1[1][None]
        A[:, 2] = x2[:, None] * P2[2][None] - P2[0][None]
        A[:, 3] = y2[:, None] * P2[2][None] - P2[1][None]
        h = (null_vector if null is None else null)(A).astype(F)
        p = [h[:, 0] / h[:, 3], h[:, 1] / h[:, 3], h[:, 2] / h[:, 3]]
        finite = np.isfinite(p[0]) & np.isfinite(p[1]) & np.isfinite(p[2])
        O2 = [-((Rt[c] * Rt[3] + Rt[4 + c] * Rt[7]) + Rt[8 + c] * Rt[11]) for c in range(3)]
        n2 = [p[c] - O2[c] for c in range(3)]
        dist1, dist2 = np.sqrt(dot3(p, p)), np.sqrt(dot3(n2, n2))
        cosv = dot3(p, n2) / (dist1 * dist2)
        par = cosv.astype(D) < 0.99998
        q = [dot3(Rt[4 * r:4 * r + 3], p) + Rt[4 * r + 3] for r in range(3)]
        th2 = th2_of(sigma)
        iz1 = inv_d(p[2])
        e1x, e1y = (fx * p[0] * iz1 + cx) - x1, (fy * p[1] * iz1 + cy) - y1
        iz2 = inv_d(q[2])
        e2x, e2y = (fx * q[0] * iz2 + cx) - x2, (fy * q[1] * iz2 + cy) - y2
        bad = ~finite | ((p[2] <= 0) & par) | ((q[2] <= 0) & par) | (e1x * e1x + e1y * e1y > th2) | (e2x * e2x + e2y * e2y > th2)
    verdict = np.where(bad, 0, np.where(par, 2, 1)).astype(np.uint8)
    return verdict, np.where(finite, cosv, F(0)).astype(F), np.stack(p, -1).astype(F)


def float_key(f):
    u = np.asarray(f, F).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def cos_at_index(cosv):
    """the value at sorted index min(50, n - 1); 1.0f for an empty list"""
    if len(cosv) == 0:
        return F(1.0)
    c = np.asarray(cosv, F)
    return c[np.argsort(float_key(c), kind="stable")][min(50, len(c) - 1)]


def decide(model, h_degenerate, ngood, cosk, n_inl, min_parallax_cos, min_tri):
    if model == MODEL_F:
        mx = max(ngood[:4])
        nmin = max(int(0.9 * float(n_inl)), min_tri)
        nsim = sum(float(g) > 0.7 * float(mx) for g in ngood[:4])
        if mx < nmin or nsim > 1:
            return F_NO_WINNER, -1
        h = list(ngood[:4]).index(mx)
        return (OK_F, h) if float(cosk[h]) < min_parallax_cos else (LOW_PARALLAX, -1)
    if h_degenerate:
        return H_DEGENERATE, -1
    best = second = 0
    idx = -1
    for h in range(8):
        if ngood[h] > best:
            second, best, idx = best, ngood[h], h
        elif ngood[h] > second:
            second = ngood[h]
    if not (float(second) < 0.75 * float(best) and best > min_tri and float(best) > 0.9 * float(n_inl)) or idx < 0:
        return H_GATES, -1
    if not float(cosk[idx]) <= min_parallax_cos:
        return LOW_PARALLAX, -1
    return OK_H, idx


# ---- the whole rule for one problem --------------------------------------------------------------------------------------------------------------
def rule(xy1, xy2, m12, cam, draws, rand_max, sigma=1.0, min_parallax_cos=DEFAULT_COS, min_tri=50, prior=None):
    """-> dict(header [24], floats [48], inl_h, inl_f, tri [n1], p3d [n1][3], matches_out [n1]) as the call writes them, and the intermediate
    sets / hyp / score.  prior: the outputs' earlier content (what a TOO_FEW call leaves untouched); zeros / matches12 by default."""
    xy1, xy2, m12 = np.asarray(xy1, F).reshape(-1, 2), np.asarray(xy2, F).reshape(-1, 2), np.asarray(m12, np.int32)
    draws = np.asarray(draws, np.int32).reshape(-1, 8)
    n1, n2, iters = len(xy1), len(xy2), len(draws)
    ok = (m12 >= 0) & (m12 < n2)
    cm1 = np.nonzero(ok)[0]
    cm2 = m12[cm1]
    N = len(cm1)
    hdr, fo = np.zeros(HEADER_INTS, np.int32), np.zeros(FLOATS, F)
    r = dict(header=hdr, floats=fo, inl_h=np.zeros(n1, np.uint8), inl_f=np.zeros(n1, np.uint8), tri=np.zeros(n1, np.uint8), p3d=np.zeros((n1, 3), F),
             matches_out=m12.copy())
    if prior is not None:
        r.update({k: np.array(v) for k, v in prior.items() if k != "header"})
    hdr[0] = N
    if N < 8:
        hdr[1], hdr[3], hdr[4], hdr[13] = TOO_FEW, -1, -1, -1
        return r
    r["floats"] = fo
    nrm1, nrm2 = normalize(xy1), normalize(xy2)
    sets = np.array([set_of_iteration(d, rand_max, N) for d in draws], np.int64)
    p1, p2 = normalized(nrm1, xy1[cm1[sets]]), normalized(nrm2, xy2[cm2[sets]])
    hyp = np.stack([compose_h(fit_h(p1, p2), nrm1, nrm2), compose_f(fit_f(p1, p2), nrm1, nrm2)])
    u1, v1, u2, v2 = xy1[cm1, 0], xy1[cm1, 1], xy2[cm2, 0], xy2[cm2, 1]
    score = np.stack([lane_sum(score_terms(m + 1, hyp[m], sigma, u1, v1, u2, v2)[2]) for m in range(2)])
    (winH, SH), (winF, SF) = argmax(score[0]), argmax(score[1])
    MH = hyp[0, winH] if winH >= 0 else np.zeros(18, F)
    MF = hyp[1, winF] if winF >= 0 else np.zeros(18, F)
    inl_h, inl_f = np.zeros(n1, np.uint8), np.zeros(n1, np.uint8)
    if winH >= 0:
        inl_h[cm1] = score_terms(MODEL_H, MH[None], sigma, u1, v1, u2, v2)[1][0]
    if winF >= 0:
        inl_f[cm1] = score_terms(MODEL_F, MF[None], sigma, u1, v1, u2, v2)[1][0]
    fo[F_SH], fo[F_SF] = SH, SF
    fo[F_H21:F_H21 + 9], fo[F_F21:F_F21 + 9] = MH[:9], MF[:9]
    model, Rt, hdeg = 0, np.zeros((0, 12), F), False
    with np.errstate(all="ignore"):
        both = F(SH + SF)
    if both != 0:
        RH = F(SH / both)
        fo[F_RH] = RH
        model = MODEL_H if D(RH) > 0.50 else MODEL_F
        if model == MODEL_H:
            Rt = motions_h(MH[:9], cam)
            hdeg = Rt is None
            if hdeg:
                Rt = np.zeros((0, 12), F)
        else:
            Rt = motions_f(MF[:9], cam)
    inl = inl_h if model == MODEL_H else inl_f
    ninl = int(inl.sum())
    idx = np.nonzero(inl)[0] if model else np.zeros(0, np.int64)
    ngood, cosk, per_h = [0] * 8, [F(1.0)] * 8, []
    for h in range(len(Rt)):
        v, c, p = check_rt(cam, Rt[h], sigma, xy1[idx, 0], xy1[idx, 1], xy2[m12[idx], 0], xy2[m12[idx], 1])
        ngood[h], cosk[h] = int((v != 0).sum()), cos_at_index(c[v != 0])
        per_h.append((v, p))
    status, chosen = (BOTH_ZERO, -1) if model == 0 else decide(model, hdeg, ngood, cosk, ninl, min_parallax_cos, min_tri)
    tri, p3d, mo = np.zeros(n1, np.uint8), np.zeros((n1, 3), F), m12.copy()
    if chosen >= 0:
        v, p = per_h[chosen]
        tri[idx] = v == 2
        p3d[idx[v != 0]] = p[v != 0]
        mo[ok & (tri == 0)] = -1
        fo[F_T21:F_T21 + 12] = Rt[chosen]
    ntri = int(tri.sum())
    hdr[1:5] = status, model, winH, winF
    hdr[5:13] = ngood
    hdr[13:19] = chosen, int(inl_h.sum()), int(inl_f.sum()), ntri, len(Rt), ntri if chosen >= 0 else N
    fo[F_COS:F_COS + 8] = cosk
    r.update(inl_h=inl_h, inl_f=inl_f, tri=tri, p3d=p3d, matches_out=mo, sets=sets, hyp=hyp, score=score, nrm=(nrm1, nrm2), motions=Rt,
             cm=(cm1, cm2))
    return r


OUTPUTS = ("header", "floats", "inl_h", "inl_f", "tri", "p3d", "matches_out")
