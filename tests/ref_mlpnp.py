"""The rule of xfh_mlpnp_solve_device (include/xfeat_hip.h), restated line by line in plain Python: IEEE doubles (Python floats) in the order the
contract writes them, numpy float32 scalars where it names a float.  No numpy linear algebra: every sum, Jacobi rotation and Householder step is
spelled out, so that the host form (xfh_mlpnp_solve_host) and the kernels can be held against it integer for integer.  The four libm functions of the
rule (sin, cos, acos, cbrt) go through LIBM, one hook, so that a test can nudge every result by a few ulp and see that no decision of a scene hangs
on the last bits of a libm (tests/test_mlpnp_ref.py); `trace`, when set to a list, receives (kind, value, bound) for every inlier test and every
Gauss-Newton decision."""
import math

import numpy as np

F = np.float32
TOO_FEW, NONE, BEST, REFINED = range(4)
STATUS = ("TOO_FEW", "NONE", "BEST", "REFINED")
HEADER = ("N", "status", "its", "min_inliers", "winner", "n_inliers", "best", "best_count", "consumed", "refines", "planar")
OUTPUTS = ("header", "Tcw", "inliers", "assigned_out")
LANES, MAX_SWEEPS, JACOBI_TOL, MIN_SET, GN_ROUNDS, GN_EPS = 256, 30, 1e-15, 6, 5, 1e-5
EPS = 2.220446049250313e-16
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31

LIBM = dict(sin=math.sin, cos=math.cos, acos=math.acos, cbrt=getattr(math, "cbrt", None) or (lambda x: float(np.cbrt(x))))
trace = None


def _note(kind, value, bound):
    if trace is not None:
        trace.append((kind, float(value), float(bound)))


def lm(name, x):
    """one libm function of the rule through the hook; a NaN or Inf argument gives NaN (math raises there)"""
    return LIBM[name](x) if math.isfinite(x) else float("nan")


def sqrt(x):
    return math.sqrt(x) if x >= 0.0 else float("nan")


def div(a, b):
    """IEEE division of doubles (Python raises on a zero divisor)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


# ---- step 2 ------------------------------------------------------------------------------------------------------------------------------------
def params(prob, min_inliers, max_its, min_set, eps, N):
    """-> (its, min_inliers_eff) of SetRansacParameters for N correspondences"""
    with np.errstate(all="ignore"):
        eps = F(eps)
        nmin = int(F(N) * eps)
        nmin = max(nmin, min_inliers, min_set)
        e = eps
        ratio = F(nmin) / F(N)
        if e < ratio:
            e = ratio
        if nmin == N:
            n = 1
        else:
            v = np.ceil(np.log(np.float64(1.0 - prob)) / np.log(np.float64(1.0) - np.power(np.float64(e), 3.0)))
            if not np.isfinite(v) or v > INT_MAX or v < INT_MIN:
                return max(max_its, 1), nmin
            n = int(v)
        return max(1, min(n, max_its)), nmin


def iterations_table(n, prob=0.99, min_inliers=10, max_its=300, min_set=6, eps=0.5):
    t = [params(prob, min_inliers, max_its, min_set, eps, N) for N in range(n + 1)]
    return np.array([a for a, _ in t], np.int32), np.array([b for _, b in t], np.int32)


# ---- step 4 ------------------------------------------------------------------------------------------------------------------------------------
def draw_index(draw, rand_max, d):
    v = (float(draw) / (float(rand_max) + 1.0)) * float(d)
    return 0 if not (v >= 0.0) else (d - 1 if v >= float(d) else int(v))


def make_set(draws6, rand_max, N):
    avail = list(range(N))
    out = []
    for j in range(MIN_SET):
        r = draw_index(int(draws6[j]), rand_max, len(avail))
        out.append(avail[r])
        avail[r] = avail[-1]
        avail.pop()
    return out


# ---- step 1, 5 (a) ---------------------------------------------------------------------------------------------------------------------------------
def bearing(cam, x, y):
    fx, fy, cx, cy = [F(v) for v in cam]
    return [float((F(x) - cx) / fx), float((F(y) - cy) / fy), 1.0]


def nullspace(f):
    n = sqrt((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2])
    sg = n if f[0] >= 0.0 else -n
    v = [f[0] + sg, f[1], f[2]]
    vv = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
    c1, c2 = div(2.0 * v[1], vv), div(2.0 * v[2], vv)
    return [-(c1 * v[0]), 1.0 - c1 * v[1], -(c1 * v[2])], [-(c2 * v[0]), -(c2 * v[1]), 1.0 - c2 * v[2]]


# ---- small algebra -------------------------------------------------------------------------------------------------------------------------------
def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def norm3(a):
    return sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])


def mv(M, v):
    return [(M[3 * r] * v[0] + M[3 * r + 1] * v[1]) + M[3 * r + 2] * v[2] for r in range(3)]


def mtv(M, v):
    return [(M[c] * v[0] + M[3 + c] * v[1]) + M[6 + c] * v[2] for c in range(3)]


def det3(A):
    return (A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6])) + A[2] * (A[3] * A[7] - A[4] * A[6])


def jacobi_rotation(alpha, beta, gamma):
    if not (abs(gamma) > JACOBI_TOL * sqrt(alpha * beta)):
        return None
    zeta = div(beta - alpha, 2.0 * gamma)
    t = div(-1.0 if zeta < 0.0 else 1.0, abs(zeta) + sqrt(1.0 + zeta * zeta))
    c = div(1.0, sqrt(1.0 + t * t))
    return c, c * t


def jacobi(U, n):
    """U (row-major n x n list, changed in place) <- U V; returns V"""
    V = [1.0 if r == c else 0.0 for r in range(n) for c in range(n)]
    for _ in range(MAX_SWEEPS):
        rot = 0
        for p in range(n - 1):
            for q in range(p + 1, n):
                alpha, beta, gamma = U[p] * U[p], U[q] * U[q], U[p] * U[q]
                for r in range(1, n):
                    up, uq = U[r * n + p], U[r * n + q]
                    alpha, beta, gamma = alpha + up * up, beta + uq * uq, gamma + up * uq
                cs = jacobi_rotation(alpha, beta, gamma)
                if cs is None:
                    continue
                c, s = cs
                for r in range(n):
                    up, uq, vp, vq = U[r * n + p], U[r * n + q], V[r * n + p], V[r * n + q]
                    U[r * n + p], U[r * n + q] = c * up - s * uq, s * up + c * uq
                    V[r * n + p], V[r * n + q] = c * vp - s * vq, s * vp + c * vq
                rot += 1
        if rot == 0:
            break
    return V


def col_norm2(U, n, c):
    s = U[c] * U[c]
    for r in range(1, n):
        s = s + U[r * n + c] * U[r * n + c]
    return s


def min_col_last(U, n):
    best, bn = 0, col_norm2(U, n, 0)
    for c in range(1, n):
        v = col_norm2(U, n, c)
        if v <= bn:
            bn, best = v, c
    return best


def order3(U, descending=True):
    n2 = [col_norm2(U, 3, c) for c in range(3)]
    o = [0, 1, 2]
    for a in range(1, 3):
        b = a
        while b > 0 and (n2[o[b]] > n2[o[b - 1]] if descending else n2[o[b]] < n2[o[b - 1]]):
            o[b], o[b - 1] = o[b - 1], o[b]
            b -= 1
    return o


def nearest_rotation(A):
    U = list(A)
    V = jacobi(U, 3)
    o = order3(U)
    w = [sqrt(col_norm2(U, 3, o[k])) for k in range(3)]
    return [(div(U[3 * i + o[0]], w[0]) * V[3 * j + o[0]] + div(U[3 * i + o[1]], w[1]) * V[3 * j + o[1]]) + div(U[3 * i + o[2]], w[2]) * V[3 * j + o[2]]
            for i in range(3) for j in range(3)]


def rank3(S6):
    A = [[S6[0], S6[1], S6[2]], [S6[1], S6[3], S6[4]], [S6[2], S6[4], S6[5]]]
    piv, first = [], 0.0
    for k in range(3):
        big, br, bc = -1.0, k, k
        for r in range(k, 3):
            for c in range(k, 3):
                a = abs(A[r][c])
                if a > big:
                    big, br, bc = a, r, c
        if k == 0:
            first = big
        if not (big > 3.0 * EPS * first):
            break
        A[k], A[br] = A[br], A[k]
        for r in range(3):
            A[r][k], A[r][bc] = A[r][bc], A[r][k]
        ss = 0.0
        for r in range(k, 3):
            ss = ss + A[r][k] * A[r][k]
        nrm = sqrt(ss)
        piv.append(nrm)
        if k == 2:
            break
        v = [0.0, 0.0, 0.0]
        for r in range(k, 3):
            v[r] = A[r][k]
        v[k] = v[k] - (-nrm if A[k][k] >= 0.0 else nrm)
        vv = 0.0
        for r in range(k, 3):
            vv = vv + v[r] * v[r]
        for c in range(k + 1, 3):
            d = 0.0
            for r in range(k, 3):
                d = d + v[r] * A[r][c]
            f = div(2.0 * d, vv)
            for r in range(k, 3):
                A[r][c] = A[r][c] - f * v[r]
    mx = 0.0
    for p in piv:
        if p > mx:
            mx = p
    return sum(1 for p in piv if p > 3.0 * EPS * mx)


def eigen_rot(S6):
    U = [S6[0], S6[1], S6[2], S6[1], S6[3], S6[4], S6[2], S6[4], S6[5]]
    V = jacobi(U, 3)
    inc = order3(U, descending=False)
    return [V[3 * c + inc[r]] for r in range(3) for c in range(3)]


def design_rows(r, s, q, planar):
    if planar:
        a, b = [0.0] * 9, [0.0] * 9
        for k in range(3):
            a[2 * k], a[2 * k + 1], a[6 + k] = r[k] * q[1], r[k] * q[2], r[k]
            b[2 * k], b[2 * k + 1], b[6 + k] = s[k] * q[1], s[k] * q[2], s[k]
        return a, b
    a, b = [0.0] * 12, [0.0] * 12
    for k in range(3):
        for c in range(3):
            a[3 * k + c], b[3 * k + c] = r[k] * q[c], s[k] * q[c]
        a[9 + k], b[9 + k] = r[k], s[k]
    return a, b


# ---- step 5 (f) ------------------------------------------------------------------------------------------------------------------------------------
def rodrigues2rot(w):
    n = norm3(w)
    R = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    if not (n > EPS):
        return R
    K = [0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0]
    a, b = div(lm("sin", n), n), div(1.0 - lm("cos", n), n * n)
    for i in range(3):
        for j in range(3):
            kk = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j]
            R[3 * i + j] = (R[3 * i + j] + a * K[3 * i + j]) + b * kk
    return R


def acos(x):
    return lm("acos", x) if -1.0 <= x <= 1.0 else float("nan")


def rot2rodrigues(R):
    trace_ = ((R[0] + R[4]) + R[8]) - 1.0
    wn = acos(trace_ / 2.0)
    if not (wn > EPS):
        return [0.0, 0.0, 0.0]
    sc = div(wn, 2.0 * lm("sin", wn))
    return [(R[7] - R[5]) * sc, (R[2] - R[6]) * sc, (R[3] - R[1]) * sc]


# ---- step 5 (g) ------------------------------------------------------------------------------------------------------------------------------------
def gn_begin(x):
    R = rodrigues2rot(x[:3])
    w = x[:3]
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    K = [0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0]
    D = [R[3 * j + i] - (1.0 if i == j else 0.0) for i in range(3) for j in range(3)]
    P = [0.0] * 9
    for i in range(3):
        for j in range(3):
            q = (D[3 * i] * K[j] + D[3 * i + 1] * K[3 + j]) + D[3 * i + 2] * K[6 + j]
            P[3 * i + j] = div(w[i] * w[j] + q, th2)
    return R, P, x[3:6]


def gn_rows(g, X, r, s):
    R, P, T = g
    q = mv(R, X)
    v = [q[k] + T[k] for k in range(3)]
    nv = norm3(v)
    u = [div(v[k], nv) for k in range(3)]
    res, J = [0.0, 0.0], [0.0] * 12
    for a, n in enumerate((r, s)):
        d = dot3(n, u)
        res[a] = d
        gg = [div(n[k] - d * u[k], nv) for k in range(3)]
        k3 = mtv(R, gg)
        h = [k3[1] * X[2] - k3[2] * X[1], k3[2] * X[0] - k3[0] * X[2], k3[0] * X[1] - k3[1] * X[0]]
        for j in range(3):
            J[6 * a + j] = -((P[j] * h[0] + P[3 + j] * h[1]) + P[6 + j] * h[2])
            J[6 * a + 3 + j] = gg[j]
    return res, J


UPPER6 = [(i, j) for i in range(6) for j in range(i, 6)]


def gn_terms(J, res):
    return [J[i] * J[j] + J[6 + i] * J[6 + j] for i, j in UPPER6] + [J[i] * res[0] + J[6 + i] * res[1] for i in range(6)]


def ldlt_solve(H21, b):
    """the unpivoted LDL^T of xfh_pose_optimize_device; None as soon as a pivot is not > 0"""
    A = [[0.0] * 6 for _ in range(6)]
    n = 0
    for i in range(6):
        for j in range(i, 6):
            A[i][j] = A[j][i] = H21[n]
            n += 1
    for i in range(6):
        A[i][i] = A[i][i] + 0.0
    d = [0.0] * 6
    for j in range(6):
        dj = A[j][j]
        for k in range(j):
            dj = dj - A[j][k] * A[j][k] * d[k]
        if not (dj > 0.0):
            return None
        d[j] = dj
        for i in range(j + 1, 6):
            s = A[i][j]
            for k in range(j):
                s = s - A[i][k] * A[j][k] * d[k]
            A[i][j] = div(s, dj)
    y = [0.0] * 6
    for i in range(6):
        s = b[i]
        for k in range(i):
            s = s - A[i][k] * y[k]
        y[i] = s
    for i in range(6):
        y[i] = div(y[i], d[i])
    x = [0.0] * 6
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s = s - A[k][i] * x[k]
        x[i] = s
    return x


def gn_solve(sums):
    """-> (dx, ends): the 6 x 6 solve and :744"""
    dx = ldlt_solve(sums[:21], sums[21:])
    if dx is None:
        return [0.0] * 6, True
    mx, mn = max(abs(v) for v in dx), min(abs(v) for v in dx)
    _note("gn744", mx, 5.0)
    _note("gn744", mn, 1.0)
    any5 = any(abs(v) > 5.0 for v in dx)
    all1 = all(abs(v) > 1.0 for v in dx)
    return dx, any5 or all1


def gn_not_below(J, dx):
    c = 0
    for a in range(2):
        j = J[6 * a:6 * a + 6]
        d = ((((j[0] * dx[0] + j[1] * dx[1]) + j[2] * dx[2]) + j[3] * dx[3]) + j[4] * dx[4]) + j[5] * dx[5]
        if not (abs(d) < GN_EPS):
            c += 1
    return c, abs(d)


# ---- the sums of step 5 (c) ------------------------------------------------------------------------------------------------------------------------
def rule_sum(idx, fold, term, K):
    """the sums of the K-vectors term(c) over the correspondences idx (ascending): in index order from 0.0, or in the 256-lane fold"""
    if not fold:
        out = [0.0] * K
        for c in idx:
            t = term(c)
            for k in range(K):
                out[k] = out[k] + t[k]
        return out
    s = [[0.0] * LANES for _ in range(K)]
    for c in idx:
        t = term(c)
        l = c % LANES
        for k in range(K):
            s[k][l] = s[k][l] + t[k]
    out = []
    for k in range(K):
        row = s[k]
        h = LANES // 2
        while h >= 1:
            for l in range(h):
                row[l] = row[l] + row[l + h]
            h //= 2
        out.append(row[0])
    return out


# ---- step 5 (d), (e) ---------------------------------------------------------------------------------------------------------------------------------
def linear(AtA, cols, planar, E, f6, p6):
    U = list(AtA)
    V = jacobi(U, cols)
    col = min_col_last(U, cols)
    res = [V[k * cols + col] if k < cols else 0.0 for k in range(12)]
    if planar:
        c1, c2 = [res[0], res[2], res[4]], [res[1], res[3], res[5]]
        c0 = [c1[1] * c2[2] - c1[2] * c2[1], c1[2] * c2[0] - c1[0] * c2[2], c1[0] * c2[1] - c1[1] * c2[0]]
        tmp = c0 + c1 + c2
        k1, k2 = [tmp[1], tmp[4], tmp[7]], [tmp[2], tmp[5], tmp[8]]
        scale = div(1.0, sqrt(abs(norm3(k1) * norm3(k2))))
        R1 = nearest_rotation(tmp)
        if det3(R1) < 0.0:
            R1 = [v * -1.0 for v in R1]
        Rb = [0.0] * 9
        for i in range(3):
            for j in range(3):
                Rb[3 * j + i] = ((E[i] * R1[j] + E[3 + i] * R1[3 + j]) + E[6 + i] * R1[6 + j]) * -1.0
        t = [scale * res[6], scale * res[7], scale * res[8]]
        if det3(Rb) < 0.0:
            Rb[2], Rb[5], Rb[8] = Rb[2] * -1.0, Rb[5] * -1.0, Rb[8] * -1.0
        best, bi = 0.0, 0
        for i in range(4):
            sr, st = (-1.0 if i >= 2 else 1.0), (-1.0 if i & 1 else 1.0)
            norms = 0.0
            for p in range(6):
                P = p6[p]
                v = [(((sr * Rb[3 * r]) * P[0] + (sr * Rb[3 * r + 1]) * P[1]) + Rb[3 * r + 2] * P[2]) + st * t[r] for r in range(3)]
                n = norm3(v)
                v = [div(v[r], n) for r in range(3)]
                norms = norms + (1.0 - dot3(v, f6[p]))
            if i == 0 or norms < best:
                best, bi = norms, i
        sr, st = (-1.0 if bi >= 2 else 1.0), (-1.0 if bi & 1 else 1.0)
        Rout = [0.0] * 9
        for r in range(3):
            Rout[3 * r], Rout[3 * r + 1], Rout[3 * r + 2] = sr * Rb[3 * r], sr * Rb[3 * r + 1], Rb[3 * r + 2]
        tout = [st * t[r] for r in range(3)]
    else:
        tmp = [res[0], res[3], res[6], res[1], res[4], res[7], res[2], res[5], res[8]]
        k0, k1, k2 = [tmp[0], tmp[3], tmp[6]], [tmp[1], tmp[4], tmp[7]], [tmp[2], tmp[5], tmp[8]]
        scale = div(1.0, lm("cbrt", abs((norm3(k0) * norm3(k1)) * norm3(k2))))
        R = nearest_rotation(tmp)
        if det3(R) < 0.0:
            R = [v * -1.0 for v in R]
        ts = [scale * res[9], scale * res[10], scale * res[11]]
        t0 = mv(R, ts)
        ti = mtv(R, t0)
        err = [0.0, 0.0]
        for sg in range(2):
            for p in range(6):
                v = mtv(R, p6[p])
                v = [v[r] + (-ti[r] if sg == 0 else ti[r]) for r in range(3)]
                n = norm3(v)
                v = [div(v[r], n) for r in range(3)]
                err[sg] = err[sg] + (1.0 - dot3(v, f6[p]))
        tout = [(-ti[r] if err[0] < err[1] else ti[r]) for r in range(3)]
        Rout = [R[3 * c + r] for r in range(3) for c in range(3)]
    return rot2rodrigues(Rout) + tout


def compute_pose(idx, f, p, rs, fold):
    """step 5 on the correspondences idx (ascending indices into f, p [..][3] doubles and rs [..] = (r, s)) -> (Rt [12] doubles, planar)"""
    S6 = rule_sum(idx, fold, lambda c: [p[c][0] * p[c][0], p[c][0] * p[c][1], p[c][0] * p[c][2], p[c][1] * p[c][1], p[c][1] * p[c][2], p[c][2] * p[c][2]], 6)
    planar = rank3(S6) == 2
    E = eigen_rot(S6) if planar else [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    cols = 9 if planar else 12
    upper = [(i, j) for i in range(cols) for j in range(i, cols)]

    def ata_terms(c):
        q = mv(E, p[c]) if planar else p[c]
        a, b = design_rows(rs[c][0], rs[c][1], q, planar)
        return [a[i] * a[j] + b[i] * b[j] for i, j in upper]
    sums = rule_sum(idx, fold, ata_terms, len(upper))
    AtA = [0.0] * (cols * cols)
    for (i, j), v in zip(upper, sums):
        AtA[i * cols + j] = AtA[j * cols + i] = v
    first = list(idx[:6])
    x = linear(AtA, cols, planar, E, [f[c] for c in first], [p[c] for c in first])
    for _ in range(GN_ROUNDS):
        g = gn_begin(x)

        def terms(c):
            res, J = gn_rows(g, p[c], rs[c][0], rs[c][1])
            return gn_terms(J, res)
        sums = rule_sum(idx, fold, terms, 27)
        dx, ends = gn_solve(sums)
        if ends:
            break
        big, worst = 0, 0.0
        for c in idx:
            _, J = gn_rows(g, p[c], rs[c][0], rs[c][1])
            n, _ = gn_not_below(J, dx)
            big += n
            for a in range(2):
                j = J[6 * a:6 * a + 6]
                d = abs(((((j[0] * dx[0] + j[1] * dx[1]) + j[2] * dx[2]) + j[3] * dx[3]) + j[4] * dx[4]) + j[5] * dx[5])
                worst = d if (d > worst or d != d) else worst
        _note("gn748", worst, GN_EPS)
        x = [x[k] - dx[k] for k in range(6)]
        if big == 0:
            break
    R = rodrigues2rot(x[:3])
    return [R[0], R[1], R[2], x[3], R[3], R[4], R[5], x[4], R[6], R[7], R[8], x[5]], int(planar)


# ---- step 6 ------------------------------------------------------------------------------------------------------------------------------------
def check(Rt, cam, X, xy, max_err):
    """-> (error2 as float32, inlier)"""
    with np.errstate(all="ignore"):
        fx, fy, cx, cy = [F(v) for v in cam]
        Xd = [float(F(v)) for v in X]
        xc = F(((Rt[0] * Xd[0] + Rt[1] * Xd[1]) + Rt[2] * Xd[2]) + Rt[3])
        yc = F(((Rt[4] * Xd[0] + Rt[5] * Xd[1]) + Rt[6] * Xd[2]) + Rt[7])
        zc = F(((Rt[8] * Xd[0] + Rt[9] * Xd[1]) + Rt[10] * Xd[2]) + Rt[11])
        u, v = fx * xc / zc + cx, fy * yc / zc + cy
        dx, dy = F(xy[0]) - u, F(xy[1]) - v
        e = dx * dx + dy * dy
        _note("inlier", e, max_err)
        return e, int(e < F(max_err))


# ---- the whole rule for one problem ------------------------------------------------------------------------------------------------------------
def rule(xy_un, assigned, points, cam, tables, draws, rand_max, max_err=5.991, chunk=5, start_iter=0, point_valid=None, min_matches=0, n_matches=None, cache=None):
    """-> dict(header [16], Tcw [12] or None, inliers [n] or None, assigned_out [n] or None, counts, refined) for one problem.
    cache: a dict a caller keeps between calls on the SAME scene (a resumed call fits and refines nothing twice)"""
    xy_un, assigned, points = np.asarray(xy_un, F).reshape(-1, 2), np.asarray(assigned, np.int64), np.asarray(points, F).reshape(-1, 3)
    n, nq, max_iters = len(assigned), len(points), len(draws)
    cm, f, p, rs, xy = [], [], [], [], []
    for i in range(n):
        q = int(assigned[i])
        if q < 0 or q >= nq or (point_valid is not None and not point_valid[q]):
            continue
        cm.append(i)
        p.append([float(v) for v in points[q]])
        xy.append(xy_un[i])
        f.append(bearing(cam, xy_un[i][0], xy_un[i][1]))
        rs.append(nullspace(f[-1]))
    N = len(cm)
    min_eff = max(int(tables[1][N]), MIN_SET)
    header = np.zeros(16, np.int32)
    if N < min_eff or N < MIN_SET or (n_matches is not None and n_matches < min_matches):
        header[0], header[4], header[6] = N, -1, -1
        return dict(header=header, Tcw=None, inliers=None, assigned_out=np.full(n, -1, np.int32), counts=[], refined={})
    its = min(max(int(tables[0][N]), 1), max_iters)
    k0 = max(int(start_iter), 0)
    end = min(max(its, min(k0, max_iters) + min(chunk, max_iters)), max_iters)
    cache = {} if cache is None else cache
    fits, refined, consulted = cache.setdefault("fits", {}), cache.setdefault("refined", {}), set()
    for k in range(end):
        if k in fits:
            continue
        st = make_set(draws[k], rand_max, N)
        Rt, planar = compute_pose(list(range(6)), [f[c] for c in st], [p[c] for c in st], [rs[c] for c in st], False)
        fits[k] = (Rt, planar, sum(check(Rt, cam, p[c], xy[c], max_err)[1] for c in range(N)))
    hyps, counts = [fits[k][:2] for k in range(end)], [fits[k][2] for k in range(end)]
    best_count, best_it, winner = 0, -1, -1
    for k in range(end):
        if counts[k] < min_eff:
            continue
        if counts[k] > best_count:
            best_count, best_it = counts[k], k
        if k < k0:
            continue
        if best_it not in refined:
            flags = [check(hyps[best_it][0], cam, p[c], xy[c], max_err)[1] for c in range(N)]
            Rr, pl = compute_pose([c for c in range(N) if flags[c]], f, p, rs, True)
            rflags = [check(Rr, cam, p[c], xy[c], max_err)[1] for c in range(N)]
            refined[best_it] = (Rr, pl, rflags)
        consulted.add(best_it)
        if sum(refined[best_it][2]) > min_eff:
            winner = k
            break
    status, rep, consumed, ninl = NONE, None, end, 0
    if winner >= 0:
        Rr, pl, rflags = refined[best_it]
        status, rep, consumed, ninl = REFINED, (Rr, pl, rflags), winner + 1, sum(rflags)
    elif best_it >= 0:
        Rt, pl = hyps[best_it]
        status, rep, ninl = BEST, (Rt, pl, [check(Rt, cam, p[c], xy[c], max_err)[1] for c in range(N)]), best_count
    header[:11] = [N, status, its, min_eff, winner, ninl, best_it, best_count, consumed, len(consulted), rep[1] if rep else 0]
    inl, aout = np.zeros(n, np.uint8), np.full(n, -1, np.int32)
    Tcw = None
    if rep:
        Tcw = np.array(rep[0], np.float64).astype(F)
        for c in range(N):
            if rep[2][c]:
                inl[cm[c]] = 1
                aout[cm[c]] = assigned[cm[c]]
    return dict(header=header, Tcw=Tcw, inliers=inl, assigned_out=aout, counts=counts, refined=refined, hyps=hyps)
