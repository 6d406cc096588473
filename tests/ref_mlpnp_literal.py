"""The SEQUENTIAL form of MLPnPsolver's RANSAC loop (src/MLPnPsolver.cpp:100-260) with the members that live across iterate() calls, as the reference
keeps them: mnIterations, mnBestInliers, the best iteration (whose flags are mvbBestInliers).  What an iteration computes is handed in as two
functions -- the inlier count of iteration k and the inlier count of Refine() on the flags of a best iteration -- so that the order-free decision and
the stateless resume of tests/ref_mlpnp.py can be held against the loop as written, whatever fills it.  SetRansacParameters is restated too, with the
C library's own float and libm calls (math), independent of the numpy form of the rule.  Below them the numeric core as the reference writes it, with
LAPACK standing in for Eigen (numpy's SVD for every JacobiSVD, the 1 x 3 null space included, eigh for the self-adjoint solver, a pivoted LDL^T,
pow(x, 1 / 3), the general 4 x 4 inverse) and a Jacobian derived on its own, and MLPnPsolver, the whole solver object; tests/test_mlpnp_forms.py
holds the rule against it."""
import math

import numpy as np

F = np.float32


def set_ransac_parameters(N, probability=0.99, minInliers=10, maxIterations=300, minSet=6, epsilon=0.5):
    """:225-255 -> (mRansacMaxIts, mRansacMinInliers); mRansacMaxIts is None where the reference converts a NaN to int"""
    mRansacEpsilon = F(epsilon)
    nMinInliers = int(F(N) * mRansacEpsilon)
    if nMinInliers < minInliers:
        nMinInliers = minInliers
    if nMinInliers < minSet:
        nMinInliers = minSet
    mRansacMinInliers = nMinInliers
    if N > 0 and mRansacEpsilon < F(mRansacMinInliers) / F(N):
        mRansacEpsilon = F(mRansacMinInliers) / F(N)
    if mRansacMinInliers == N:
        nIterations = 1
    else:
        x = 1.0 - math.pow(float(mRansacEpsilon), 3.0)
        nIterations = math.ceil(math.log(1.0 - probability) / math.log(x)) if 0.0 < x < 1.0 else (0 if x == 0.0 else None)
    if nIterations is None:                                                      # log of a negative number: the reference's int cast is undefined there
        return None, mRansacMinInliers
    return max(1, min(nIterations, maxIterations)), mRansacMinInliers


class Solver:
    def __init__(self, N, max_its, min_inliers, count_of, refine_of, max_iters):
        self.N, self.mRansacMaxIts, self.mRansacMinInliers, self.count_of, self.refine_of, self.max_iters = N, max_its, min_inliers, count_of, refine_of, max_iters
        self.mnIterations, self.mnBestInliers, self.best = 0, 0, -1

    def iterate(self, nIterations):
        """-> (returned, bNoMore, nInliers, the iteration it returned at or -1)"""
        if self.N < self.mRansacMinInliers:
            return False, True, 0, -1
        nCurrentIterations = 0
        while self.mnIterations < self.mRansacMaxIts or nCurrentIterations < nIterations:
            if self.mnIterations >= self.max_iters:                              # the caller's draws end here
                break
            nCurrentIterations += 1
            k = self.mnIterations
            self.mnIterations += 1
            mnInliersi = self.count_of(k)
            if mnInliersi >= self.mRansacMinInliers:
                if mnInliersi > self.mnBestInliers:
                    self.mnBestInliers, self.best = mnInliersi, k
                mnRefinedInliers = self.refine_of(self.best)
                if mnRefinedInliers > self.mRansacMinInliers:
                    return True, False, mnRefinedInliers, k
        if self.mnIterations >= self.mRansacMaxIts:
            if self.mnBestInliers >= self.mRansacMinInliers:
                return True, True, self.mnBestInliers, -1
            return False, True, 0, -1
        return False, False, 0, -1


# ---- the numeric core, as the reference writes it, with LAPACK standing in for Eigen -----------------------------------------------------------
D = np.float64


def null_space(f):
    """:371-373: JacobiSVD of the 1 x 3 bearing vector, columns 2 and 3 of V"""
    V = np.linalg.svd(np.asarray(f, D).reshape(1, 3))[2].T
    return V[:, 1].copy(), V[:, 2].copy()


def rodrigues2rot(w):
    w = np.asarray(w, D)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    n = np.linalg.norm(w)
    R = np.eye(3)
    if n > np.finfo(D).eps:
        R = R + math.sin(n) / n * K + (1 - math.cos(n)) / (n * n) * (K @ K)
    return R


def rot2rodrigues(R):
    wn = math.acos(min(1.0, max(-1.0, (np.trace(R) - 1.0) / 2.0))) if np.isfinite(np.trace(R)) else float("nan")
    if not wn > np.finfo(D).eps:
        return np.zeros(3)
    return np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * (wn / (2.0 * math.sin(wn)))


def ldlt_solve(A, g):
    """a pivoted LDL^T (the largest remaining diagonal entry is the pivot, as Eigen::LDLT chooses it)"""
    n = len(g)
    A, perm = np.array(A, D), list(range(n))
    L, d = np.eye(n), np.zeros(n)
    for k in range(n):
        j = k + int(np.argmax(np.abs(np.diag(A)[k:])))
        if j != k:
            A[[k, j], :] = A[[j, k], :]; A[:, [k, j]] = A[:, [j, k]]
            L[[k, j], :k] = L[[j, k], :k]
            perm[k], perm[j] = perm[j], perm[k]
        d[k] = A[k, k]
        if d[k] != 0.0:
            L[k + 1:, k] = A[k + 1:, k] / d[k]
            A[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], A[k, k + 1:])
    b = np.asarray(g, D)[perm]
    y = np.linalg.solve(L, b)
    with np.errstate(all="ignore"):
        z = np.linalg.solve(L.T, y / d)
    x = np.zeros(n)
    x[perm] = z
    return x


def d_rotated_point(w, X):
    """d (R(w) X) / d w, 3 x 3, from the derivative of R = I + a K + b K^2 entry by entry (a = sin t / t, b = (1 - cos t) / t^2)"""
    t = np.linalg.norm(w)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    a, b = math.sin(t) / t, (1 - math.cos(t)) / (t * t)
    da, db = (t * math.cos(t) - math.sin(t)) / (t * t), (t * math.sin(t) - 2 * (1 - math.cos(t))) / (t ** 3)
    out = np.zeros((3, 3))
    for i in range(3):
        Ki = np.zeros((3, 3))
        e = np.zeros(3); e[i] = 1.0
        Ki = np.array([[0.0, -e[2], e[1]], [e[2], 0.0, -e[0]], [-e[1], e[0], 0.0]])
        dR = da * (w[i] / t) * K + a * Ki + db * (w[i] / t) * (K @ K) + b * (Ki @ K + K @ Ki)
        out[:, i] = dR @ X
    return out


def residuals_and_jacs(x, pts, ns):
    """:760-806 with the derivative written out by hand (the reference's is machine generated)"""
    w, T = x[:3], x[3:]
    R = rodrigues2rot(w)
    r, J = np.zeros(2 * len(pts)), np.zeros((2 * len(pts), 6))
    for i, X in enumerate(pts):
        v = R @ X + T
        nv = np.linalg.norm(v)
        u = v / nv
        dv = np.concatenate([d_rotated_point(w, X), np.eye(3)], 1)           # d v / d (w, T)
        du = (np.eye(3) - np.outer(u, u)) / nv @ dv
        for a in range(2):
            r[2 * i + a] = ns[i][a] @ u
            J[2 * i + a] = ns[i][a] @ du
    return r, J


def mlpnp_gn(x, pts, ns):
    """:694-758"""
    x = np.array(x, D)
    it_cnt, stop = 0, False
    while it_cnt < 5 and not stop:
        r, Jac = residuals_and_jacs(x, pts, ns)
        with np.errstate(all="ignore"):
            dx = ldlt_solve(Jac.T @ Jac, Jac.T @ r)
        if np.abs(dx).max() > 5.0 or np.abs(dx).min() > 1.0:
            break
        dl = Jac @ dx
        if np.abs(dl).max() < 1e-5:
            stop = True
            x = x - dx
            break
        x = x - dx
        it_cnt += 1
    return x


def compute_pose(f, p):
    """:356-658 on bearing vectors f [m][3] and points p [m][3] (doubles) -> (R [3][3], t [3], planar, relative gap of the two least eigenvalues of A^T A)"""
    f, p = np.asarray(f, D), np.asarray(p, D)
    m = len(f)
    ns = [null_space(f[i]) for i in range(m)]
    points3 = p.T.copy()
    planarTest = points3 @ points3.T
    eigenRot = np.eye(3)
    planar = np.linalg.matrix_rank(planarTest, tol=3 * np.finfo(D).eps * np.linalg.norm(planarTest, 2)) == 2          # FullPivHouseholderQR's rank with its default threshold
    if planar:
        eigenRot = np.linalg.eigh(planarTest)[1].T
        points3 = eigenRot @ points3
    cols = 9 if planar else 12
    A = np.zeros((2 * m, cols))
    for i in range(m):
        q = points3[:, i]
        for a in range(2):
            n = ns[i][a]
            A[2 * i + a] = ([n[0] * q[1], n[0] * q[2], n[1] * q[1], n[1] * q[2], n[2] * q[1], n[2] * q[2], n[0], n[1], n[2]] if planar else
                            [n[0] * q[0], n[0] * q[1], n[0] * q[2], n[1] * q[0], n[1] * q[1], n[1] * q[2], n[2] * q[0], n[2] * q[1], n[2] * q[2], n[0], n[1], n[2]])
    _, sv, Vt = np.linalg.svd(A.T @ A)
    res = Vt[-1]
    gap = abs(sv[-2] - sv[-1]) / sv[-2] if sv[-2] > 0 else 0.0
    with np.errstate(all="ignore"):
        if planar:
            tmp = np.array([[0.0, res[0], res[1]], [0.0, res[2], res[3]], [0.0, res[4], res[5]]])
            tmp[:, 0] = np.cross(tmp[:, 1], tmp[:, 2])
            tmp = tmp.T.copy()
            scale = 1.0 / math.sqrt(abs(np.linalg.norm(tmp[:, 1]) * np.linalg.norm(tmp[:, 2])))
            U, _, Wt = np.linalg.svd(tmp)
            Rout1 = U @ Wt
            if np.linalg.det(Rout1) < 0:
                Rout1 = Rout1 * -1.0
            Rout1 = eigenRot.T @ Rout1
            t = scale * res[6:9]
            Rout1 = Rout1.T * -1.0
            if np.linalg.det(Rout1) < 0:
                Rout1[:, 2] *= -1.0
            R2 = Rout1.copy(); R2[:, :2] *= -1.0
            Ts = [(Rout1, t), (Rout1, -t), (R2, t), (R2, -t)]
            normVal = []
            for Rc, tc in Ts:
                norms = 0.0
                for k in range(6):
                    v = Rc @ p[k] + tc
                    norms += 1.0 - (v / np.linalg.norm(v)) @ f[k]
                normVal.append(norms)
            Rout, tout = Ts[int(np.argmin(normVal))]
        else:
            tmp = np.array([[res[0], res[3], res[6]], [res[1], res[4], res[7]], [res[2], res[5], res[8]]])
            scale = 1.0 / math.pow(abs(np.linalg.norm(tmp[:, 0]) * np.linalg.norm(tmp[:, 1]) * np.linalg.norm(tmp[:, 2])), 1.0 / 3.0)
            U, _, Wt = np.linalg.svd(tmp)
            Rout = U @ Wt
            if np.linalg.det(Rout) < 0:
                Rout = Rout * -1.0
            tout = Rout @ (scale * res[9:12])
            error, Ts = [0.0, 0.0], []
            for s in range(2):
                T4 = np.eye(4)
                T4[:3, :3] = Rout
                T4[:3, 3] = tout if s == 0 else -tout
                T4 = np.linalg.inv(T4)
                Ts.append(T4)
                for k in range(6):
                    v = T4[:3, :3] @ p[k] + T4[:3, 3]
                    error[s] += 1.0 - (v / np.linalg.norm(v)) @ f[k]
            tout = Ts[0][:3, 3] if error[0] < error[1] else Ts[1][:3, 3]
            Rout = Ts[0][:3, :3]
        x = mlpnp_gn(np.concatenate([rot2rodrigues(Rout), tout]), p, ns)
    return rodrigues2rot(x[:3]), x[3:].copy(), bool(planar), float(gap)


class MLPnPsolver:
    """The solver object as the reference keeps it (constructor :55-97, iterate :100-223, CheckInliers :262-293, Refine :295-353), one iterate() per
    call, the members alive in between.  store_refined = False is the reference AS WRITTEN: Refine() calls computePose(.., result) and then
    CheckInliers(), but never copies `result` into mRi / mti, so what it counts and reports is the pose of the iteration that called it.
    store_refined = True is the same code with that one copy added, which is what the rule of xfh_mlpnp_solve_device states."""

    def __init__(self, xy_un, assigned, points, valid, cam, draws, rand_max, max_err, store_refined, eps=0.5, min_inliers=10, max_its=300):
        self.cam = [F(c) for c in cam]
        self.kp, self.P2D, self.f, self.P3D = [], [], [], []
        for i, q in enumerate(np.asarray(assigned, np.int64)):
            if q < 0 or q >= len(points) or (valid is not None and not valid[q]):
                continue
            x, y = F(xy_un[i][0]), F(xy_un[i][1])
            self.kp.append(i); self.P2D.append((x, y)); self.P3D.append(np.asarray(points[q], F))
            self.f.append(np.array([(x - self.cam[2]) / self.cam[0], (y - self.cam[3]) / self.cam[1], F(1.0)], D))
        self.n, self.N = len(assigned), len(self.kp)
        pr = set_ransac_parameters(self.N, 0.99, min_inliers, max_its, 6, eps)
        self.mRansacMaxIts, self.mRansacMinInliers = min(max_its if pr[0] is None else pr[0], len(draws)), pr[1]        # (the rule's clamp: the draws hold no more)
        self.draws, self.rand_max, self.max_err, self.store = np.asarray(draws), rand_max, F(max_err), store_refined
        self.mnIterations, self.mnBestInliers, self.mvbBestInliers = 0, 0, []
        self.mRi, self.mti, self.mvbInliersi, self.mnInliersi, self.gaps = np.eye(3), np.zeros(3), [], 0, {}

    def CheckInliers(self):
        with np.errstate(all="ignore"):
            fx, fy, cx, cy = self.cam
            self.mvbInliersi = []
            for i in range(self.N):
                X = self.P3D[i].astype(D)
                c = [F(self.mRi[r, 0] * X[0] + self.mRi[r, 1] * X[1] + self.mRi[r, 2] * X[2] + self.mti[r]) for r in range(3)]
                u, v = fx * c[0] / c[2] + cx, fy * c[1] / c[2] + cy
                dx, dy = self.P2D[i][0] - u, self.P2D[i][1] - v
                self.mvbInliersi.append(bool(dx * dx + dy * dy < self.max_err))
            self.mnInliersi = sum(self.mvbInliersi)

    def Tcw(self):
        return np.concatenate([self.mRi, self.mti[:, None]], 1).astype(F).ravel()

    def Refine(self):
        idx = [i for i in range(self.N) if self.mvbBestInliers[i]]
        R, t, planar, gap = compute_pose([self.f[i] for i in idx], [self.P3D[i].astype(D) for i in idx])
        if self.store:
            self.mRi, self.mti = R, t
        self.CheckInliers()
        self.mnRefinedInliers, self.mvbRefinedInliers = self.mnInliersi, list(self.mvbInliersi)
        self.refined_gap = gap
        if self.mnInliersi > self.mRansacMinInliers:
            self.mRefinedTcw = self.Tcw()
            return True
        return False

    def flags(self, vb):
        out = np.zeros(self.n, np.uint8)
        for i in range(self.N):
            if vb[i]:
                out[self.kp[i]] = 1
        return out

    def iterate(self, nIterations):
        """-> dict(ret, bNoMore, nInliers, vbInliers [n], Tcw [12] float32 or None, at, gap)"""
        none = dict(ret=False, bNoMore=True, nInliers=0, vbInliers=np.zeros(self.n, np.uint8), Tcw=None, at=-1, gap=0.0)
        if self.N < self.mRansacMinInliers or self.N < 6:
            return none
        nCurrentIterations = 0
        while self.mnIterations < self.mRansacMaxIts or nCurrentIterations < nIterations:
            if self.mnIterations >= len(self.draws):                             # the caller's draws end here
                break
            nCurrentIterations += 1
            k = self.mnIterations
            self.mnIterations += 1
            avail, st = list(range(self.N)), []
            for j in range(6):
                v = (float(self.draws[k][j]) / (float(self.rand_max) + 1.0)) * len(avail)
                r = 0 if not v >= 0.0 else (len(avail) - 1 if v >= len(avail) else int(v))
                st.append(avail[r])
                avail[r] = avail[-1]
                avail.pop()
            self.mRi, self.mti, _, gap = compute_pose([self.f[i] for i in st], [self.P3D[i].astype(D) for i in st])
            self.gaps[k] = gap
            self.CheckInliers()
            if self.mnInliersi >= self.mRansacMinInliers:
                if self.mnInliersi > self.mnBestInliers:
                    self.mvbBestInliers, self.mnBestInliers, self.mBestTcw, self.best = list(self.mvbInliersi), self.mnInliersi, self.Tcw(), k
                if self.Refine():
                    return dict(ret=True, bNoMore=False, nInliers=self.mnRefinedInliers, vbInliers=self.flags(self.mvbRefinedInliers), Tcw=self.mRefinedTcw, at=k,
                                gap=self.refined_gap if self.store else gap)
        if self.mnIterations >= self.mRansacMaxIts and self.mnBestInliers >= self.mRansacMinInliers:
            return dict(ret=True, bNoMore=True, nInliers=self.mnBestInliers, vbInliers=self.flags(self.mvbBestInliers), Tcw=self.mBestTcw, at=-1, gap=self.gaps[self.best])
        return none
