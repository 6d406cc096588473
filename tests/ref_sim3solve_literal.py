"""The literal form of Sim3Solver (src/Sim3Solver.cc) and of the merge in front of it (src/LoopClosing.cc:670-710), restated on its own and NOT by the
rule of ref_sim3solve.py: float32 throughout, the sequential loop -- iterate(20) inside `while(!bConverge && !bNoMore)` with mnBestInliers and
mnIterations carried across the chunks --, LAPACK's float32 general eigen-solver (sgeev behind numpy.linalg.eig) standing in for
Eigen::EigenSolver<Matrix4f>, the quaternion -> atan2 -> angle-axis -> Sophus::SO3f::exp chain, matrix products as numpy's float32 matmul, and the
merge as the loop with a Python set.  tests/test_sim3solve_forms.py holds the rule against it."""
import math

import numpy as np

F = np.float32


def random_int(draw, rand_max, lo, hi):
    d = hi - lo + 1
    v = (float(draw) / (float(rand_max) + 1.0)) * d
    return (min(max(int(v), 0), d - 1) if v == v else 0) + lo


def so3_exp(omega):
    """Sophus::SO3f::exp: the quaternion of half the angle, then Eigen's toRotationMatrix, in float32"""
    with np.errstate(all="ignore"):
        theta_sq = F(omega @ omega)
        theta = F(np.sqrt(theta_sq))
        half = F(0.5) * theta
        if theta_sq < F(1e-5) * F(1e-5):
            t4 = theta_sq * theta_sq
            imag = F(0.5) - F(1.0 / 48.0) * theta_sq + F(1.0 / 3840.0) * t4
            real = F(1) - F(1.0 / 8.0) * theta_sq + F(1.0 / 384.0) * t4
        else:
            imag = F(np.sin(half)) / theta
            real = F(np.cos(half))
        w, x, y, z = real, imag * omega[0], imag * omega[1], imag * omega[2]
        tx, ty, tz = F(2) * x, F(2) * y, F(2) * z
        twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
        return np.array([[F(1) - (tyy + tzz), txy - twz, txz + twy], [txy + twz, F(1) - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, F(1) - (txx + tyy)]], F)


def compute_sim3(P1, P2, fix_scale):
    """P1, P2: 3 x 3 float32 with the points in COLUMNS, as the reference holds them -> (T12 [4][4], T21 [4][4], R, t, s)"""
    with np.errstate(all="ignore"):
        O1, O2 = (P1.sum(1) / F(3)).astype(F), (P2.sum(1) / F(3)).astype(F)
        Pr1, Pr2 = P1 - O1[:, None], P2 - O2[:, None]
        M = Pr2 @ Pr1.T
        N11, N12, N13, N14 = M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]
        N22, N23, N24 = M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]
        N33, N34, N44 = -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1], -M[0, 0] - M[1, 1] + M[2, 2]
        N = np.array([[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]], F)
        if np.isfinite(N).all():
            ev, evec = np.linalg.eig(N)
            ev, evec = ev.real.astype(F), evec.real.astype(F)
            k = int(np.argmax(ev))
            q = evec[:, k]
        else:
            q = np.full(4, np.nan, F)
        vec = q[1:4].copy()
        nrm = F(np.sqrt(vec @ vec))
        ang = math.atan2(float(nrm), float(q[0]))
        vec = F(2.0 * ang) * vec / nrm
        Rm = so3_exp(vec)
        P3 = Rm @ Pr2
        if not fix_scale:
            nom, den = float((Pr1 * P3).sum(dtype=F)), float((P3 * P3).sum(dtype=F))
            s = F(np.float64(nom) / np.float64(den))
        else:
            s = F(1)
        t = O1 - (s * Rm) @ O2
        T12, T21 = np.eye(4, dtype=F), np.eye(4, dtype=F)
        T12[:3, :3], T12[:3, 3] = s * Rm, t
        sRinv = F(1.0 / np.float64(s)) * Rm.T
        T21[:3, :3], T21[:3, 3] = sRinv, -(sRinv @ t)
        return T12, T21, Rm, t, s


def project_all(X, T, cam):
    with np.errstate(all="ignore"):
        Xc = (X @ T[:3, :3].T + T[:3, 3]).astype(F)
        return np.stack([F(cam[0]) * Xc[:, 0] / Xc[:, 2] + F(cam[2]), F(cam[1]) * Xc[:, 1] / Xc[:, 2] + F(cam[3])], 1)


class Sim3Solver:
    def __init__(self, points, point1, matched, T1w, T2w, cam1, cam2, fix_scale, max_err1=9.0, max_err2=9.0):
        points = np.asarray(points, F).reshape(-1, 3)
        M = len(points)
        T1w, T2w = np.asarray(T1w, F).reshape(3, 4), np.asarray(T2w, F).reshape(3, 4)
        self.mN1, self.fix, self.cam1, self.cam2 = len(point1), fix_scale, cam1, cam2
        self.idx1, X1, X2 = [], [], []
        for i1 in range(self.mN1):
            r1, r2 = int(point1[i1]), int(matched[i1])
            if r2 < 0 or r2 >= M or r1 < 0 or r1 >= M:
                continue
            self.idx1.append(i1)
            with np.errstate(all="ignore"):
                X1.append(T1w[:, :3] @ points[r1] + T1w[:, 3]); X2.append(T2w[:, :3] @ points[r2] + T2w[:, 3])
        self.X1, self.X2 = np.array(X1, F).reshape(-1, 3), np.array(X2, F).reshape(-1, 3)
        eye = np.eye(4, dtype=F)
        self.P1im1, self.P2im2 = project_all(self.X1, eye, cam1), project_all(self.X2, eye, cam2)
        self.max1, self.max2 = F(max_err1), F(max_err2)
        self.N = len(self.idx1)
        self.best_inliers, self.iterations_done, self.best = 0, 0, None
        self.errs = []

    def set_ransac_parameters(self, prob, min_inliers, max_its):
        self.min_inliers = min_inliers
        if min_inliers == self.N:
            n = 1
        else:
            try:
                with np.errstate(all="ignore"):
                    eps = float(F(min_inliers) / F(self.N))
                n = math.ceil(math.log(1 - prob) / math.log(1 - math.pow(eps, 3)))
            except (ValueError, ZeroDivisionError, OverflowError):
                n = max_its
        self.max_its = max(1, min(n, max_its))

    def check_inliers(self, T12, T21):
        with np.errstate(all="ignore"):
            d1 = self.P1im1 - project_all(self.X2, T12, self.cam1)
            d2 = project_all(self.X1, T21, self.cam2) - self.P2im2
            e1, e2 = (d1 * d1).sum(1, dtype=F), (d2 * d2).sum(1, dtype=F)
            self.errs.append(np.stack([e1, e2], 1))
            return (e1 < self.max1) & (e2 < self.max2)

    def iterate(self, n_iterations, draws, rand_max):
        """-> (T12 or None, bNoMore, vbInliers [mN1], nInliers, bConverge); draws: the stream, consumed three per iteration"""
        inliers = np.zeros(self.mN1, bool)
        if self.N < self.min_inliers or self.N < 3:                         # (fewer than three: the reference's set generation is undefined)
            return None, True, inliers, 0, False
        cur = 0
        while self.iterations_done < self.max_its and cur < n_iterations:
            cur += 1
            avail = list(range(self.N))
            P1, P2 = np.zeros((3, 3), F), np.zeros((3, 3), F)
            for i in range(3):
                randi = random_int(int(draws[3 * self.iterations_done + i]), rand_max, 0, len(avail) - 1)
                idx = avail[randi]
                P1[:, i], P2[:, i] = self.X1[idx], self.X2[idx]
                avail[randi] = avail[-1]
                avail.pop()
            self.iterations_done += 1
            T12, T21, Rm, t, s = compute_sim3(P1, P2, self.fix)
            flags = self.check_inliers(T12, T21)
            n = int(flags.sum())
            if n >= self.best_inliers:
                self.best_inliers, self.best = n, dict(T12=T12, R=Rm, t=t, s=s, it=self.iterations_done - 1, flags=flags)
                if n > self.min_inliers:
                    inliers[np.array(self.idx1)[flags]] = True
                    return T12, False, inliers, n, True
        return (self.best["T12"] if self.best else None), self.iterations_done >= self.max_its, inliers, 0, False


def solve(points, point1, matched, T1w, T2w, cam1, cam2, draws, rand_max, prob=0.99, min_inliers=15, max_its=300, fix_scale=False, max_err1=9.0, max_err2=9.0,
          chunk=20):
    """LoopClosing.cc:698-710 -> dict(converged, no_more, winner, n_inliers, inliers, best (dict or None), N, iterations, errs)"""
    sv = Sim3Solver(points, point1, matched, T1w, T2w, cam1, cam2, fix_scale, max_err1, max_err2)
    sv.set_ransac_parameters(prob, min_inliers, max_its)
    sv.max_its = min(sv.max_its, len(np.asarray(draws).reshape(-1)) // 3)                    # the draws the caller holds
    draws = np.asarray(draws).reshape(-1)
    converged = no_more = False
    inl, n = np.zeros(sv.mN1, bool), 0
    while not converged and not no_more:
        _, no_more, inl, n, converged = sv.iterate(chunk, draws, rand_max)
    return dict(converged=converged, no_more=no_more, winner=sv.best["it"] if converged else -1, n_inliers=n, inliers=inl, best=sv.best, N=sv.N,
                iterations=sv.iterations_done, errs=sv.errs)


def merge(match12, point2, M):
    """LoopClosing.cc:670-687 with vvpMatchedMPs[j][k] = the map point of covisible j at keypoint match12[j][k]"""
    J, n1 = np.asarray(match12).shape
    n2 = np.asarray(point2).shape[1]
    seen, matched, kf, num = set(), [-1] * n1, [-1] * n1, 0
    for j in range(J):
        for k in range(n1):
            m = int(match12[j][k])
            if m < 0 or m >= n2:
                continue
            p = int(point2[j][m])
            if p < 0 or p >= M:
                continue
            if p not in seen:
                seen.add(p)
                num += 1
                matched[k], kf[k] = p, j
    return np.array(matched, np.int32), np.array(kf, np.int32), num
