"""Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:1532-1779) as g2o's lines read, one by one, in float64 with numpy's own matrix products, sums and
solvers: Sim3 as (Quaterniond r, Vector3d t, double s) with r * v through toRotationMatrix, Sim3::log with numpy's functions and numpy.linalg.solve for
W.lu().solve(t), BaseBinaryEdge::linearizeOplus edge by edge, constructQuadraticForm into the blocks of one dense H, numpy.linalg.solve on the full
symmetric matrix for the step, OptimizationAlgorithmLevenberg::solve.  An independent statement of the same optimisation: nothing of the library's
summation orders, its fold or its LDL^T is in it.  The decisions (rho, lambda, ni, the stops) are tests/ref_local_ba.py's Machine.  No test lives here."""
import numpy as np

import ref_local_ba as RB

F, D = np.float32, np.float64
DELTA = 1e-9


def rot_of(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], D)


def quat_of(R):
    """Eigen's Quaterniond(Matrix3d)"""
    t = np.trace(R)
    q = np.zeros(4, D)
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3], q[j], q[k] = (R[k, j] - R[j, k]) * t, (R[j, i] + R[i, j]) * t, (R[k, i] + R[i, k]) * t
    return q


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz], D)


class Sim3:
    def __init__(self, q, t, s):
        self.q, self.t, self.s = np.asarray(q, D), np.asarray(t, D), float(s)

    def __mul__(self, o):
        return Sim3(qmul(self.q, o.q), self.s * (rot_of(self.q) @ o.t) + self.t, self.s * o.s)

    def inverse(self):
        qc = self.q * np.array([-1, -1, -1, 1.0])
        return Sim3(qc, rot_of(qc) @ ((-1.0 / self.s) * self.t), 1.0 / self.s)

    def map(self, X):
        return self.s * (rot_of(self.q) @ X) + self.t

    def vec(self):
        return np.concatenate([self.q, self.t, [self.s]])


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], D)


def sim3_exp(u):
    """Sim3(Vector7d), sim3.h:70-142"""
    omega, upsilon, sigma = u[:3], u[3:6], u[6]
    theta = np.sqrt(omega @ omega)
    O = skew(omega)
    O2 = O @ O
    s, eps, I = np.exp(sigma), 0.00001, np.eye(3)
    if abs(sigma) < eps:
        C = 1.0
        if theta < eps:
            A, B, R = 0.5, 1.0 / 6.0, I + O + O2
        else:
            A, B = (1 - np.cos(theta)) / theta ** 2, (theta - np.sin(theta)) / theta ** 3
            R = I + np.sin(theta) / theta * O + (1 - np.cos(theta)) / (theta * theta) * O2
    else:
        C = (s - 1) / sigma
        if theta < eps:
            A, B = ((sigma - 1) * s + 1) / sigma ** 2, ((0.5 * sigma ** 2 - sigma + 1) * s) / sigma ** 3
            R = I + O + O2
        else:
            R = I + np.sin(theta) / theta * O + (1 - np.cos(theta)) / (theta * theta) * O2
            a, b, c = s * np.sin(theta), s * np.cos(theta), theta ** 2 + sigma ** 2
            A, B = (a * sigma + (1 - b) * theta) / (theta * c), (C - ((b - 1) * sigma + a * theta) / c) / theta ** 2
    return Sim3(quat_of(R), (A * O + B * O2 + C * I) @ upsilon, s)


def sim3_log(S):
    """Sim3::log, sim3.h:148-229"""
    with np.errstate(all="ignore"):
        sigma, R, eps, I = np.log(S.s), rot_of(S.q), 0.00001, np.eye(3)
        d = 0.5 * (np.trace(R) - 1)
        dR = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]], D)
        if d > 1 - eps:
            omega, theta = 0.5 * dR, None
        else:
            theta = np.arccos(d)
            omega = theta / (2 * np.sqrt(1 - d * d)) * dR
        if abs(sigma) < eps:
            C = 1.0
            A, B = (0.5, 1.0 / 6.0) if theta is None else ((1 - np.cos(theta)) / theta ** 2, (theta - np.sin(theta)) / theta ** 3)
        else:
            C = (S.s - 1) / sigma
            if theta is None:
                A, B = ((sigma - 1) * S.s + 1) / sigma ** 2, ((0.5 * sigma ** 2 - sigma + 1) * S.s) / sigma ** 3
            else:
                a, b, c = S.s * np.sin(theta), S.s * np.cos(theta), theta ** 2 + sigma ** 2
                A, B = (a * sigma + (1 - b) * theta) / (theta * c), (C - ((b - 1) * sigma + a * theta) / c) / theta ** 2
        O = skew(omega)
        W = A * O + B * (O @ O) + C * I
        try:
            ups = np.linalg.solve(W, S.t) if np.isfinite(W).all() else np.full(3, np.nan)
        except np.linalg.LinAlgError:
            ups = np.full(3, np.nan)
        return np.concatenate([omega, ups, [sigma]])


def oplus(u, est, fix_scale):
    u = np.array(u, D)
    if fix_scale:
        u[6] = 0.0
    return sim3_exp(u) * est


def error(C, v1, v2):
    return sim3_log(C * v1 * v2.inverse())


def numeric_jacobian(C, v1, v2, which, fix_scale):
    J = np.zeros((7, 7), D)
    for d in range(7):
        add = np.zeros(7, D)
        add[d] = DELTA
        ep = error(C, oplus(add, v1, fix_scale), v2) if which == 0 else error(C, v1, oplus(add, v2, fix_scale))
        add[d] = -DELTA
        em = error(C, oplus(add, v1, fix_scale), v2) if which == 0 else error(C, v1, oplus(add, v2, fix_scale))
        J[:, d] = (1.0 / (2 * DELTA)) * (ep - em)
    return J


def literal(p, n_free=None):
    T, X = np.asarray(p["pose_table"], F).reshape(-1, 12), np.asarray(p["point_table"], F).reshape(-1, 3)
    row, fixed = np.asarray(p["kf_row"], np.int64), np.asarray(p["kf_fixed"], np.uint8) != 0
    sim3 = np.asarray(p["sim3"], D).reshape(-1, 8)
    ci, ni = np.asarray(p["corrected_index"], np.int64), np.asarray(p["noncorrected_index"], np.int64)
    nV, fix_scale, max_it = len(row), int(p.get("fix_scale", 0)), int(p.get("max_iterations", 20))
    row_ok = (row >= 0) & (row < len(T))
    entry = lambda k: Sim3(sim3[k, :4], sim3[k, 4:7], sim3[k, 7])
    vScw, Smw = [], []
    for v in range(nV):
        if 0 <= ci[v] < len(sim3):
            S = entry(ci[v])
        elif row_ok[v]:
            M = T[row[v]].astype(D).reshape(3, 4)
            S = Sim3(quat_of(M[:, :3]), M[:, 3], 1.0)
        else:
            S = Sim3([0, 0, 0, 1], [0, 0, 0], 1.0)
        vScw.append(S)
        Smw.append(entry(ni[v]) if 0 <= ni[v] < len(sim3) else S)
    ei, ej, kind = (np.asarray(p[k], np.int64) for k in ("edge_i", "edge_j", "edge_kind"))
    edges = [e for e in range(len(ei)) if 0 <= ei[e] < nV and 0 <= ej[e] < nV and ei[e] != ej[e] and row_ok[ei[e]] and row_ok[ej[e]]]
    meas = {e: (vScw if kind[e] == 0 else Smw)[ej[e]] * (vScw if kind[e] == 0 else Smw)[ei[e]].inverse() for e in edges}
    free = [v for v in range(nV) if not fixed[v]]
    idx = {v: f for f, v in enumerate(free)}
    nf = len(free)
    n_free = nf if n_free is None else n_free
    status = 2 if nf != n_free else 1 if nf == 0 else 3 if not edges else 0
    est, last = list(vScw), {e: 0.0 for e in edges}
    M = RB.Machine(max_it)
    M.act = "build" if status == 0 else "done"
    n = 7 * nf
    x, H, b = np.zeros(n, D), np.zeros((n, n), D), np.zeros(n, D)

    def active_errors(E):
        chi = 0.0
        with np.errstate(all="ignore"):
            for e in edges:
                er = error(meas[e], E[ei[e]], E[ej[e]])
                last[e] = float(er @ er)
                chi += last[e]
        return chi

    with np.errstate(all="ignore"):
        for _ in range(max_it * 11):
            if M.act == "done":
                break
            if M.act == "build":
                chi = active_errors(est)
                H[:], b[:] = 0.0, 0.0
                for e in edges:
                    i, j = int(ei[e]), int(ej[e])
                    er = error(meas[e], est[i], est[j])
                    Ji = numeric_jacobian(meas[e], est[i], est[j], 0, fix_scale) if i in idx else None
                    Jj = numeric_jacobian(meas[e], est[i], est[j], 1, fix_scale) if j in idx else None
                    for J, v in ((Ji, i), (Jj, j)):
                        if J is not None:
                            f = idx[v]
                            H[7 * f:7 * f + 7, 7 * f:7 * f + 7] += J.T @ J
                            b[7 * f:7 * f + 7] += J.T @ (-er)
                    if Ji is not None and Jj is not None:
                        fi, fj = idx[i], idx[j]
                        H[7 * fi:7 * fi + 7, 7 * fj:7 * fj + 7] += Ji.T @ Jj
                        H[7 * fj:7 * fj + 7, 7 * fi:7 * fi + 7] += Jj.T @ Ji
                M.after_build(chi, 1e-16)
                continue
            A = H + M.lam * np.eye(n)
            ok = bool(np.isfinite(A).all())
            if ok:
                try:
                    np.linalg.cholesky(A)
                    x = np.linalg.solve(A, b)
                except np.linalg.LinAlgError:
                    ok = False
            M.solved = 1 if ok else 0
            trial = list(est)
            for v, f in idx.items():
                trial[v] = oplus(x[7 * f:7 * f + 7], est[v], fix_scale)
            chi = active_errors(trial)
            if M.after_trial(chi, float(np.sum(x * (M.lam * x + b)))):
                est = trial
    Sim3_out = np.stack([S.vec() for S in est])
    Tcw_out = np.zeros((nV, 12), F)
    for v, S in enumerate(est):
        Tcw_out[v] = np.hstack([rot_of(S.q / np.sqrt(S.q @ S.q)), (S.t / S.s)[:, None]]).reshape(12).astype(F)
    prow, pref = np.asarray(p["point_row"], np.int64), np.asarray(p["point_ref"], np.int64)
    points_out, n_points = np.zeros((len(prow), 3), F), 0
    for q in range(len(prow)):
        if not 0 <= prow[q] < len(X):
            continue
        points_out[q] = X[prow[q]]
        if 0 <= pref[q] < nV:
            points_out[q] = est[pref[q]].inverse().map(vScw[pref[q]].map(X[prow[q]].astype(D))).astype(F)
            n_points += 1
    chi2 = np.zeros(len(ei), F)
    if M.iterations > 0:
        with np.errstate(all="ignore"):
            for e in edges:
                chi2[e] = F(last[e])
    header = np.array([status, nf, len(edges), sum(1 for e in edges if kind[e] == 0), M.iterations, M.trials, M.rejected, M.failures, n_points], np.int32)
    return dict(Sim3_out=Sim3_out, Tcw_out=Tcw_out, points_out=points_out, chi2=chi2, header=header, final_chi2=float(M.currentChi))
