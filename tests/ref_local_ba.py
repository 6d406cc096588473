"""The rule of xfh_local_ba_device (include/xfeat_hip.h, "LocalBundleAdjustment") restated in numpy float64: Optimizer::LocalBundleAdjustment from the
graph to vToErase (src/Optimizer.cc:1188-1460), optimize(10) of OptimizationAlgorithmLevenberg over BlockSolver_6_3 with the Schur complement.

  rule(problem)                    the kernels' own organisation: the lines of xfeatslam_amd/csrc/lba_math.h operation by operation and every sum in the
                                   order the header states (a point's sums in edge order; the 256-lane fold per keyframe, per block of S, for the chi2
                                   of the graph and for computeScale; the right-looking LDL^T).  The host form equals it by bits.
  rule(problem, libm_jitter=seed)  the rule with every sqrt / sin / cos result moved by up to one double ulp: the device's libm is not the host's.

The per-edge pose arithmetic is tests/ref_poseopt.py's (the lines of poseopt_math.h).  A problem is a dict: pose_table (R, 12) and point_table (M, 3)
float32, kf_row, kf_fixed, point_row, edge_begin (a proper CSR), edge_kf, edge_obs (nE, 3), cam (fx, fy, cx, cy, bf), inv_sigma2, max_iterations.
Every decision records how far it was from its decision point (`margins`), which is what the rig's condition is."""
import math

import numpy as np

import ref_poseopt as RP

D, F = np.float64, np.float32
DBL_MAX = RP.DBL_MAX
TH_MONO, TH_STEREO = 5.991, 7.815
OK, ABORTED, NOTHING_FREE, FREE_MISMATCH = 0, 1, 2, 3
H_KEYS = ("status", "free", "fixed_with_edge", "mono", "stereo", "iterations", "trials", "rejected", "ldlt_failures", "erase")
MAX_FREE = 128


# ---- the binary edge -------------------------------------------------------------------------------------------------------------------------------
def point_jacobian(cam, R, pc, stereo):
    """-> 9 arrays, the 3x3 point Jacobian row-major (third row zero for mono); R: the 9 entries of the pose's rotation matrix"""
    fx, fy, cx, cy, bf = cam
    x, y, z = pc
    with np.errstate(all="ignore"):
        a, c, b, d = fx / z, -fx * x / (z * z), fy / z, -fy * y / (z * z)
        zero = np.zeros_like(np.asarray(x, D))
        M = [-(a * R[k] + c * R[6 + k]) for k in range(3)] + [-(b * R[3 + k] + d * R[6 + k]) for k in range(3)] + [zero] * 3
        z2 = z * z
        S0 = [-fx * R[k] / z + fx * x * R[6 + k] / z2 for k in range(3)]
        S1 = [-fy * R[3 + k] / z + fy * y * R[6 + k] / z2 for k in range(3)]
        S2 = [S0[k] - bf * R[6 + k] / z2 for k in range(3)]
        S = S0 + S1 + S2
        return [np.where(stereo, S[k], M[k]) for k in range(9)]


def linearize(pose, cam, X, obs, stereo, w):
    """n edges at one pose -> e [3], chi2, rho0, rho1, Jp [18], Jl [9] (lists of arrays)"""
    pc, e, chi2 = RP.edge_error(pose, cam, X, obs, stereo, w)
    r0, r1 = RP.huber(chi2, stereo)
    Jp = RP.edge_jacobian(cam, pc, stereo)
    Jl = point_jacobian(cam, RP.matrix_from_quat(pose[:4]), pc, stereo)
    return e, chi2, r0, r1, Jp, Jl


def records(e, chi2, r1, Jp, Jl, stereo, w, free):
    """lba_edge_record: (n, 28)"""
    ww = r1 * w
    out = []
    with np.errstate(all="ignore"):
        for a in range(3):
            for b in range(a, 3):
                c = Jl[a] * (ww * Jl[b]) + Jl[3 + a] * (ww * Jl[3 + b])
                out.append(np.where(stereo, c + Jl[6 + a] * (ww * Jl[6 + b]), c))
        for a in range(3):
            c = Jl[a] * (w * e[0]) + Jl[3 + a] * (w * e[1])
            c = np.where(stereo, c + Jl[6 + a] * (w * e[2]), c)
            out.append(-(r1 * c))
        for i in range(6):
            for a in range(3):
                c = Jp[i] * (ww * Jl[a]) + Jp[6 + i] * (ww * Jl[3 + a])
                c = np.where(stereo, c + Jp[12 + i] * (ww * Jl[6 + a]), c)
                out.append(c if free else np.zeros_like(c))
        out.append(chi2)
    return np.stack([np.asarray(o, D) * np.ones_like(np.asarray(chi2, D)) for o in out], -1)


def point_block(H6, lam):
    """(n, 6) upper triangles -> (n, 9): the cofactor inverse of H + lam I"""
    H6 = np.asarray(H6, D).reshape(-1, 6)
    with np.errstate(all="ignore"):
        m00, m01, m02, m11, m12, m22 = H6[:, 0] + lam, H6[:, 1], H6[:, 2], H6[:, 3] + lam, H6[:, 4], H6[:, 5] + lam
        c00, c10, c20 = m11 * m22 - m12 * m12, m02 * m12 - m01 * m22, m01 * m12 - m02 * m11
        det = (c00 * m00 + c10 * m01) + c20 * m02
        inv = 1.0 / det
        d4, d5, d8 = (m00 * m22 - m02 * m02) * inv, (m01 * m02 - m00 * m12) * inv, (m00 * m11 - m01 * m01) * inv
        return np.stack([c00 * inv, c10 * inv, c20 * inv, c10 * inv, d4, d5, c20 * inv, d5, d8], -1)


def ldlt_factor(S, b, x_old):
    """the right-looking LDL^T on the lower triangle of S (a copy is factorised) -> ok, x, pivots [(d_k, |S_kk| before the updates)], the copy as the
    factorisation left it: L below the diagonal and d on it, down to the column at which it stopped (the copy's upper triangle means nothing)"""
    S = np.array(S, D)
    n = len(b)
    diag0 = np.abs(np.diag(S)).copy()
    piv = []
    with np.errstate(all="ignore"):
        for k in range(n):
            dk = S[k, k]
            piv.append((float(dk), float(diag0[k])))
            if not dk > 0.0:
                return False, np.array(x_old, D), piv, S
            S[k + 1:, k] = S[k + 1:, k] / dk
            col = S[k + 1:, k]
            S[k + 1:, k + 1:] = S[k + 1:, k + 1:] - col[:, None] * col[None, :] * dk
        y = np.array(b, D)
        for k in range(n):
            y[k + 1:] = y[k + 1:] - S[k + 1:, k] * y[k]
        y = y / np.diag(S)
        for k in range(n - 1, -1, -1):
            y[:k] = y[:k] - S[k, :k] * y[k]
    return True, y, piv, S


def ldlt_solve(S, b, x_old):
    """-> ok, x, pivots of ldlt_factor"""
    return ldlt_factor(S, b, x_old)[:3]


def lambda_init(diag):
    m = 0.0
    if not np.isnan(diag).any():
        return 1e-5 * max(m, float(np.max(diag))) if len(diag) else 0.0
    for a in diag.tolist():
        m = m if a < m else a
    return 1e-5 * m


class Machine:
    """the Levenberg decisions of lba_math.h (LbaCtl): after_build / after_trial with the sums handed in"""

    def __init__(self, max_it):
        self.lam, self.ni, self.currentChi, self.iniChi = 0.0, 2.0, 0.0, 0.0
        self.act, self.iter, self.qmax, self.nbad, self.solved, self.cur, self.max_it = "build", 0, 0, 0, 0, 0, max_it
        self.iterations = self.trials = self.rejected = self.failures = 0
        self.margin_rho = self.margin_stop = np.inf

    def after_build(self, chi, lam0):
        self.currentChi = self.iniChi = chi
        if self.iter == 0:
            self.lam, self.ni, self.nbad = lam0, 2.0, 0
        self.qmax = 0
        self.iterations += 1
        self.act = "trial"

    def after_trial(self, chi, scale):
        """-> accepted"""
        self.trials += 1
        self.failures += 0 if self.solved else 1
        tempChi = chi if self.solved else DBL_MAX
        with np.errstate(all="ignore"):
            rho = float(D(self.currentChi - tempChi) / D(scale + 1e-3))
        if rho == rho:
            self.margin_rho = min(self.margin_rho, abs(rho))
        accepted = rho > 0.0 and math.isfinite(tempChi)
        if accepted:
            t = 2.0 * rho - 1.0
            alpha = 1.0 - t * t * t
            alpha = 2.0 / 3.0 if 2.0 / 3.0 < alpha else alpha
            f = alpha if 1.0 / 3.0 < alpha else 1.0 / 3.0
            self.lam *= f
            self.ni = 2.0
            self.currentChi = tempChi
            self.cur = 1 - self.cur
        else:
            self.lam *= self.ni
            self.ni *= 2.0
            self.rejected += 1
        self.qmax += 1
        if rho < 0.0 and self.qmax < 10:
            self.act = "trial"
            return accepted
        if self.qmax == 10 or rho == 0.0:
            self.act = "done"
            return accepted
        ini, cur = self.iniChi, self.currentChi
        if ini == ini and cur == cur and ini != 0.0:
            self.margin_stop = min(self.margin_stop, abs((ini - cur) * 1e3 - ini) / abs(ini))
        if (ini - cur) * 1e3 < ini:
            self.nbad += 1
        else:
            self.nbad = 0
        if self.nbad >= 3:
            self.act = "done"
            return accepted
        self.iter += 1
        self.act = "build" if self.iter < self.max_it else "done"
        return accepted

    def fields(self):
        return dict(lam=self.lam, ni=self.ni, currentChi=self.currentChi, iniChi=self.iniChi, act=self.act, iter=self.iter, qmax=self.qmax, nbad=self.nbad,
                    cur=self.cur, iterations=self.iterations, trials=self.trials, rejected=self.rejected, failures=self.failures)


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------------------
class Plan:
    def __init__(self, p):
        self.cam, self.w = RP.cam_of(p["cam"]), float(F(p["inv_sigma2"]))
        self.kf_row, self.point_row = np.asarray(p["kf_row"], np.int32), np.asarray(p["point_row"], np.int32)
        self.fixed = np.asarray(p["kf_fixed"], np.uint8) != 0
        self.nK, self.nP = len(self.kf_row), len(self.point_row)
        begin = np.asarray(p["edge_begin"], np.int64)
        self.edge_kf = np.asarray(p["edge_kf"], np.int32)
        self.nE = len(self.edge_kf)
        assert begin[0] == 0 and begin[-1] == self.nE and np.all(np.diff(begin) >= 0), "edge_begin is not a CSR"
        assert np.all((self.kf_row >= 0) & (self.kf_row < len(p["pose_table"]))) and np.all((self.point_row >= 0) & (self.point_row < len(p["point_table"])))
        self.begin = begin
        self.obs = np.asarray(p["edge_obs"], F).reshape(-1, 3)
        self.stereo = ~(self.obs[:, 2] < 0)
        self.obs = self.obs.astype(D)
        self.edge_pt = np.repeat(np.arange(self.nP), np.diff(begin)).astype(np.int64)
        self.valid = (self.edge_kf >= 0) & (self.edge_kf < self.nK)
        self.kf_edges = [np.nonzero(self.valid & (self.edge_kf == k))[0] for k in range(self.nK)]
        self.pt_edges = np.bincount(self.edge_pt[self.valid], minlength=self.nP)
        self.free_kf = [k for k in range(self.nK) if not self.fixed[k]]
        self.kf_free = {k: i for i, k in enumerate(self.free_kf)}
        self.fixed_with_edge = sum(1 for k in range(self.nK) if self.fixed[k] and len(self.kf_edges[k]))
        self.mono, self.stereo_n = int(np.sum(self.valid & ~self.stereo)), int(np.sum(self.valid & self.stereo))
        ve = np.nonzero(self.valid)[0]
        self.rank = np.zeros(self.nE, np.int64)                             # the position of a valid edge among its point's valid edges
        seen = np.zeros(self.nP, np.int64)
        for e in ve.tolist():
            self.rank[e] = seen[self.edge_pt[e]]
            seen[self.edge_pt[e]] += 1
        self.by_point_kf = {}
        for e in ve.tolist():
            self.by_point_kf.setdefault((int(self.edge_pt[e]), int(self.edge_kf[e])), []).append(e)


def fold1(v):
    return float(RP.fold(np.asarray(v, D).reshape(-1, 1))[0])


def rule(p, libm_jitter=None, n_free=None):
    RP._JITTER = None if libm_jitter is None else np.random.RandomState(libm_jitter)
    try:
        return _rule(p, n_free)
    finally:
        RP._JITTER = None


def _rule(p, n_free):
    P = Plan(p)
    cam, w, nK, nP, nE = P.cam, P.w, P.nK, P.nP, P.nE
    pose_table, point_table = np.asarray(p["pose_table"], F).reshape(-1, 12), np.asarray(p["point_table"], F).reshape(-1, 3)
    nF = len(P.free_kf)
    hdr = dict.fromkeys(H_KEYS, 0)
    hdr.update(free=nF, fixed_with_edge=P.fixed_with_edge, mono=P.mono, stereo=P.stereo_n)
    status = OK
    if n_free is not None and n_free != nF:
        status = FREE_MISMATCH
    elif P.fixed_with_edge == 0:
        status = ABORTED
    elif nF == 0:
        status = NOTHING_FREE
    hdr["status"] = status
    res = dict(Tcw_out=pose_table[P.kf_row].copy(), points_out=point_table[P.point_row].copy(), erase=np.zeros(nE, np.uint8), chi2=np.zeros(nE, F),
               final_chi2=0.0, events=[], margins=dict(classify=np.inf, depth=np.inf, rho=np.inf, stop=np.inf, pivot=np.inf), lambdas=[])
    if status != OK:
        res["header"] = np.array([hdr[k] for k in H_KEYS], np.int32)
        return res

    poses = [[RP.from_tcw(pose_table[r]) for r in P.kf_row], None]
    poses[1] = [list(q) for q in poses[0]]
    pts = [point_table[P.point_row].astype(D), point_table[P.point_row].astype(D)]
    rec = np.zeros((nE, 28), D)
    kf_sum, kf_chi = np.zeros((nK, 28), D), np.zeros(nK, D)
    Hll, bl, xl, pscale, xp = np.zeros((nP, 6), D), np.zeros((nP, 3), D), np.zeros((nP, 3), D), np.zeros(nP, D), np.zeros(6 * nF, D)
    M = Machine(int(p.get("max_iterations", 10)))
    ve = np.nonzero(P.valid)[0]
    maxdeg = int(P.pt_edges.max()) if nP else 0

    def kf_pass(buf, build):
        for k in range(nK):
            idx = P.kf_edges[k]
            X, ob, st = pts[buf][P.edge_pt[idx]], P.obs[idx], P.stereo[idx]
            if build:
                free = k in P.kf_free
                e, chi2, r0, r1, Jp, Jl = linearize(poses[buf][k], cam, X, ob, st, w)
                rec[idx] = records(e, chi2, r1, Jp, Jl, st, w, free)
                sh = RP.shares(Jp, e, st, w, r1) if free else np.zeros((len(idx), 28), D)
                sh = sh * np.ones((len(idx), 1), D) if sh.ndim == 2 else sh
                sh[:, 27] = r0
                kf_sum[k] = RP.fold(sh)
            else:
                _, _, chi2 = RP.edge_error(poses[buf][k], cam, X, ob, st, w)
                rec[idx, 27] = chi2
                kf_chi[k] = fold1(RP.huber(chi2, st)[0])

    for _ in range(M.max_it * 11):
        if M.act == "done":
            break
        if M.act == "build":
            kf_pass(M.cur, True)
            Hll[:], bl[:] = 0.0, 0.0
            with np.errstate(all="ignore"):
                for d in range(maxdeg):                                     # a point's shares in edge order
                    sel = ve[P.rank[ve] == d]
                    Hll[P.edge_pt[sel]] += rec[sel, :6]
                    bl[P.edge_pt[sel]] += rec[sel, 6:9]
            diag = np.concatenate([np.abs(kf_sum[P.free_kf][:, [0, 6, 11, 15, 18, 20]]).reshape(-1), np.abs(Hll[:, [0, 3, 5]]).reshape(-1)])
            M.after_build(fold1(kf_sum[:, 27]), lambda_init(diag))
            res["events"].append(("build", M.iter))
            continue
        lam = M.lam
        res["lambdas"].append(lam)
        S, bS = np.zeros((6 * nF, 6 * nF), D), np.zeros(6 * nF, D)
        Dall = point_block(Hll, lam)
        with np.errstate(all="ignore"):
            for i in range(nF):
                ei = P.kf_edges[P.free_kf[i]]
                pi = P.edge_pt[ei]
                Wm, Dm = rec[ei, 9:27].reshape(-1, 6, 3), Dall[pi].reshape(-1, 3, 3)
                Y = (Wm[:, :, 0, None] * Dm[:, None, 0, :] + Wm[:, :, 1, None] * Dm[:, None, 1, :]) + Wm[:, :, 2, None] * Dm[:, None, 2, :]
                for j in range(i, nF):
                    kj = P.free_kf[j]
                    terms = np.zeros((len(ei), 42), D)
                    if i == j:
                        b3 = bl[pi]
                        terms[:, 36:] = (Y[:, :, 0] * b3[:, None, 0] + Y[:, :, 1] * b3[:, None, 1]) + Y[:, :, 2] * b3[:, None, 2]
                    mates = [P.by_point_kf.get((int(pp), kj), ()) for pp in pi]
                    assert all(len(m) <= 1 for m in mates), "a keyframe sees a point twice: not a graph the reference builds"
                    has = np.array([len(m) == 1 for m in mates], bool)
                    if has.any():
                        V = rec[[m[0] for m in mates if m], 9:27].reshape(-1, 6, 3)
                        Yh = Y[has]
                        blk = (Yh[:, :, None, 0] * V[:, None, :, 0] + Yh[:, :, None, 1] * V[:, None, :, 1]) + Yh[:, :, None, 2] * V[:, None, :, 2]
                        terms[has, :36] = blk.reshape(-1, 36)
                    s = RP.fold(terms)
                    if i == j:
                        Hs, m = kf_sum[P.free_kf[i]], 0
                        for r in range(6):
                            for c in range(r, 6):
                                S[6 * i + c, 6 * i + r] = ((Hs[m] + lam) if r == c else Hs[m]) - s[6 * r + c]
                                m += 1
                        bS[6 * i:6 * i + 6] = Hs[21:27] - s[36:42]
                    else:
                        S[6 * j:6 * j + 6, 6 * i:6 * i + 6] = -s[:36].reshape(6, 6).T
        ok, xp, piv = ldlt_solve(S, bS, xp)
        for dj, ajj in piv:
            if ajj > 0 and dj == dj:
                res["margins"]["pivot"] = min(res["margins"]["pivot"], abs(dj) / ajj)
        M.solved = 1 if ok else 0
        cur, nxt = M.cur, 1 - M.cur
        with np.errstate(all="ignore"):
            if ok:
                t = bl.copy()
                for d in range(maxdeg):
                    sel = ve[P.rank[ve] == d]
                    sel = sel[~P.fixed[P.edge_kf[sel]]]
                    f = np.array([P.kf_free[int(k)] for k in P.edge_kf[sel]], np.int64)
                    Wm, pp = rec[sel, 9:27].reshape(-1, 6, 3), P.edge_pt[sel]
                    for r in range(6):
                        t[pp] = t[pp] - Wm[:, r, :] * xp[6 * f + r][:, None]
                Dm = Dall.reshape(-1, 3, 3)
                new = (Dm[:, :, 0] * t[:, None, 0] + Dm[:, :, 1] * t[:, None, 1]) + Dm[:, :, 2] * t[:, None, 2]
                xl[P.pt_edges > 0] = new[P.pt_edges > 0]
            pts[nxt] = pts[cur] + xl
            s = np.zeros(nP, D)
            for r in range(3):
                s = s + xl[:, r] * (lam * xl[:, r] + bl[:, r])
            untouched = P.pt_edges == 0
            pts[nxt][untouched] = pts[cur][untouched]
            s[untouched] = 0.0
            pscale[:] = s
            for k in range(nK):
                if k in P.kf_free:
                    f = P.kf_free[k]
                    poses[nxt][k] = RP.oplus(xp[6 * f:6 * f + 6], poses[cur][k])
            kf_pass(nxt, False)
            bp = kf_sum[P.free_kf][:, 21:27].reshape(-1)
            scale = fold1(np.concatenate([xp * (lam * xp + bp), pscale]))
        accepted = M.after_trial(fold1(kf_chi), scale)
        res["events"].append(("trial", M.iter, M.qmax, bool(accepted), bool(ok)))

    cur = M.cur
    hdr.update(iterations=M.iterations, trials=M.trials, rejected=M.rejected, ldlt_failures=M.failures)
    res["margins"]["rho"], res["margins"]["stop"] = M.margin_rho, M.margin_stop
    Tcw_out, points_out = res["Tcw_out"], res["points_out"]
    for k, f in P.kf_free.items():
        Tcw_out[k] = RP.to_tcw(poses[cur][k])
    points_out[P.pt_edges > 0] = pts[cur][P.pt_edges > 0].astype(F)
    for k in range(nK):
        idx = P.kf_edges[k]
        if not len(idx):
            continue
        r = RP.rotate(poses[cur][k][:4], [pts[cur][P.edge_pt[idx], c] for c in range(3)])
        z = r[2] + poses[cur][k][6]
        c2 = rec[idx, 27]
        th = np.where(P.stereo[idx], TH_STEREO, TH_MONO)
        with np.errstate(all="ignore"):
            res["erase"][idx] = (c2 > th) | ~(z > 0.0)
            res["chi2"][idx] = c2.astype(F)
            good = np.isfinite(c2)
            if good.any():
                res["margins"]["classify"] = min(res["margins"]["classify"], float(np.min(np.abs(c2[good] - th[good]) / th[good])))
            zf = z[np.isfinite(z)]
            if len(zf):
                res["margins"]["depth"] = min(res["margins"]["depth"], float(np.min(np.abs(zf))))
    hdr["erase"] = int(res["erase"].sum())
    res["header"] = np.array([hdr[k] for k in H_KEYS], np.int32)
    res["final_chi2"] = float(M.currentChi)
    res["poses"], res["points"] = poses[cur], pts[cur]
    return res
