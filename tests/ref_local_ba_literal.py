"""Optimizer::LocalBundleAdjustment (src/Optimizer.cc:1188-1460) the way the reference's own objects do it: vertex and edge objects, every sum
sequential in g2o's order (the edges in insertion order), push / pop on the vertices, numpy.linalg for the point blocks and the reduced system.  It
shares the per-edge formulas with tests/ref_local_ba.py (the lines of the C++ edges) and nothing else: no lanes, no folds, no LDL^T of its own.
tests/test_local_ba_forms.py holds the rule against it; tests/test_local_ba_ref.py holds its Jacobians against central differences."""
import math

import numpy as np

import ref_local_ba as R
import ref_poseopt as RP

D, F = np.float64, np.float32


class Vertex:
    def __init__(self, estimate, fixed, dim):
        self.estimate, self.fixed, self.dim, self.stack, self.index, self.edges = estimate, fixed, dim, [], -1, []

    def push(self):
        self.stack.append(self.estimate)

    def pop(self):
        self.estimate = self.stack.pop()

    def discard(self):
        self.stack.pop()


class Edge:
    def __init__(self, e, point, pose, obs, stereo):
        self.e, self.point, self.pose, self.obs, self.stereo, self.error = e, point, pose, obs, bool(stereo), None

    def compute_error(self, cam, w):
        _, er, _ = RP.edge_error(self.pose.estimate, cam, np.asarray(self.point.estimate, D), self.obs, self.stereo, w)
        self.error = np.array([float(er[0]), float(er[1]), float(er[2])], D)

    def chi2(self, w):
        """sum_r e_r (w e_r), as include/xfeat_hip.h states it: the information is w I, and no product with one of its zeros is formed (an infinite
        component makes chi2 Inf, not 0 * Inf)"""
        n = 3 if self.stereo else 2
        return float(sum(self.error[r] * (w * self.error[r]) for r in range(n)))

    def jacobians(self, cam):
        """linearizeOplus -> (rows x 3, rows x 6)"""
        pose, X = self.pose.estimate, np.asarray(self.point.estimate, D)
        r = RP.rotate(pose[:4], [X[0], X[1], X[2]])
        pc = [r[0] + pose[4], r[1] + pose[5], r[2] + pose[6]]
        n = 3 if self.stereo else 2
        Jp = np.array([float(v) for v in RP.edge_jacobian(cam, pc, self.stereo)], D).reshape(3, 6)[:n]
        Jl = np.array([float(v) for v in R.point_jacobian(cam, RP.matrix_from_quat(pose[:4]), pc, self.stereo)], D).reshape(3, 3)[:n]
        return Jl, Jp

    def depth(self):
        pose, X = self.pose.estimate, np.asarray(self.point.estimate, D)
        return RP.rotate(pose[:4], [X[0], X[1], X[2]])[2] + pose[6]


def literal(p):
    cam, w = RP.cam_of(p["cam"]), float(F(p["inv_sigma2"]))
    pose_table, point_table = np.asarray(p["pose_table"], F).reshape(-1, 12), np.asarray(p["point_table"], F).reshape(-1, 3)
    kf_row, point_row, fixed = np.asarray(p["kf_row"]), np.asarray(p["point_row"]), np.asarray(p["kf_fixed"]) != 0
    begin, edge_kf, obs = np.asarray(p["edge_begin"]), np.asarray(p["edge_kf"]), np.asarray(p["edge_obs"], F).reshape(-1, 3)
    nK, nP, nE = len(kf_row), len(point_row), len(edge_kf)
    poses = [Vertex(RP.from_tcw(pose_table[kf_row[k]]), bool(fixed[k]), 6) for k in range(nK)]
    points = [Vertex(point_table[point_row[q]].astype(D), False, 3) for q in range(nP)]
    edges = []
    for q in range(nP):
        for e in range(begin[q], begin[q + 1]):
            if 0 <= edge_kf[e] < nK:
                ed = Edge(e, points[q], poses[edge_kf[e]], obs[e].astype(D), not obs[e, 2] < 0)
                edges.append(ed)
                points[q].edges.append(ed)
                poses[edge_kf[e]].edges.append(ed)
    free = [v for v in poses if not v.fixed]
    hdr = dict.fromkeys(R.H_KEYS, 0)
    hdr.update(free=len(free), fixed_with_edge=sum(1 for v in poses if v.fixed and v.edges), mono=sum(1 for e in edges if not e.stereo),
               stereo=sum(1 for e in edges if e.stereo))
    res = dict(Tcw_out=pose_table[kf_row].copy(), points_out=point_table[point_row].copy(), erase=np.zeros(nE, np.uint8), chi2=np.zeros(nE, F), final_chi2=0.0,
               events=[])
    hdr["status"] = R.ABORTED if hdr["fixed_with_edge"] == 0 else (R.NOTHING_FREE if not free else R.OK)
    if hdr["status"] != R.OK:
        res["header"] = np.array([hdr[k] for k in R.H_KEYS], np.int32)
        return res
    for i, v in enumerate(free):
        v.index = i
    active_points = [v for v in points if v.edges]
    active = free + active_points
    nF = len(free)

    def robust_chi2():
        s = 0.0
        for e in edges:
            s += float(RP.huber(e.chi2(w), e.stereo)[0])
        return s

    def compute_errors():
        for e in edges:
            e.compute_error(cam, w)

    M = R.Machine(int(p.get("max_iterations", 10)))
    x_pose, x_point = np.zeros(6 * nF, D), {id(v): np.zeros(3, D) for v in active_points}
    with np.errstate(all="ignore"):
        while M.act != "done":
            compute_errors()
            chi = robust_chi2()
            Hpp, bp = np.zeros((nF, 6, 6), D), np.zeros((nF, 6), D)
            Hll, bl, W = {id(v): np.zeros((3, 3), D) for v in active_points}, {id(v): np.zeros(3, D) for v in active_points}, {}
            for e in edges:                                                   # buildSystem: constructQuadraticForm of each edge in insertion order
                Jl, Jp = e.jacobians(cam)
                n = len(Jl)
                rho1 = float(RP.huber(e.chi2(w), e.stereo)[1])
                Om = rho1 * w * np.eye(n)
                we = w * e.error[:n]
                Hll[id(e.point)] += Jl.T @ Om @ Jl
                bl[id(e.point)] -= rho1 * (Jl.T @ we)
                if not e.pose.fixed:
                    i = e.pose.index
                    Hpp[i] += Jp.T @ Om @ Jp
                    bp[i] -= rho1 * (Jp.T @ we)
                    W[(i, id(e.point))] = W.get((i, id(e.point)), np.zeros((6, 3), D)) + Jp.T @ Om @ Jl
            diag = [abs(Hpp[i][c, c]) for i in range(nF) for c in range(6)] + [abs(Hll[id(v)][c, c]) for v in points if v.edges for c in range(3)]
            M.after_build(chi, R.lambda_init(np.array(diag, D)))
            res["events"].append(("build", M.iter))
            while M.act == "trial":
                lam = M.lam
                for v in active:
                    v.push()
                S, bS = np.zeros((6 * nF, 6 * nF), D), bp.reshape(-1).copy()
                for i in range(nF):
                    S[6 * i:6 * i + 6, 6 * i:6 * i + 6] = Hpp[i] + lam * np.eye(6)
                Dinv = {}
                for v in active_points:                                       # the points in index order: the Schur sums over shared points ascending
                    Dv = np.linalg.inv(Hll[id(v)] + lam * np.eye(3)) if np.isfinite(Hll[id(v)]).all() and lam == lam else np.full((3, 3), np.nan)
                    Dinv[id(v)] = Dv
                    seen = sorted({e.pose.index for e in v.edges if not e.pose.fixed})
                    for i in seen:
                        Y = W[(i, id(v))] @ Dv
                        bS[6 * i:6 * i + 6] -= Y @ bl[id(v)]
                        for j in seen:
                            S[6 * i:6 * i + 6, 6 * j:6 * j + 6] -= Y @ W[(j, id(v))].T
                ok = bool(np.isfinite(S).all())                               # LinearSolverEigen::solve judges the matrix alone: a NaN in b makes a NaN x
                if ok:
                    try:
                        np.linalg.cholesky((S + S.T) / 2)
                        x_pose = np.linalg.solve(S, bS) if np.isfinite(bS).all() else np.full(6 * nF, np.nan)
                    except np.linalg.LinAlgError:
                        ok = False
                if ok:
                    for v in active_points:
                        t = bl[id(v)].copy()
                        for i in sorted({e.pose.index for e in v.edges if not e.pose.fixed}):
                            t -= W[(i, id(v))].T @ x_pose[6 * i:6 * i + 6]
                        x_point[id(v)] = Dinv[id(v)] @ t
                M.solved = 1 if ok else 0
                scale = 0.0
                for j in range(6 * nF):
                    scale += x_pose[j] * (lam * x_pose[j] + bp.reshape(-1)[j])
                for v in free:
                    v.estimate = RP.oplus(x_pose[6 * v.index:6 * v.index + 6], v.estimate)
                for v in active_points:
                    v.estimate = v.estimate + x_point[id(v)]
                    for c in range(3):
                        scale += x_point[id(v)][c] * (lam * x_point[id(v)][c] + bl[id(v)][c])
                compute_errors()
                accepted = M.after_trial(robust_chi2(), scale)
                for v in active:
                    v.discard() if accepted else v.pop()
                res["events"].append(("trial", M.iter, M.qmax, bool(accepted), bool(ok)))
        hdr.update(iterations=M.iterations, trials=M.trials, rejected=M.rejected, ldlt_failures=M.failures)
        for k, v in enumerate(poses):
            if not v.fixed:
                res["Tcw_out"][k] = RP.to_tcw(v.estimate)
        for q, v in enumerate(points):
            if v.edges:
                res["points_out"][q] = np.asarray(v.estimate, D).astype(F)
        for e in edges:                                                       # e->chi2() reads _error as the last computeActiveErrors() left it
            c2 = e.chi2(w)
            res["erase"][e.e] = c2 > (R.TH_STEREO if e.stereo else R.TH_MONO) or not e.depth() > 0.0
            res["chi2"][e.e] = F(c2)
    hdr["erase"] = int(res["erase"].sum())
    res["header"] = np.array([hdr[k] for k in R.H_KEYS], np.int32)
    res["final_chi2"] = float(M.currentChi)
    return res
