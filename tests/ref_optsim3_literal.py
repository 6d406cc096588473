"""Optimizer::OptimizeSim3 (reference src/Optimizer.cc:2100-2381) transcribed with the objects the reference has: a g2o::Sim3 with the members of
thirdparty/g2o/g2o/types/sim3.h, a VertexSim3Expmap with push / pop / oplus, EdgeSim3ProjectXYZ and EdgeInverseSim3ProjectXYZ with a stored _error, a
robust kernel that can be taken away and the numeric linearizeOplus of base_binary_edge.hpp:130-205 restated on its own through the vertex's push /
oplus / pop, an optimizer that sums the active edges one after the other in insertion order (e12 of pair 0, e21 of pair 0, e12 of pair 1, ..) into a
7 x 7 matrix, and the Levenberg solve() line by line with a LAPACK factorisation standing in for Eigen's LDLT.  numpy only.

It shares with tests/ref_optsim3.py (the kernel's rule) the Sim3 exponential of sim3.h:70-142, the quaternion-times-vector formula, the Huber
formula, the pair set-up and the result layout.  The Sim3 product, the inverse, the map, the Levenberg step with its stop rules, the sums, the
Jacobian bookkeeping and the solve are transcribed here on their own: what the two forms differ by is the reference's own freedom."""
import numpy as np

import ref_optsim3 as R
import ref_poseopt as RP

D, F = np.float64, np.float32


class Sim3:
    def __init__(self, r, t, s):
        self.r, self.t, self.s = list(r), list(t), float(s)

    @classmethod
    def from_update(cls, u):
        e = R.exp7(u)
        return cls(e[:4], e[4:7], e[7])

    def map(self, X):
        v = RP.rotate(self.r, X)
        return [self.s * v[0] + self.t[0], self.s * v[1] + self.t[1], self.s * v[2] + self.t[2]]

    def inverse(self):
        c = [-self.r[0], -self.r[1], -self.r[2], self.r[3]]
        m = -1.0 / self.s
        return Sim3(c, RP.rotate(c, [m * self.t[0], m * self.t[1], m * self.t[2]]), 1.0 / self.s)

    def __mul__(self, o):
        """ret.r = r * other.r (Eigen's quaternion product, written from its definition on (w, x, y, z)); ret.t = s * (r * other.t) + t; ret.s = s * other.s"""
        aw, ax, ay, az = self.r[3], self.r[0], self.r[1], self.r[2]
        bw, bx, by, bz = o.r[3], o.r[0], o.r[1], o.r[2]
        w = aw * bw - ax * bx - ay * by - az * bz
        x = aw * bx + ax * bw + ay * bz - az * by
        y = aw * by + ay * bw + az * bx - ax * bz
        z = aw * bz + az * bw + ax * by - ay * bx
        rt = RP.rotate(self.r, o.t)
        return Sim3([x, y, z, w], [self.s * rt[0] + self.t[0], self.s * rt[1] + self.t[1], self.s * rt[2] + self.t[2]], self.s * o.s)

    def as_list(self):
        return self.r + self.t + [self.s]


class VertexSim3Expmap:
    def __init__(self, estimate, fix_scale):
        self._estimate, self._fix_scale, self._backup = estimate, bool(fix_scale), []

    def estimate(self):
        return self._estimate

    def push(self):
        self._backup.append(self._estimate)

    def pop(self):
        self._estimate = self._backup.pop()

    def oplus(self, update):
        update = [float(v) for v in update]
        if self._fix_scale:
            update[6] = 0.0
        self._estimate = Sim3.from_update(update) * self._estimate


class Edge:
    """EdgeSim3ProjectXYZ (inverse=False: camera 1 sees S12.map(P3D2c)) or EdgeInverseSim3ProjectXYZ (camera 2 sees S12.inverse().map(P3D1c))"""

    def __init__(self, vertex, inverse, cam, X, measurement, information, delta):
        self.v, self.inverse, self.cam, self.X, self.z, self.w, self.delta = vertex, inverse, cam, [float(x) for x in X], [float(m) for m in measurement], information, delta
        self._error, self.J = [0.0, 0.0], None

    def computeError(self):
        S = self.v.estimate()
        p = (S.inverse() if self.inverse else S).map(self.X)
        with np.errstate(all="ignore"):
            proj = [float(D(self.cam[0]) * p[0] / D(p[2]) + self.cam[2]), float(D(self.cam[1]) * p[1] / D(p[2]) + self.cam[3])]
        self._error = [self.z[0] - proj[0], self.z[1] - proj[1]]

    def chi2(self):
        e = self._error
        return e[0] * (self.w * e[0]) + e[1] * (self.w * e[1])

    def rho(self):
        c = self.chi2()
        if self.delta is None:
            return c, 1.0
        r0, r1 = R.huber(D(c), self.delta)
        return float(r0), float(r1)

    def linearizeOplus(self):
        delta = 1e-9
        scalar = 1.0 / (2 * delta)
        before = list(self._error)
        add = [0.0] * 7
        J = np.zeros((2, 7), D)
        for d in range(7):
            self.v.push()
            add[d] = delta
            self.v.oplus(add)
            self.computeError()
            bak = list(self._error)
            self.v.pop()
            self.v.push()
            add[d] = -delta
            self.v.oplus(add)
            self.computeError()
            bak = [bak[0] - self._error[0], bak[1] - self._error[1]]
            self.v.pop()
            add[d] = 0.0
            J[:, d] = [scalar * bak[0], scalar * bak[1]]
        self._error = before
        self.J = J


def _levenberg_accept(S, tempChi):
    """optimization_algorithm_levenberg.cpp:129-166, transcribed on its own: rho, the accept / reject update of lambda, the stop rules.
    -> 'trial' (another trial of this iteration) | 'stop' (terminate) | 'ok', accepted"""
    rho = S["currentChi"] - tempChi
    scale = float(np.dot(np.asarray(S["x"], D), S["lam"] * np.asarray(S["x"], D) + np.asarray(S["b"], D)))      # computeScale()
    scale += 1e-3
    with np.errstate(all="ignore"):
        rho = float(D(rho) / D(scale))
    good = rho > 0 and bool(np.isfinite(tempChi))
    if good:
        alpha = 1.0 - pow(2 * rho - 1, 3)
        alpha = min(alpha, 2.0 / 3.0)                                      # _goodStepUpperScale
        scaleFactor = max(1.0 / 3.0, alpha)                                # _goodStepLowerScale
        S["lam"] *= scaleFactor
        S["ni"] = 2.0
        S["currentChi"] = tempChi
    else:
        S["lam"] *= S["ni"]
        S["ni"] *= 2
    S["qmax"] += 1
    if rho < 0 and S["qmax"] < 10:                                         # while (rho < 0 && qmax < _maxTrialsAfterFailure->value())
        return "trial", good
    if S["qmax"] == 10 or rho == 0:
        return "stop", good                                                # Terminate
    # SparseOptimizer::optimize: three iterations in a row that gain less than a thousandth end it
    if (S["iniChi"] - S["currentChi"]) * 1e3 < S["iniChi"]:
        S["nbad"] += 1
    else:
        S["nbad"] = 0
    return ("stop" if S["nbad"] >= 3 else "ok"), good


def _solve(H, lam, b):
    """(H + lambda I) x = b with LAPACK: ok = the matrix is positive definite (Eigen: ldlt.isPositive())"""
    A = H + lam * np.eye(7)
    if not np.all(np.isfinite(A)) or not np.all(np.isfinite(b)):
        return False, None
    try:
        np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return False, None
    return True, np.linalg.solve(A, b)


def literal(p, stale=True):
    cam1, cam2 = R.cam_of(p["cam1"]), R.cam_of(p["cam2"])
    w1, w2, th2 = float(F(p["inv_sigma2_1"])), float(F(p["inv_sigma2_2"])), float(F(p["th2"]))
    delta = float(F(np.sqrt(F(p["th2"]))))
    st, P1, P2, o1, o2 = R.pairs_of(p)
    n1 = len(st)
    v = VertexSim3Expmap(Sim3(*(lambda e: (e[:4], e[4:7], e[7]))(R.state_from(p["S12"]))), p["fix_scale"])
    inp = v.estimate()
    idx = [int(i) for i in np.nonzero(st & R.EDGE)[0]]
    e12 = {i: Edge(v, False, cam1, P2[i].astype(D), o1[i].astype(D), w1, delta) for i in idx}
    e21 = {i: Edge(v, True, cam2, P1[i].astype(D), o2[i].astype(D), w2, delta) for i in idx}
    in2 = (st & R.IN_KF2) != 0
    n_corr, n_out = len(idx), sum(1 for i in idx if not in2[i])
    hdr = [n_corr, n_corr - n_out, n_out, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    bad1, bad2 = np.zeros(n1, bool), np.zeros(n1, bool)
    cls1, cls2 = np.full((n1, 2), np.nan), np.full((n1, 2), np.nan)
    S = dict(x=[0.0] * 7, currentChi=0.0)
    events, piv_min, has2 = [], np.inf, np.zeros(n1, bool)

    def active():
        return [e for i in idx if not bad1[i] for e in (e12[i], e21[i])]

    def robust_chi2(es):
        s = 0.0
        for e in es:
            s += e.rho()[0]
        return s

    def optimize(iterations):
        es = active()
        for i in range(iterations if es else 0):
            for e in es:
                e.computeError()
            S["currentChi"] = robust_chi2(es)
            S["iniChi"] = S["currentChi"]
            H, b = np.zeros((7, 7), D), np.zeros(7, D)
            with np.errstate(all="ignore"):
                for e in es:                                              # linearizeOplus + constructQuadraticForm, edge after edge
                    e.linearizeOplus()
                    r1 = e.rho()[1]
                    omega_r = -(e.w * np.array(e._error, D)) * r1
                    b += e.J.T @ omega_r
                    H += e.J.T @ ((r1 * e.w) * e.J)
            S["b"] = b.tolist()
            if i == 0:
                S["lam"], S["ni"], S["nbad"] = 1e-5 * max([0.0] + [abs(float(H[j, j])) for j in range(7)]), 2.0, 0
            S["qmax"] = 0
            hdr[8] += 1
            while True:
                v.push()
                ok, x = _solve(H, S["lam"], b)
                if ok:
                    S["x"] = x.tolist()
                v.oplus(S["x"])
                hdr[9] += 1
                hdr[11] += 0 if ok else 1
                for e in es:
                    e.computeError()
                step, accepted = _levenberg_accept(S, robust_chi2(es) if ok else R.DBL_MAX)
                if accepted:
                    v._backup.pop()                                       # discardTop()
                else:
                    v.pop()                                               # the edges keep the errors of the rejected estimate
                    hdr[10] += 1
                events.append((accepted, ok))
                if step != "trial":
                    break
            if step == "stop":
                break

    def too_large(i):
        return e12[i].chi2() > th2 or e21[i].chi2() > th2

    optimize(5)
    hdr[7] += 1
    for i in idx:
        if not stale:
            e12[i].computeError()
            e21[i].computeError()
        cls1[i] = [e12[i].chi2(), e21[i].chi2()]
        if too_large(i):
            bad1[i] = True
            hdr[3] += 1
            hdr[4] += 0 if in2[i] else 1
        else:
            e12[i].delta = e21[i].delta = None                            # setRobustKernel(0)
    hdr[5] = 10 if hdr[3] > 0 else 5
    if n_corr - hdr[3] < 10:
        est = inp
    else:
        optimize(hdr[5])
        hdr[7] += 1
        n_in = 0
        for i in idx:
            if bad1[i]:
                continue
            e12[i].computeError()
            e21[i].computeError()
            cls2[i], has2[i] = [e12[i].chi2(), e21[i].chi2()], True
            if too_large(i):
                bad2[i] = True
            else:
                n_in += 1
        hdr[6] = n_in
        est = v.estimate()
    last = np.where(has2[:, None], cls2, cls1)
    return R.result(p, est.as_list(), st, bad1, bad2, last, hdr, S["currentChi"], cls1, cls2, events, piv_min)
