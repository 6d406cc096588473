"""TwoViewReconstruction::Reconstruct for the Pinhole camera, restated literally from the reference's behaviour: float32 throughout, every sum
sequential, and numpy's float32 LAPACK SVD / inverse standing in for Eigen's JacobiSVD<float> / inverse() (which cannot be reproduced bit for
bit).  The rule form of tests/ref_twoview.py is compared with this one in tests/test_twoview_forms.py: the decisions must be equal and the pose
and points close.  This file restates every formula itself -- the design matrices, the transfer and epipolar errors, the projection matrices,
the triangulation and CheckRT's gates, as float32 matrix products where the reference has Eigen products -- so that a wrong line of the rule does
not sit in both forms; it takes from the rule's file only the transcription of the shrinking-vector set loop (itself the reference's loop),
(float)(1.0 / (double)x), and the status names."""
from __future__ import annotations

import numpy as np

import ref_twoview as R

F, D = np.float32, np.float64


def seqsum(x):
    x = np.asarray(x, F)
    return np.cumsum(x, dtype=F)[-1] if len(x) else F(0)


def svd32(A):
    return np.linalg.svd(np.asarray(A, F))


def null32(A):
    return svd32(A)[2][..., -1, :]


def normalize(xy):
    xy = np.asarray(xy, F)
    n = F(len(xy))
    mx, my = F(seqsum(xy[:, 0]) / n), F(seqsum(xy[:, 1]) / n)
    dx, dy = F(seqsum(np.abs(xy[:, 0] - mx)) / n), F(seqsum(np.abs(xy[:, 1] - my)) / n)
    sx, sy = R.inv_d(dx), R.inv_d(dy)
    T = np.array([[sx, 0, (-mx) * sx], [0, sy, (-my) * sy], [0, 0, 1]], F)
    pts = np.stack([(xy[:, 0] - mx) * sx, (xy[:, 1] - my) * sy], -1).astype(F)
    return pts, T


def design_h(p1, p2):
    """ComputeH21's A for K sets of eight pairs [K][8][2] -> [K][16][9]"""
    K = len(p1)
    A = np.zeros((K, 16, 9), F)
    for i in range(8):
        u1, v1, u2, v2 = p1[:, i, 0], p1[:, i, 1], p2[:, i, 0], p2[:, i, 1]
        z, o = np.zeros(K, F), np.ones(K, F)
        A[:, 2 * i] = np.stack([z, z, z, -u1, -v1, -o, v2 * u1, v2 * v1, v2], -1)
        A[:, 2 * i + 1] = np.stack([u1, v1, o, z, z, z, -u2 * u1, -u2 * v1, -u2], -1)
    return A


def design_f(p1, p2):
    K = len(p1)
    A = np.zeros((K, 8, 9), F)
    for i in range(8):
        u1, v1, u2, v2 = p1[:, i, 0], p1[:, i, 1], p2[:, i, 0], p2[:, i, 1]
        A[:, i] = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones(K, F)], -1)
    return A


def homog(xy):
    return np.concatenate([np.asarray(xy, F), np.ones((len(xy), 1), F)], 1)


def check_homography(H21, H12, x1, x2, sigma):
    """K models [K][3][3], the N matches as homogeneous pixels [N][3] -> chi [K][N][2], bIn [K][N], the two halves of the score [K][N][2]"""
    inv_s2 = R.inv_d(F(sigma) * F(sigma))
    a = np.einsum("kij,nj->kni", H12, x2).astype(F)                         # x2 in image 1
    w = R.inv_d(a[..., 2])
    d1 = (x1[None, :, 0] - a[..., 0] * w) ** 2 + (x1[None, :, 1] - a[..., 1] * w) ** 2
    b = np.einsum("kij,nj->kni", H21, x1).astype(F)                         # x1 in image 2
    w = R.inv_d(b[..., 2])
    d2 = (x2[None, :, 0] - b[..., 0] * w) ** 2 + (x2[None, :, 1] - b[..., 1] * w) ** 2
    chi = np.stack([d1 * inv_s2, d2 * inv_s2], -1).astype(F)
    th = F(5.991)
    return chi, ~(chi > th).any(-1), np.where(chi > th, F(0), th - chi).astype(F)


def check_fundamental(F21, x1, x2, sigma):
    inv_s2 = R.inv_d(F(sigma) * F(sigma))
    l2 = np.einsum("kij,nj->kni", F21, x1).astype(F)                        # F21 x1
    num2 = (l2 * x2[None]).sum(-1, dtype=F)
    l1 = np.einsum("kji,nj->kni", F21, x2).astype(F)                        # x2^T F21
    num1 = (l1 * x1[None]).sum(-1, dtype=F)
    chi = np.stack([num2 * num2 / (l2[..., 0] ** 2 + l2[..., 1] ** 2) * inv_s2, num1 * num1 / (l1[..., 0] ** 2 + l1[..., 1] ** 2) * inv_s2], -1).astype(F)
    th, ts = F(3.841), F(5.991)
    return chi, ~(chi > th).any(-1), np.where(chi > th, F(0), ts - chi).astype(F)


def check_rt(K, Rm, t, x1, x2, th2):
    """CheckRT for the inlier pairs (pixels [n][2]) -> counted [n], good [n], cosParallax [n], points [n][3]"""
    n = len(x1)
    P1 = np.concatenate([K, np.zeros((3, 1), F)], 1).astype(F)
    P2 = (K @ np.concatenate([Rm, t[:, None]], 1)).astype(F)
    O2 = (-Rm.T @ t).astype(F)
    A = np.zeros((n, 4, 4), F)
    A[:, 0] = x1[:, :1] * P1[2] - P1[0]
    A[:, 1] = x1[:, 1:] * P1[2] - P1[1]
    A[:, 2] = x2[:, :1] * P2[2] - P2[0]
    A[:, 3] = x2[:, 1:] * P2[2] - P2[1]
    counted, good, cosv, pts = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, F), np.zeros((n, 3), F)
    for i in range(n):
        try:
            h = np.linalg.svd(A[i])[2][-1]
        except np.linalg.LinAlgError:
            continue
        p = (h[:3] / h[3]).astype(F)
        pts[i] = p
        if not np.isfinite(p).all():
            continue
        n1, n2 = p, (p - O2).astype(F)
        c = F(F(n1 @ n2) / (F(np.sqrt(F(n1 @ n1))) * F(np.sqrt(F(n2 @ n2)))))
        cosv[i] = c
        par = D(c) < 0.99998
        if p[2] <= 0 and par:
            continue
        q = (Rm @ p + t).astype(F)
        if q[2] <= 0 and par:
            continue
        iz1, iz2 = R.inv_d(p[2]), R.inv_d(q[2])
        e1 = (K[0, 0] * p[0] * iz1 + K[0, 2] - x1[i, 0]) ** 2 + (K[1, 1] * p[1] * iz1 + K[1, 2] - x1[i, 1]) ** 2
        if e1 > th2:
            continue
        e2 = (K[0, 0] * q[0] * iz2 + K[0, 2] - x2[i, 0]) ** 2 + (K[1, 1] * q[1] * iz2 + K[1, 2] - x2[i, 1]) ** 2
        if e2 > th2:
            continue
        counted[i], good[i] = True, par
    return counted, good, cosv, pts


def argmax_first(score):
    best, win = F(0), -1
    for it in range(len(score)):
        if score[it] > best:
            best, win = score[it], it
    return win, best


def literal(xy1, xy2, m12, cam, draws, rand_max, sigma=1.0, min_parallax=1.0, min_tri=50):
    xy1, xy2, m12 = np.asarray(xy1, F).reshape(-1, 2), np.asarray(xy2, F).reshape(-1, 2), np.asarray(m12, np.int32)
    draws = np.asarray(draws, np.int32).reshape(-1, 8)
    n1, iters = len(xy1), len(draws)
    cm1 = np.nonzero(m12 >= 0)[0]
    cm2 = m12[cm1]
    N = len(cm1)
    r = dict(N=N, status=R.TOO_FEW, model=0, win_h=-1, win_f=-1, chosen=-1, tri=np.zeros(n1, bool), p3d=np.zeros((n1, 3), F), T21=np.zeros((3, 4), F),
             inl_h=np.zeros(n1, bool), inl_f=np.zeros(n1, bool), motions=np.zeros((0, 12), F), ngood=[], parallax=[], margins={})
    if N < 8:
        return r
    with np.errstate(all="ignore"):
        sets = np.array([R.set_of_iteration(d, rand_max, N) for d in draws], np.int64)
        pn1, T1 = normalize(xy1)
        pn2, T2 = normalize(xy2)
        T2inv, T2t = np.linalg.inv(T2).astype(F), T2.T.copy()
        p1, p2 = pn1[cm1[sets]], pn2[cm2[sets]]
        Hn = null32(design_h(p1, p2)).reshape(iters, 3, 3)
        fpre = null32(design_f(p1, p2)).reshape(iters, 3, 3)
        U, w, Vt = svd32(fpre)
        w[:, 2] = 0
        Fn = (U * w[:, None, :]) @ Vt
        H21 = (T2inv @ Hn @ T1).astype(F)
        H12 = np.linalg.inv(H21).astype(F)
        F21 = (T2t @ Fn @ T1).astype(F)
        X1, X2 = homog(xy1[cm1]), homog(xy2[cm2])
        score, chis = [], []
        for m in range(2):
            chi, inl, halves = check_homography(H21, H12, X1, X2, sigma) if m == 0 else check_fundamental(F21, X1, X2, sigma)
            score.append(np.array([seqsum(h) for h in halves.reshape(iters, 2 * N)], F))       # chi1 of match 0, chi2 of match 0, chi1 of match 1, ..
            chis.append((chi, inl))
        (winH, SH), (winF, SF) = argmax_first(score[0]), argmax_first(score[1])
        r.update(win_h=winH, win_f=winF, SH=SH, SF=SF, score=score, chi=[chis[0][0][winH] if winH >= 0 else None, chis[1][0][winF] if winF >= 0 else None])
        if winH >= 0:
            r["inl_h"][cm1] = chis[0][1][winH]
        if winF >= 0:
            r["inl_f"][cm1] = chis[1][1][winF]
        # how far every decision of the scoring sits from its threshold
        for m, win, th in ((0, winH, 5.991), (1, winF, 3.841)):
            if win >= 0:
                r["margins"][f"chi_{'hf'[m]}"] = float(np.abs(chis[m][0][win].astype(D) - th).min())
                others = np.delete(score[m], win)
                r["margins"][f"lead_{'hf'[m]}"] = float(score[m][win] - others.max()) if len(others) else float(score[m][win])
        if F(SH + SF) == 0:
            r["status"] = R.BOTH_ZERO
            return r
        RH = F(SH / F(SH + SF))
        r["RH"] = RH
        r["margins"]["RH"] = abs(float(RH) - 0.5)
        fx, fy, cx, cy = [F(c) for c in cam]
        K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], F)
        model = R.MODEL_H if D(RH) > 0.50 else R.MODEL_F
        r["model"] = model
        inl = r["inl_h"] if model == R.MODEL_H else r["inl_f"]
        Ninl = int(inl.sum())
        idx = np.nonzero(inl)[0]
        if model == R.MODEL_F:
            E = (K.T @ F21[winF] @ K).astype(F)
            U, _, Vt = svd32(E)
            t = U[:, 2] / F(np.sqrt(F((U[:, 2] * U[:, 2]).sum(dtype=F))))
            W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], F)
            R1, R2 = (U @ W @ Vt).astype(F), (U @ W.T @ Vt).astype(F)
            R1 = -R1 if np.linalg.det(R1) < 0 else R1
            R2 = -R2 if np.linalg.det(R2) < 0 else R2
            motions = [(R1, t), (R2, t), (R1, -t), (R2, -t)]
        else:
            A = (np.linalg.inv(K).astype(F) @ H21[winH] @ K).astype(F)
            U, w, Vt = svd32(A)
            V = Vt.T
            s = F(np.linalg.det(U)) * F(np.linalg.det(Vt))
            d1, d2, d3 = w
            r["margins"]["d_ratio"] = float(min(D(d1 / d2), D(d2 / d3)) - 1.00001)
            if D(d1 / d2) < 1.00001 or D(d2 / d3) < 1.00001:
                r["status"] = R.H_DEGENERATE
                return r
            aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)); aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
            x1, x3 = [aux1, aux1, -aux1, -aux1], [aux3, -aux3, aux3, -aux3]
            root = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3))
            ast, ct = root / ((d1 + d3) * d2), (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
            asp, cp = root / ((d1 - d3) * d2), (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
            sth, sph = [ast, -ast, -ast, ast], [asp, -asp, -asp, asp]
            motions = []
            for i in range(4):
                Rp = np.array([[ct, 0, -sth[i]], [0, 1, 0], [sth[i], 0, ct]], F)
                tp = np.array([x1[i], 0, -x3[i]], F) * (d1 - d3)
                tt = (U @ tp).astype(F)
                motions.append(((s * U @ Rp @ Vt).astype(F), tt / F(np.linalg.norm(tt))))
            for i in range(4):
                Rp = np.array([[cp, 0, sph[i]], [0, -1, 0], [sph[i], 0, -cp]], F)
                tp = np.array([x1[i], 0, x3[i]], F) * (d1 + d3)
                tt = (U @ tp).astype(F)
                motions.append(((s * U @ Rp @ Vt).astype(F), tt / F(np.linalg.norm(tt))))
        Rts = np.array([np.concatenate([Rm, np.asarray(t, F)[:, None]], 1).reshape(12) for Rm, t in motions], F)
        r["motions"] = Rts
        ngood, par, per = [], [], []
        for Rt in Rts:
            Rm, t = Rt.reshape(3, 4)[:, :3], Rt.reshape(3, 4)[:, 3]
            counted, good, c, p = check_rt(K, Rm, t, xy1[idx], xy2[m12[idx]], F(4.0 * D(F(sigma) * F(sigma))))
            v = np.where(counted, np.where(good, 2, 1), 0)
            cs = np.sort(c[counted])                                             # sort(vCosParallax)
            ngood.append(int(counted.sum()))
            par.append(F(D(np.arccos(cs[min(50, len(cs) - 1)])) * 180.0 / np.pi) if len(cs) else F(0))
            per.append((v, p))
        r.update(ngood=ngood, parallax=par)
        mp = float(min_parallax)
        if model == R.MODEL_F:
            mx = max(ngood)
            nmin = max(int(0.9 * Ninl), min_tri)
            nsim = sum(g > 0.7 * mx for g in ngood)
            r["margins"]["similar"] = min(abs(g - 0.7 * mx) for g in ngood)
            r["margins"]["min_good"] = abs(mx - nmin) + 0.5
            if mx < nmin or nsim > 1:
                r["status"] = R.F_NO_WINNER
                return r
            h = ngood.index(mx)
            r["margins"]["parallax"] = abs(float(par[h]) - mp)
            if not par[h] > mp:
                r["status"] = R.LOW_PARALLAX
                return r
            r["status"] = R.OK_F
        else:
            best = second = 0
            h = -1
            for i, g in enumerate(ngood):
                if g > best:
                    second, best, h = best, g, i
                elif g > second:
                    second = g
            r["margins"]["second"] = abs(second - 0.75 * best)
            r["margins"]["n09"] = abs(best - 0.9 * Ninl)
            if not (second < 0.75 * best and best > min_tri and best > 0.9 * Ninl) or h < 0:
                r["status"] = R.H_GATES
                return r
            r["margins"]["parallax"] = abs(float(par[h]) - mp)
            if not par[h] >= mp:
                r["status"] = R.LOW_PARALLAX
                return r
            r["status"] = R.OK_H
        v, p = per[h]
        r["chosen"] = h
        r["tri"][idx] = v == 2
        r["p3d"][idx[v != 0]] = p[v != 0]
        r["T21"] = Rts[h].reshape(3, 4)
    return r
