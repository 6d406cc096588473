"""numpy fp32 restatement of ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono) (src/ORBmatcher.cc:1861-2047) and of
the SearchLocalPoints form (:42-141) as include/xfeat_hip.h states them: the plain sequential loop, one query at a time (test
infrastructure, no GPU; shares no code with the library).

  project   :1888-1909 / :1938 with Pinhole::project (src/CameraModels/Pinhole.cpp:43-49): x3Dc from a row-major 3x4 [R|t] in the
            stated order, invzc = (float)(1.0 / (double)zc), u = fx*xc/zc + cx, the bounds cull, ur = u - bf*invzc
  search    the loop: Frame::GetFeaturesInArea (ref_window.features_in_area), the uright filter, the claim test against what EARLIER
            iterations wrote (:1932-1934 / :87-89), best / second with the oracle's best2_csr (the DescriptorDistance the window
            tests use), the acceptance rule (:1955 / :122-127), the write (:1957 / :128)
  scene     the seeded inputs of the tests: world points from the last frame's keypoints and a seeded depth, a small seeded pose,
            flags with about half the claim bits set and about 10 % inactive

Every fp32 expression is evaluated in np.float32 in the written order (numpy never contracts a multiply and an add).
"""
import numpy as np

import ref_window as RW

F = np.float32
D = np.float64
INACTIVE, BEHIND, OUT_OF_BOUNDS, NO_CANDIDATES, REJECTED, MATCHED = range(6)
VISIBLE = NO_CANDIDATES                                     # what the projection stage calls a point that reaches the search


def project(T, cam, bounds, xyz):
    """-> u, v, ur (fp32 arrays), status (BEHIND / OUT_OF_BOUNDS / VISIBLE).  BEHIND: u = v = ur = 0."""
    T = np.asarray(T, F).reshape(12)
    p = np.asarray(xyz, F).reshape(-1, 3)
    X, Y, Z = p[:, 0], p[:, 1], p[:, 2]
    fx, fy, cx, cy, bf = (F(cam[k]) for k in ("fx", "fy", "cx", "cy", "bf"))
    mnx, mny, mxx, mxy = (F(b) for b in bounds)
    with np.errstate(all="ignore"):
        xc = ((T[0] * X + T[1] * Y) + T[2] * Z) + T[3]
        yc = ((T[4] * X + T[5] * Y) + T[6] * Z) + T[7]
        zc = ((T[8] * X + T[9] * Y) + T[10] * Z) + T[11]
        invz = (D(1.0) / zc.astype(D)).astype(F)
        behind = invz < 0
        u = (fx * xc) / zc + cx
        v = (fy * yc) / zc + cy
        ur = u - bf * invz
        out = (u < mnx) | (u > mxx) | (v < mny) | (v > mxy)
    st = np.where(behind, BEHIND, np.where(out, OUT_OF_BOUNDS, VISIBLE)).astype(np.uint8)
    z = F(0)
    return np.where(behind, z, u).astype(F), np.where(behind, z, v).astype(F), np.where(behind, z, ur).astype(F), st


def search(O, status_in, claims, u, v, r, ur, qdesc, grid, x, y, bounds, tg, skip=None, uright=None, init_dist=256, th_high=1000, nn_ratio=0.0):
    """the sequential loop over the queries in index order.  status_in[q] == VISIBLE: the query reaches the search; anything else is
    kept as the query's status.  r: one radius or one per query.  O: the oracle module (best2_csr)."""
    nq, nt = len(qdesc), len(tg)
    r = np.broadcast_to(np.asarray(r, F), (nq,))
    x = np.asarray(x, F); y = np.asarray(y, F)
    claimed = np.zeros(nt, bool) if skip is None else (np.asarray(skip) != 0)
    claimed = claimed.copy()
    assigned = np.full(nt, -1, np.int32)
    status = np.asarray(status_in, np.uint8).copy()
    match = np.full(nq, -1, np.int32); best = np.full(nq, init_dist, np.int32); second = np.full(nq, init_dist, np.int32)
    ncand = np.zeros(nq, np.int32)
    n_matches = 0
    for q in range(nq):
        if status[q] != VISIBLE:
            continue
        c = RW.features_in_area(grid, x, y, u[q], v[q], r[q], bounds)
        if uright is not None and len(c):
            w = np.asarray(uright, F)[c]
            with np.errstate(all="ignore"):
                c = c[~((w > 0) & (np.abs(F(ur[q]) - w) > r[q]))]
        c = c[~claimed[c]]
        ncand[q] = len(c)
        if len(c) == 0:
            status[q] = NO_CANDIDATES
            continue
        bi, bd, si, sd = (int(a[0]) for a in O.best2_csr(qdesc[q:q + 1], tg, np.array([0, len(c)], np.int32), c, init_dist))
        best[q] = bd; second[q] = sd
        accept = bi >= 0 and bd <= th_high and not (nn_ratio > 0 and si >= 0 and F(bd) > F(nn_ratio) * F(sd))
        if not accept:
            status[q] = REJECTED
            continue
        status[q] = MATCHED; match[q] = bi; assigned[bi] = q; n_matches += 1
        if claims[q]:
            claimed[bi] = True
    return dict(status=status, match_idx=match, best_dist=best, second_dist=second, n_candidates=ncand, assigned=assigned, n_matches=n_matches)


def pose(seed, shift=(2.0, 1.0), depth=2.1, cam=None, angle=0.002):
    """a small seeded pose as a row-major 3x4 fp32 matrix: rotations of about `angle` rad about the three axes (composed in float64,
    rounded once) and the translation that moves a point at `depth` by `shift` pixels"""
    rng = np.random.RandomState(seed)
    a, b, c = rng.uniform(-angle, angle, 3)
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    t = np.array([shift[0] * depth / float(cam["fx"]), shift[1] * depth / float(cam["fy"]), rng.uniform(-0.01, 0.01)])
    return np.concatenate([Rz @ Ry @ Rx, t[:, None]], 1).astype(F).reshape(12)


def scene(seed, xy_last, cam, inactive=0.1, claiming=0.5):
    """world points of the last frame's keypoints (its camera frame is the world frame) at a seeded depth of 1.9 .. 2.3 m, and the
    query flags: bit0 active (about 90 %), bit1 "the map point has observations" (about half)"""
    rng = np.random.RandomState(seed)
    xy = np.asarray(xy_last, F).reshape(-1, 2)
    n = len(xy)
    z = rng.uniform(1.9, 2.3, n).astype(F)
    xyz = np.stack([(xy[:, 0] - F(cam["cx"])) / F(cam["fx"]) * z, (xy[:, 1] - F(cam["cy"])) / F(cam["fy"]) * z, z], 1).astype(F)
    flags = ((rng.rand(n) >= inactive).astype(np.uint8) | ((rng.rand(n) < claiming).astype(np.uint8) << 1)).astype(np.uint8)
    return xyz, flags
