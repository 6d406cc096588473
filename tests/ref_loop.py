"""numpy fp32 restatements of the loop-closing and relocalisation matchers as include/xfeat_hip.h states them, one query at a time,
written from the reference's lines (test infrastructure, no GPU; shares no code with the library):

  map_project / map_search    the Sim3 forms of ORBmatcher::SearchByProjection (src/ORBmatcher.cc:612-717, :719-831) and the relocalisation
                              form (:2074-2195): the per-point arithmetic with the four form bits, then the SEQUENTIAL loop with the claim
                              (vpMatched[idx] / mvpMapPoints[i2] written by an earlier iteration skips the keypoint)
  sim3_project / sim3_search / sim3_agree   ORBmatcher::SearchBySim3 (:1642-1859): one direction's arithmetic and search, and the agreement
  map_scene / sim3_scene      the seeded inputs of the tests, on top of ref_fuse.scene / ref_fuse.query_descriptors
  handmade_map / handmade_sim3   small cases whose answers are written out

Every fp32 expression is evaluated in np.float32 in the written order (numpy never contracts a multiply and an add).  The level is
ref_fuse.predict_level -- the reference's ceil / log expression, not the library's threshold table."""
import numpy as np

import ref_fuse as RU
import ref_projection as RP
import ref_window as RW

F = np.float32
D = np.float64
INACTIVE, BEHIND, OUT_OF_IMAGE, OUT_OF_RANGE, BAD_ANGLE, NO_CANDIDATES, REJECTED, MATCHED = range(8)
VISIBLE = NO_CANDIDATES
FOUND = MATCHED                                              # SearchBySim3's word for it; it has no BAD_ANGLE
CULL_BEHIND, CHECK_ANGLE, PROJECT_INVZ, BOUNDS_CLOSED = 1, 2, 4, 8
FORM_SIM3, FORM_SIM3_KF, FORM_RELOC = CULL_BEHIND | CHECK_ANGLE, CULL_BEHIND | CHECK_ANGLE | PROJECT_INVZ, BOUNDS_CLOSED
FORMS = dict(sim3=FORM_SIM3, sim3_kf=FORM_SIM3_KF, reloc=FORM_RELOC)
TH_LOW, TH_HIGH = 100, 1000
INT_MAX = 0x7fffffff


def rows(T, p):
    """row-major 3x4 times point, each row as ((m0*x + m1*y) + m2*z) + m3"""
    X, Y, Z = p
    return (((T[0] * X + T[1] * Y) + T[2] * Z) + T[3], ((T[4] * X + T[5] * Y) + T[6] * Z) + T[7], ((T[8] * X + T[9] * Y) + T[10] * Z) + T[11])


def map_project(T, Ow, cam, bounds, th, scale_factor, nlevels, form, xyz, normals, dist):
    """-> u, v, r (fp32 arrays), level (int32), status (BEHIND .. BAD_ANGLE or VISIBLE).  BEHIND: u = v = 0; every culled point has level -1, r = 0"""
    T = np.asarray(T, F).reshape(12); Ow = np.asarray(Ow, F).reshape(3)
    p = np.asarray(xyz, F).reshape(-1, 3); nr = np.asarray(normals, F).reshape(-1, 3); dd = np.asarray(dist, F).reshape(-1, 3)
    n = len(p)
    fx, fy, cx, cy = (F(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    mnx, mny, mxx, mxy = (F(b) for b in bounds)
    sf = RU.scale_factors(scale_factor, nlevels)
    u = np.zeros(n, F); v = np.zeros(n, F); r = np.zeros(n, F)
    level = np.full(n, -1, np.int32); st = np.zeros(n, np.uint8)
    with np.errstate(all="ignore"):
        for i in range(n):
            xc, yc, zc = rows(T, p[i])
            if (form & CULL_BEHIND) and zc < F(0):                                           # :646 / :754
                st[i] = BEHIND
                continue
            if form & PROJECT_INVZ:                                                          # :758-763
                invz = F(1) / zc
                x = xc * invz; y = yc * invz
                u[i] = fx * x + cx; v[i] = fy * y + cy
            else:                                                                            # Pinhole.cpp:45-46
                u[i] = (fx * xc) / zc + cx; v[i] = (fy * yc) / zc + cy
            if form & BOUNDS_CLOSED:                                                         # :2103-2106
                out = u[i] < mnx or u[i] > mxx or v[i] < mny or v[i] > mxy
            else:                                                                            # KeyFrame.cc:752
                out = not (u[i] >= mnx and u[i] < mxx and v[i] >= mny and v[i] < mxy)
            if out:
                st[i] = OUT_OF_IMAGE
                continue
            po = p[i] - Ow
            d3 = np.sqrt((po[0] * po[0] + po[1] * po[1]) + po[2] * po[2], dtype=F)
            if d3 < dd[i, 0] or d3 > dd[i, 1]:
                st[i] = OUT_OF_RANGE
                continue
            if form & CHECK_ANGLE:                                                           # :668 / :781
                dot = (po[0] * nr[i, 0] + po[1] * nr[i, 1]) + po[2] * nr[i, 2]
                if D(dot) < D(0.5) * D(d3):
                    st[i] = BAD_ANGLE
                    continue
            level[i] = RU.predict_level(dd[i, 2] / d3, scale_factor, nlevels)
            r[i] = F(th) * sf[level[i]]
            st[i] = VISIBLE
    return u, v, r, level, st


def map_search(O, status_in, level, u, v, r, qdesc, grid, x, y, bounds, tg, taken=None, init_dist=256, accept_max=100.0, claim=True):
    """the sequential loop.  status_in[q] == VISIBLE: the query reaches the search.  claim = False: the claim-free evaluation (no query
    sees another), which the scene conditions compare with.  redo[q]: the query had more than four candidates under the static filter
    and the four best of them by (distance, visiting position) were all claimed when its turn came."""
    nq, nt = len(qdesc), len(tg)
    x = np.asarray(x, F); y = np.asarray(y, F)
    taken0 = np.zeros(nt, bool) if taken is None else (np.asarray(taken) != 0)
    tk = taken0.copy()
    assigned = np.full(nt, -1, np.int32)
    status = np.asarray(status_in, np.uint8).copy()
    match = np.full(nq, -1, np.int32); best = np.full(nq, init_dist, np.int32)
    n_window = np.zeros(nq, np.int32); n_tested = np.zeros(nq, np.int32); redo = np.zeros(nq, bool)
    n_matches = 0
    for q in range(nq):
        if status[q] != VISIBLE:
            continue
        c = RW.features_in_area(grid, x, y, u[q], v[q], r[q], bounds)
        n_window[q] = len(c)
        if level[q] > 1:                                                                     # kpLevel = 0 (:694 / :807 / :2124)
            c = c[:0]
        cs = c[~taken0[c]]
        if len(cs) > 4:
            d = O.distance_i32(qdesc[q:q + 1], tg[cs])[0]
            redo[q] = bool(np.all(tk[cs[np.argsort(d, kind="stable")[:4]]]))
        c = c[~tk[c]]                                                                        # :689 / :802 / :2137
        n_tested[q] = len(c)
        bi = -1
        if len(c):
            bi, bd, _, _ = (int(a[0]) for a in O.best2_csr(qdesc[q:q + 1], tg, np.array([0, len(c)], np.int32), c, init_dist))
            best[q] = bd
        if bi >= 0 and F(best[q]) <= F(accept_max):                                          # :708 / :821 / :2151
            status[q] = MATCHED; match[q] = bi; assigned[bi] = q; n_matches += 1
            if claim:
                tk[bi] = True
        else:
            status[q] = NO_CANDIDATES if len(c) == 0 else REJECTED
    return dict(status=status, match_idx=match, best_dist=best, n_window=n_window, n_tested=n_tested, assigned=assigned, n_matches=n_matches, redo=redo)


def sim3_project(T, M, cam, bounds, th, scale_factor, nlevels, xyz, dist):
    """one direction of SearchBySim3 -> u, v, r (fp32), level (int32), status (BEHIND, OUT_OF_IMAGE, OUT_OF_RANGE or VISIBLE)"""
    T = np.asarray(T, F).reshape(12); M = np.asarray(M, F).reshape(12)
    p = np.asarray(xyz, F).reshape(-1, 3); dd = np.asarray(dist, F).reshape(-1, 3)
    n = len(p)
    fx, fy, cx, cy = (F(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    mnx, mny, mxx, mxy = (F(b) for b in bounds)
    sf = RU.scale_factors(scale_factor, nlevels)
    u = np.zeros(n, F); v = np.zeros(n, F); r = np.zeros(n, F)
    level = np.full(n, -1, np.int32); st = np.zeros(n, np.uint8)
    with np.errstate(all="ignore"):
        for i in range(n):
            p1 = rows(T, p[i])                                                               # :1692
            x2, y2, z2 = rows(M, p1)                                                         # :1693
            if z2 < F(0):                                                                    # :1696
                st[i] = BEHIND
                continue
            invz = F(D(1.0) / D(z2))                                                         # :1699
            x = x2 * invz; y = y2 * invz
            u[i] = fx * x + cx; v[i] = fy * y + cy                                           # :1703-1704
            if not (u[i] >= mnx and u[i] < mxx and v[i] >= mny and v[i] < mxy):              # :1707
                st[i] = OUT_OF_IMAGE
                continue
            d3 = np.sqrt((x2 * x2 + y2 * y2) + z2 * z2, dtype=F)                             # :1712
            if d3 < dd[i, 0] or d3 > dd[i, 1]:                                               # :1715
                st[i] = OUT_OF_RANGE
                continue
            level[i] = RU.predict_level(dd[i, 2] / d3, scale_factor, nlevels)
            r[i] = F(th) * sf[level[i]]
            st[i] = VISIBLE
    return u, v, r, level, st


def sim3_search(O, status_in, level, u, v, r, mp_desc, grid, x, y, bounds, tg, th_high=TH_HIGH):
    """one direction's loop over the queries (:1724-1757); no query sees another"""
    nq = len(mp_desc)
    x = np.asarray(x, F); y = np.asarray(y, F)
    status = np.asarray(status_in, np.uint8).copy()
    match = np.full(nq, -1, np.int32); best = np.full(nq, INT_MAX, np.int32)
    n_window = np.zeros(nq, np.int32); n_tested = np.zeros(nq, np.int32)
    for q in range(nq):
        if status[q] != VISIBLE:
            continue
        c = RW.features_in_area(grid, x, y, u[q], v[q], r[q], bounds)
        n_window[q] = len(c)
        if len(c) == 0:                                                                      # :1726
            status[q] = NO_CANDIDATES
            continue
        if level[q] > 1:                                                                     # :1740
            c = c[:0]
        n_tested[q] = len(c)
        bi = -1
        if len(c):
            bi, bd, _, _ = (int(a[0]) for a in O.best2_csr(mp_desc[q:q + 1], tg, np.array([0, len(c)], np.int32), c, INT_MAX))
            best[q] = bd
        if bi >= 0 and best[q] <= th_high:                                                   # :1754
            status[q] = FOUND; match[q] = bi
        else:
            status[q] = REJECTED
    return dict(status=status, match=match, best_dist=best, n_window=n_window, n_tested=n_tested)


def sim3_agree(match1, match2):
    """:1840-1856 -> match12, n_found"""
    m12 = np.full(len(match1), -1, np.int32)
    for i1, idx2 in enumerate(match1):
        if idx2 >= 0 and match2[idx2] == i1:
            m12[i1] = idx2
    return m12, int((m12 >= 0).sum())


def sim3_matrix(s, R, t):
    """the row-major 3x4 [s*R | t] of a Sim3, composed in float64 and rounded once"""
    return np.concatenate([D(s) * np.asarray(R, D).reshape(3, 3), np.asarray(t, D).reshape(3, 1)], 1).astype(F).reshape(12)


def sim3_inverse(s, R, t):
    """(s, R, t) of the inverse Sim3: (1/s, R^T, -R^T t / s)"""
    R = np.asarray(R, D).reshape(3, 3); t = np.asarray(t, D).reshape(3)
    return 1.0 / s, R.T, -(R.T @ t) / s


# ---- the seeded scenes ---------------------------------------------------------------------------------------------------------------
PILES, PILE = 2, 24                                          # queries piled on one spot, for the resolver's full re-search
PILE_R = F(4) * F(1.2)                                       # the radius of a level-1 query at th = 4: the smallest window a pile must fill
PILE_BIG = F(15) * F(1.2) - F(0.4)                           # ... and at th = 15, less a margin


def pile_spots(x, y, desc, O):
    """where the keyframe is densest: window centres (u, v) with the most keypoints inside PILE_R - 0.4, the closer their descriptors the
    better -> [(u, v, members, the keypoints whose rows the pile's descriptor is the mean of)], best first.  Candidates: a coarse lattice round every keypoint that has company."""
    x = np.asarray(x, F); y = np.asarray(y, F)
    rr = PILE_R - F(0.4)
    found = {}
    for k in range(len(x)):
        near = np.nonzero((np.abs(x - x[k]) < 2 * rr) & (np.abs(y - y[k]) < 2 * rr))[0]
        if len(near) < 3:
            continue
        for dx in (-3.0, -1.5, 0.0, 1.5, 3.0):
            for dy in (-3.0, -1.5, 0.0, 1.5, 3.0):
                u, v = F(x[k] + F(dx)), F(y[k] + F(dy))
                m = tuple(near[(np.abs(x[near] - u) < rr) & (np.abs(y[near] - v) < rr)].tolist())
                if len(m) >= 3 and m not in found:
                    found[m] = (float(u), float(v))
    spots = []
    desc = np.asarray(desc, F)
    for m, (u, v) in found.items():
        idx = np.array(m)
        if len(m) < 5:
            # too few for a truncated list at th = 4: the pile's descriptor then sits between the five rows nearest to the members' mean
            # inside the window of a level-1 query at th = 15, where the list does get truncated
            big = np.nonzero((np.abs(x - F(u)) < PILE_BIG) & (np.abs(y - F(v)) < PILE_BIG))[0]
            if len(big) < 5:
                continue
            for _ in range(2):
                c = desc[idx].astype(D).mean(0).astype(F)
                idx = big[np.argsort(O.distance_i32(c[None], desc[big])[0], kind="stable")[:5]]
        c = desc[idx].astype(D).mean(0).astype(F)
        spots.append((-min(len(m), 5), int(np.sort(O.distance_i32(c[None], desc[idx])[0])[:4].max()), u, v, m, tuple(idx.tolist())))
    spots.sort()
    return [(u, v, m, rows_) for _, _, u, v, m, rows_ in spots]


def map_scene(O, seed, xy_kf, desc_kf, cam, T, bounds, ratio_max, scale_factor=1.2, nlevels=8):
    """the map points of the map-projection tests, one per keypoint of the keyframe (nq = nt): ref_fuse.scene and ref_fuse.query_descriptors,
    then roughly a third of the queries are replaced by a near-duplicate of an EARLIER one -- position jittered by well under a pixel, the
    descriptor jittered (DescriptorDistance to the original about 10, for one in three 200 and more) -- so that two queries want the same
    keypoint and the order decides; every 37th is mirrored through the camera centre.
    The last PILES * PILE queries are piles: PILE queries on one of the keyframe's densest spots (pile_spots), all at level 1 and all
    with the same descriptor, the mean of the rows of the keypoints round the spot (jittered in the last places; it is not a unit
    vector, which a map point's descriptor need not be here).  They share one order of preference, so each takes the best keypoint the
    ones before it left, and from the fifth on a query finds its four best taken.  taken: about 8 % of the keypoints, none of them on
    a pile's spot.  O: the oracle module.  -> dict(xyz, normals, dist, flags, qdesc, taken, spots)"""
    x, y = np.asarray(xy_kf, F)[:, 0].copy(), np.asarray(xy_kf, F)[:, 1].copy()
    n = len(x)
    xyz, nr, dist, flags = RU.scene(seed, xy_kf, cam, T, ratio_max)
    Ow = RU.camera_centre(T)
    u, v = RU.project(T, Ow, cam, bounds, 3.0, scale_factor, nlevels, xyz, nr, dist)[:2]
    qd = RU.query_descriptors(seed, u, v, x, y, desc_kf, desc_kf)
    rng = np.random.RandomState(seed + 41)
    jit = lambda row, s: (lambda w: (w / np.linalg.norm(w)).astype(F))(np.asarray(row, D) + s * (rng.rand(64) - 0.5) * np.sqrt(12.0))
    npile = PILES * PILE
    for i in range(1, n - npile):
        if rng.rand() < 1 / 3:
            j = rng.randint(0, i)
            xyz[i] = xyz[j] + (rng.uniform(-0.001, 0.001, 3)).astype(F); nr[i] = nr[j]; dist[i] = dist[j]; flags[i] = flags[j]
            qd[i] = jit(qd[j], 0.1 if i % 3 == 0 else 0.017)                   # (one in three far enough to be rejected: 200 and more)
    Td = np.asarray(T, D).reshape(3, 4)
    for i in range(5, n - npile, 37):                                            # mirrored through the camera centre: behind, and for the
        pc = Td[:, :3] @ xyz[i].astype(D) + Td[:, 3]                             # relocalisation form, which has no depth test, where it was
        xyz[i] = (Td[:, :3].T @ (-pc - Td[:, 3])).astype(F)
    taken = (np.random.RandomState(seed + 43).rand(n) < 0.08).astype(np.uint8) * 5
    spots = []
    for su, sv, m, rows_ in pile_spots(x, y, desc_kf, O):
        if all(abs(su - a) > 40 or abs(sv - b_) > 40 for a, b_, _, _ in spots):
            spots.append((su, sv, m, rows_))
        if len(spots) == PILES:
            break
    for g, (su, sv, m, rows_) in enumerate(spots):
        # the point on the spot's ray at 2 m in the keyframe's camera, taken back to the world
        pc = np.array([(su - float(cam["cx"])) / float(cam["fx"]) * 2.0, (sv - float(cam["cy"])) / float(cam["fy"]) * 2.0, 2.0])
        pw = Td[:, :3].T @ (pc - Td[:, 3])
        mean = np.asarray(desc_kf, D)[list(rows_)].mean(0)
        taken[list(m)] = 0; taken[list(rows_)] = 0
        for j in range(PILE):
            i = n - npile + g * PILE + j
            xyz[i] = (pw + rng.uniform(-0.0001, 0.0001, 3)).astype(F)
            po = xyz[i] - Ow
            d3 = np.sqrt((po[0] * po[0] + po[1] * po[1]) + po[2] * po[2], dtype=F)
            nr[i] = po / d3; dist[i] = (F(0.5) * d3, F(2) * d3, F(1.1) * d3); flags[i] = 1
            qd[i] = (mean + 1e-4 * (rng.rand(64) - 0.5)).astype(F)
    return dict(xyz=xyz, normals=nr, dist=dist, flags=flags, qdesc=qd, taken=taken, spots=spots)


def sim3_pair(seed, cam, shift=(2, 1)):
    """the two poses and the Sim3 of the SearchBySim3 tests: T1w a small seeded pose, T2w = another (it moves a point at 2 m by `shift` pixels), S12 the transform from camera 2 to
    camera 1 that follows from them with a scale of 1.03 put on top (as a loop with scale drift would) -> T1w, T2w, M21, M12"""
    T1 = RP.pose(seed + 5, (0, 0), cam=cam); T2 = RP.pose(seed + 6, shift, cam=cam)
    A1 = np.vstack([np.asarray(T1, D).reshape(3, 4), [0, 0, 0, 1]]); A2 = np.vstack([np.asarray(T2, D).reshape(3, 4), [0, 0, 0, 1]])
    T12 = A1 @ np.linalg.inv(A2)
    s, R, t = 1.03, T12[:3, :3], T12[:3, 3] * 1.03
    si, Ri, ti = sim3_inverse(s, R, t)
    return T1, T2, sim3_matrix(si, Ri, ti), sim3_matrix(s, R, t)


def sim3_side(seed, xy, desc_own, xy_other, desc_other, cam, Tw, M, bounds, ratio_max, scale_factor=1.2, nlevels=8):
    """the map points one keyframe holds, one per keypoint: ref_fuse.scene for the positions, distances and flags (its normals are not
    used), with min / max distance re-centred on the CAMERA-frame norm in the other keyframe, which is what SearchBySim3 tests; the map
    point's own descriptor is the row of the other keyframe's keypoint it projects next to, jittered (ref_fuse.query_descriptors), else
    this keyframe's row.  -> dict(points, dist, mp_desc, flags)"""
    xyz, _, dist, flags = RU.scene(seed, xy, cam, Tw, ratio_max)
    u, v, _, _, _ = sim3_project(Tw, M, cam, bounds, 3.0, scale_factor, nlevels, xyz, np.tile(np.array([0, np.inf, 1], F), (len(xyz), 1)))
    with np.errstate(all="ignore"):
        d3 = np.array([np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2], dtype=F) for q in (rows(np.asarray(M, F), rows(np.asarray(Tw, F), p)) for p in xyz)], F)
    rng = np.random.RandomState(seed + 31)
    ratio = (dist[:, 2] / np.maximum(np.sqrt(((xyz - RU.camera_centre(Tw)) ** 2).sum(1)), F(1e-6))).astype(F)      # the spread of levels ref_fuse.scene chose
    pd = (ratio * d3).astype(F)
    lo = (F(0.8) * (pd * F(0.4))).astype(F); hi = (F(1.2) * pd).astype(F)
    far = rng.rand(len(xyz)) < 0.06
    hi[far] = (d3[far] * F(0.9)).astype(F)
    dist = np.stack([lo, hi, pd], 1).astype(F)
    xo, yo = np.asarray(xy_other, F)[:, 0].copy(), np.asarray(xy_other, F)[:, 1].copy()
    mp = RU.query_descriptors(seed, u, v, xo, yo, desc_other, desc_own)
    return dict(points=xyz, dist=dist, mp_desc=mp, flags=flags)


# ---- hand-made cases -------------------------------------------------------------------------------------------------------------------
def bits(h):
    return np.array([h], np.uint32).view(F)[0]


def tiny_map(cands, queries, form=FORM_SIM3, th=3.0, accept_max=100.0, taken=None, xyz=None, T=None):
    """cands: (x, y, descriptor value) per keypoint; queries: (u, v, descriptor value, ratio) -- the query sits at (u, v, 1) (or at xyz[q])
    with the normal along its viewing ray and predict_distance = ratio * dist3D; unit camera, identity pose, Ow = 0 -> one problem as a dict"""
    c = np.asarray(cands, D).reshape(-1, 3); q = np.asarray(queries, D).reshape(-1, 4)
    p = np.stack([q[:, 0], q[:, 1], np.ones(len(q))], 1).astype(F) if xyz is None else np.asarray(xyz, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        d3 = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2], dtype=F)
    dist = np.stack([np.zeros(len(q), F), np.full(len(q), np.inf, F), (q[:, 3].astype(F) * d3).astype(F)], 1)
    return dict(xyz=p, normals=p.copy(), dist=dist, qdesc=RU.line_descriptors(q[:, 2]), flags=np.ones(len(q), np.uint8), T=RU.I34 if T is None else T,
                Ow=np.zeros(3, F), cam=RU.UNIT_CAM, bounds=RU.B640, th=th, scale_factor=1.2, nlevels=8, x=c[:, 0].astype(F), y=c[:, 1].astype(F),
                tg=RU.line_descriptors(c[:, 2]), form=form, accept_max=F(accept_max), taken=None if taken is None else np.asarray(taken, np.uint8))


def run_map_case(O, k):
    u, v, r, level, st = map_project(k["T"], k["Ow"], k["cam"], k["bounds"], k["th"], k["scale_factor"], k["nlevels"], k["form"], k["xyz"], k["normals"], k["dist"])
    st = np.where(k["flags"] & 1, st, INACTIVE).astype(np.uint8)
    m = map_search(O, st, level, u, v, r, k["qdesc"], RW.build(k["x"], k["y"], k["bounds"]), k["x"], k["y"], k["bounds"], k["tg"], taken=k["taken"],
                   accept_max=k["accept_max"])
    act = (k["flags"] & 1) != 0
    m["level"] = np.where(act, level, -1).astype(np.int32)
    m["proj"] = np.where(act[:, None], np.stack([u, v, r], 1), F(0)).astype(F)
    m["proj_u"] = m["proj"][:, 0]
    return m


def handmade_map():
    """(name, inputs, expected) -- expected: dict of lists per output (proj_u: the exact floats of u)"""
    cases = []
    same = [(100, 100, 0.0, 1.0), (100, 100, 0.0, 1.0)]
    # the claim: both queries want keypoint 0 (distance 0); the second takes its runner-up (distance 5) ...
    k = tiny_map([(100, 100, 0.0), (101, 100, 0.1)], same)
    cases.append(("claim: runner-up", k, dict(status=[MATCHED, MATCHED], match_idx=[0, 1], best_dist=[0, 5], n_window=[2, 2], n_tested=[2, 1], assigned=[0, 1],
                                             n_matches=2, level=[0, 0])))
    # ... or is rejected when the runner-up is too far (distance 128 > 100)
    k = tiny_map([(100, 100, 0.0), (101, 100, 0.5)], same)
    cases.append(("claim: rejected", k, dict(status=[MATCHED, REJECTED], match_idx=[0, -1], best_dist=[0, 128], n_window=[2, 2], n_tested=[2, 1], assigned=[0, -1],
                                            n_matches=1, level=[0, 0])))
    # a keypoint taken at entry is skipped; a window whose members are all taken tests nothing
    k = tiny_map([(100, 100, 0.0), (101, 100, 0.1), (200, 200, 0.0)], [(100, 100, 0.0, 1.0), (200, 200, 0.0, 1.0)], taken=[1, 0, 9])
    cases.append(("taken at entry", k, dict(status=[MATCHED, NO_CANDIDATES], match_idx=[1, -1], best_dist=[5, 256], n_window=[2, 1], n_tested=[1, 0],
                                           assigned=[-1, 0, -1], n_matches=1, level=[0, 0])))
    # accept_max = 100.0f * 1.0f: a best of 100 is in, 101 is out
    two = [(100, 100, 0.0, 1.0), (200, 100, 0.0, 1.0)]
    k = tiny_map([(100, 100, 0.4425), (200, 100, 0.4445)], two, accept_max=F(100) * F(1.0))
    cases.append(("accept 100 / 101", k, dict(status=[MATCHED, REJECTED], match_idx=[0, -1], best_dist=[100, 101], n_tested=[1, 1], assigned=[0, -1], n_matches=1)))
    # ratioHamming = 0.455: accept_max = 45.5, no integer: 45 is in, 46 is out
    k = tiny_map([(100, 100, 0.2975), (200, 100, 0.3)], two, accept_max=F(100) * F(0.455))
    cases.append(("accept 45.5", k, dict(status=[MATCHED, REJECTED], match_idx=[0, -1], best_dist=[45, 46], n_tested=[1, 1], assigned=[0, -1], n_matches=1)))
    # levels: 1 widens the radius to 1.2f * th (x = 103.5 is inside 3.6, outside 3); 2 and above count the window and test nothing
    k = tiny_map([(103.5, 100, 0.0)], [(100, 100, 0.0, 1.0), (100, 100, 0.0, 1.3), (100, 100, 0.0, 100.0), (100, 100, 0.0, 1.1)])
    cases.append(("levels 0 2 7 1", k, dict(status=[NO_CANDIDATES, NO_CANDIDATES, NO_CANDIDATES, MATCHED], match_idx=[-1, -1, -1, 0], best_dist=[256, 256, 256, 0],
                                           n_window=[0, 1, 1, 1], n_tested=[0, 0, 0, 1], level=[0, 2, 7, 1], assigned=[3], n_matches=1)))
    # the two projections on (5, 300, 3): 5.0f / 3.0f = 0x3fd55555, 5.0f * (1.0f / 3.0f) = 0x3fd55556
    p53 = [(5, 300, 3)]
    for form, h in ((FORM_SIM3, 0x3fd55555), (FORM_SIM3_KF, 0x3fd55556), (FORM_RELOC, 0x3fd55555), (FORM_RELOC | PROJECT_INVZ, 0x3fd55556)):
        k = tiny_map([(2, 100, 0.0)], [(0, 0, 0.0, 1.0)], form=form, xyz=p53)
        cases.append((f"projection, form {form}", k, dict(status=[MATCHED], match_idx=[0], proj_u=[bits(h)], n_window=[1], level=[0])))
    # u = max_x exactly: outside the half-open IsInImage, inside the closed bounds of the relocalisation form (th = 7: the keypoint at x = 634 is binned)
    for form, st, mi in ((FORM_SIM3, OUT_OF_IMAGE, -1), (FORM_SIM3_KF, OUT_OF_IMAGE, -1), (FORM_RELOC, MATCHED, 0)):
        k = tiny_map([(634, 100, 0.0)], [(640, 100, 0.0, 1.0)], form=form, th=7.0)
        cases.append((f"u on max_x, form {form}", k, dict(status=[st], match_idx=[mi], proj_u=[F(640)], level=[0 if mi == 0 else -1])))
    # zc = -0.0 is not behind (u = +Inf: out of every image); a NaN is out of IsInImage but PASSES the closed bounds, and then opens no
    # window; zc = -1 is behind in the Sim3 forms, and the relocalisation form, which has no depth test, matches it at (100, 100)
    T0 = RU.I34.copy(); T0[11] = -0.0
    odd = [(-100, -100, -0.0), (100, 100, np.nan), (-100, -100, -1)]
    k = tiny_map([(100, 100, 0.0)], [(0, 0, 0.0, 1.0)] * 3, form=FORM_SIM3, xyz=odd, T=T0)
    cases.append(("zc -0 / NaN / -1, sim3", k, dict(status=[OUT_OF_IMAGE, OUT_OF_IMAGE, BEHIND], match_idx=[-1, -1, -1], level=[-1, -1, -1], n_matches=0)))
    k = tiny_map([(100, 100, 0.0)], [(0, 0, 0.0, 1.0)] * 3, form=FORM_RELOC, xyz=odd, T=T0)
    cases.append(("zc -0 / NaN / -1, reloc", k, dict(status=[OUT_OF_IMAGE, NO_CANDIDATES, MATCHED], match_idx=[-1, -1, 0], level=[-1, 0, 0], n_window=[0, 0, 1],
                                                    n_matches=1)))
    return cases


def tiny_sim3(side1, side2, M21=None, M12=None, th=3.0):
    """side: (x, y, keyframe descriptor value, map point u, map point v, map point descriptor value, min_distance, max_distance, active) per
    keypoint: the keypoint at (x, y) holds a map point at (u, v, 1); unit camera, identity poses, level 0 -> the inputs as a dict"""
    def side(rows_):
        a = np.asarray(rows_, D).reshape(-1, 9)
        p = np.stack([a[:, 3], a[:, 4], np.ones(len(a))], 1).astype(F)
        return dict(x=a[:, 0].astype(F), y=a[:, 1].astype(F), desc=RU.line_descriptors(a[:, 2]), points=p, mp_desc=RU.line_descriptors(a[:, 5]),
                    dist=np.stack([a[:, 6], a[:, 7], np.full(len(a), 1e-3)], 1).astype(F), flags=a[:, 8].astype(np.uint8), Tw=RU.I34)
    return dict(s1=side(side1), s2=side(side2), M21=RU.I34 if M21 is None else np.asarray(M21, F), M12=RU.I34 if M12 is None else np.asarray(M12, F),
                cam=RU.UNIT_CAM, bounds=RU.B640, th=th, scale_factor=1.2, nlevels=8)


def run_sim3_case(O, k, th_high=TH_HIGH):
    r = {}
    for q, g, M, s in ((k["s1"], k["s2"], k["M21"], "1"), (k["s2"], k["s1"], k["M12"], "2")):
        u, v, rr, level, st = sim3_project(q["Tw"], M, k["cam"], k["bounds"], k["th"], k["scale_factor"], k["nlevels"], q["points"], q["dist"])
        st = np.where(q["flags"] & 1, st, INACTIVE).astype(np.uint8)
        m = sim3_search(O, st, level, u, v, rr, q["mp_desc"], RW.build(g["x"], g["y"], k["bounds"]), g["x"], g["y"], k["bounds"], g["desc"], th_high)
        act = (q["flags"] & 1) != 0
        m["level"] = np.where(act, level, -1).astype(np.int32)
        m["proj"] = np.where(act[:, None], np.stack([u, v, rr], 1), F(0)).astype(F)
        r.update({name + s: val for name, val in m.items()})
    r["match12"], r["n_found"] = sim3_agree(r["match1"], r["match2"])
    return r


def handmade_sim3():
    """(name, inputs, expected)"""
    cases = []
    inf = np.inf
    # both directions name each other: idx2 = 0 is a match like any other
    k = tiny_sim3([(100, 100, 0.0, 100, 100, 0.0, 0, inf, 1)], [(100, 100, 0.0, 100, 100, 0.0, 0, inf, 1)])
    cases.append(("mutual, idx2 = 0", k, dict(status1=[FOUND], status2=[FOUND], match1=[0], match2=[0], best_dist1=[0], match12=[0], n_found=1)))
    # one-sided: keypoint 0 of side 1 finds keypoint 0 of side 2, whose map point prefers keypoint 1 of side 1 (distance 0 against 46)
    k = tiny_sim3([(100, 100, 0.3, 100, 100, 0.0, 0, inf, 1), (101, 100, 0.0, 101, 100, 0.0, 0, inf, 0)], [(100, 100, 0.0, 100, 100, 0.0, 0, inf, 1)])
    cases.append(("one-sided", k, dict(status1=[FOUND, INACTIVE], status2=[FOUND], match1=[0, -1], match2=[1], best_dist2=[0], n_window2=[2], match12=[-1, -1],
                                      n_found=0)))
    # two equal rows on side 2: slot 1 lies in grid column 9 (x = 94.5), slot 0 in column 10 (x = 95.5): slot 1 is visited first and keeps the tie
    k = tiny_sim3([(95, 100, 0.0, 95, 100, 0.0, 0, inf, 1)], [(95.5, 100, 0.1, 0, 0, 0.0, 0, inf, 0), (94.5, 100, 0.1, 0, 0, 0.0, 0, inf, 0)])
    cases.append(("tie goes to the first visited", k, dict(status1=[FOUND], match1=[1], best_dist1=[5], n_window1=[2], n_tested1=[2], match2=[-1, -1],
                                                          match12=[-1], n_found=0)))
    # S21 with scale 2: p2 = (200, 200, 2), projected to (100, 100) as before, |p2| = 282.85 while |X - Ow| = 141.4.  A range of [0, 200]
    # holds the world distance and not the camera-frame norm: out of range; [200, 300] the other way round: found
    M2 = np.array([2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 0], F); Mh = np.array([.5, 0, 0, 0, 0, .5, 0, 0, 0, 0, .5, 0], F)
    k = tiny_sim3([(100, 100, 0.0, 100, 100, 0.0, 0, 200, 1), (100, 101, 0.0, 100, 100, 0.0, 200, 300, 1)], [(100, 100, 0.0, 0, 0, 0.0, 0, inf, 0)], M21=M2, M12=Mh)
    cases.append(("camera-frame norm", k, dict(status1=[OUT_OF_RANGE, FOUND], match1=[-1, 0], level1=[-1, 0], match12=[-1, -1], n_found=0)))
    # TH_HIGH: a best of 1000 is in, 1001 is out (descriptor values 1.3976 and 1.3983)
    k = tiny_sim3([(100, 100, 0.0, 100, 100, 1.3976, 0, inf, 1), (200, 100, 0.0, 200, 100, 1.3983, 0, inf, 1)],
                  [(100, 100, 0.0, 0, 0, 0.0, 0, inf, 0), (200, 100, 0.0, 0, 0, 0.0, 0, inf, 0)])
    cases.append(("best 1000 / 1001", k, dict(status1=[FOUND, REJECTED], match1=[0, -1], best_dist1=[1000, 1001], match12=[-1, -1], n_found=0)))
    return cases
