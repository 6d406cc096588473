"""Restatement of ORBmatcher::SearchForTriangulation (reference src/ORBmatcher.cc:1092-1331, mbCheckOrientation = false, no second camera)
with Pinhole::epipolarConstrain (src/CameraModels/Pinhole.cpp:107-129) on the caller's F12, in two forms:

  literal()     the loop of :1148-1297 transcribed: the two map iterators with lower_bound, the carried bestDist, and the `continue`s in the
                reference's order (DescriptorDistance BEFORE the geometry), every float operation a numpy fp32 scalar operation
  order_free()  the contract of xfh_triangulation_search_device: per query the least distance over the members that pass every gate, the
                member visited last winning a tie, with the statuses and the two counts

`dist` is the n1 x n2 table of DescriptorDistance (the C oracle's distance_i32).  No test lives here."""
import bisect

import numpy as np

F = np.float32
NONE = 0xFFFFFFFF
INACTIVE, NO_NODE, NO_CANDIDATES, REJECTED, MATCHED = range(5)
SKIPPED, GATE_REJECTED, PASSED = range(3)
ONLY_STEREO, COARSE = 1, 2
TH_LOW = 100
OUT = ("status", "match12", "best_dist", "n_candidates", "n_geom")


def feature_vector(node_of):
    """mFeatVec as TemplatedVocabulary::transform builds it: features in ascending index, addFeature push_backs; std::map orders the ids"""
    fv = {}
    for i, nd in enumerate(np.asarray(node_of, np.uint32).tolist()):
        if nd != NONE:
            fv.setdefault(nd, []).append(i)
    return dict(sorted(fv.items()))


def line(Fm, x1, y1):
    """a, b, c, den of Pinhole.cpp:115-121; F12(r, c) = Fm[3r + c]"""
    Fm = np.asarray(Fm, F).reshape(9)
    x1, y1 = F(x1), F(y1)
    with np.errstate(all="ignore"):
        a = F(F(x1 * Fm[0]) + F(y1 * Fm[3])) + Fm[6]
        b = F(F(x1 * Fm[1]) + F(y1 * Fm[4])) + Fm[7]
        c = F(F(x1 * Fm[2]) + F(y1 * Fm[5])) + Fm[8]
        den = F(a * a) + F(b * b)
    return F(a), F(b), F(c), F(den)


def near_epipole(ep, r2, x2, y2):
    """:1213-1215: distex*distex + distey*distey < 100 * mvScaleFactors[0]"""
    with np.errstate(all="ignore"):
        dx, dy = F(F(ep[0]) - F(x2)), F(F(ep[1]) - F(y2))
        return bool(F(F(dx * dx) + F(dy * dy)) < F(r2))


def epipolar_ok(l, unc, x2, y2):
    """Pinhole.cpp:119-128"""
    a, b, c, den = l
    with np.errstate(all="ignore"):
        num = F(F(F(a * F(x2)) + F(b * F(y2))) + c)
        if den == 0:
            return False
        dsqr = F(F(num * num) / den)
        return bool(float(dsqr) < 3.84 * float(F(unc)))


def stereo(ur, k):
    return ur is not None and bool(ur[k] >= 0)


def member(l, ep, r2, unc, flags, stereo1, x2, y2, stereo2):
    """one member of KF2's node without a map point -> SKIPPED / GATE_REJECTED / PASSED (xfh_epipolar_gate)"""
    if (flags & ONLY_STEREO) and not stereo2:
        return SKIPPED
    if not stereo1 and not stereo2 and near_epipole(ep, r2, x2, y2):
        return GATE_REJECTED
    if not (flags & COARSE) and not epipolar_ok(l, unc, x2, y2):
        return GATE_REJECTED
    return PASSED


def literal(dist, k1, k2, Fm, ep, flags=0, th_low=TH_LOW, r2=100.0, unc=1.0):
    """k1 / k2: dict(node_of, xy, ur (or None), has).  -> dict(match12, best_dist, n_candidates, n_matches, pairs)"""
    fv1, fv2 = feature_vector(k1["node_of"]), feature_vector(k2["node_of"])
    key1, key2 = list(fv1), list(fv2)
    n1 = len(k1["node_of"])
    vMatches12 = np.full(n1, -1, np.int32); best = np.full(n1, th_low, np.int32); ncand = np.zeros(n1, np.int32)
    nmatches = 0
    bOnlyStereo, bCoarse = bool(flags & ONLY_STEREO), bool(flags & COARSE)
    f1, f2 = 0, 0
    while f1 != len(key1) and f2 != len(key2):
        if key1[f1] == key2[f2]:
            for idx1 in fv1[key1[f1]]:
                if k1["has"][idx1]:
                    continue
                bStereo1 = stereo(k1["ur"], idx1)
                if bOnlyStereo and not bStereo1:
                    continue
                l = line(Fm, k1["xy"][idx1, 0], k1["xy"][idx1, 1])          # (the reference recomputes F12 and the line per candidate: same values)
                bestDist, bestIdx2 = th_low, -1
                for idx2 in fv2[key2[f2]]:
                    if k2["has"][idx2]:
                        continue
                    bStereo2 = stereo(k2["ur"], idx2)
                    if bOnlyStereo and not bStereo2:
                        continue
                    ncand[idx1] += 1
                    d = int(dist[idx1, idx2])
                    if d > th_low or d > bestDist:
                        continue
                    x2, y2 = k2["xy"][idx2]
                    if not bStereo1 and not bStereo2 and near_epipole(ep, r2, x2, y2):
                        continue
                    if bCoarse or epipolar_ok(l, unc, x2, y2):
                        bestIdx2, bestDist = idx2, d
                if bestIdx2 >= 0:
                    vMatches12[idx1] = bestIdx2; best[idx1] = bestDist
                    nmatches += 1
            f1 += 1; f2 += 1
        elif key1[f1] < key2[f2]:
            f1 = bisect.bisect_left(key1, key2[f2])
        else:
            f2 = bisect.bisect_left(key2, key1[f1])
    pairs = [(i, int(vMatches12[i])) for i in range(n1) if vMatches12[i] >= 0]
    return dict(match12=vMatches12, best_dist=best, n_candidates=ncand, n_matches=nmatches, pairs=pairs)


def order_free(dist, k1, k2, Fm, ep, flags=0, th_low=TH_LOW, r2=100.0, unc=1.0, stats=None):
    """the contract of include/xfeat_hip.h.  stats (a dict): counts of what the scene is chosen for are added to it"""
    fv2 = feature_vector(k2["node_of"])
    n1 = len(k1["node_of"])
    o = dict(status=np.zeros(n1, np.uint8), match12=np.full(n1, -1, np.int32), best_dist=np.full(n1, th_low, np.int32), n_candidates=np.zeros(n1, np.int32),
             n_geom=np.zeros(n1, np.int32))
    for i in range(n1):
        if k1["has"][i]:
            continue
        s1 = stereo(k1["ur"], i)
        if (flags & ONLY_STEREO) and not s1:
            continue
        nd = int(k1["node_of"][i])
        if nd == NONE or nd not in fv2:
            o["status"][i] = NO_NODE
            continue
        l = line(Fm, k1["xy"][i, 0], k1["xy"][i, 1])
        best, bi, passing = th_low, -1, []
        for k in fv2[nd]:
            if k2["has"][k]:
                continue
            s2 = stereo(k2["ur"], k)
            x2, y2 = k2["xy"][k]
            g = member(l, ep, r2, unc, flags, s1, x2, y2, s2)
            if g == SKIPPED:
                continue
            o["n_candidates"][i] += 1
            if stats is not None and near_epipole(ep, r2, x2, y2):
                stats["epipole_mono" if not s1 and not s2 else "epipole_stereo"] += 1
            if g != PASSED:
                if stats is not None and int(dist[i, k]) <= th_low:
                    passing.append((int(dist[i, k]), k, False))
                continue
            o["n_geom"][i] += 1
            d = int(dist[i, k])
            passing.append((d, k, True))
            if d <= th_low and d <= best:
                best, bi = d, k
        if bi >= 0:
            o["status"][i] = MATCHED; o["match12"][i] = bi; o["best_dist"][i] = best
        else:
            o["status"][i] = NO_CANDIDATES if o["n_candidates"][i] == 0 else REJECTED
        if stats is not None and bi >= 0:
            ties = [k for d, k, ok in passing if ok and d == best]
            if len(ties) > 1 and bi == max(ties):
                stats["tie_last_wins"] += 1
            if any(not ok and d < best for d, k, ok in passing):
                stats["nearest_fails_gate"] += 1
    o["n_matches"] = int((o["status"] == MATCHED).sum())
    return o


def new_stats():
    return dict(epipole_mono=0, epipole_stereo=0, tie_last_wins=0, nearest_fails_gate=0)


# x1 = R12 x2 + t12 with R12 = I, t12 = (1, 0, 0), K = I: the epipolar line of (x1, y1) is y2 = y1 and dsqr = (y2 - y1)^2
F_X = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], F)


def handmade():
    """-> (name, dist, k1, k2, F12, ep, flags, want) with the answers written out"""
    kf = lambda node, xy, ur, has: dict(node_of=np.array(node, np.uint32), xy=np.array(xy, F).reshape(-1, 2), ur=None if ur is None else np.array(ur, F),
                                        has=np.array(has, np.uint8))
    N = NONE
    far = np.array([1e4, 1e4], F)
    c = []
    # one node; members 0 and 2 on the line at equal distance (the LATER wins), member 1 nearer but 3 px off the line, member 3 has a map point
    k1 = kf([5], [[10, 20]], None, [0]); k2 = kf([5, 5, 5, 5], [[0, 20], [0, 23], [50, 20.5], [0, 20]], None, [0, 0, 0, 1])
    c.append(("tie: last wins", np.array([[40, 10, 40, 0]]), k1, k2, F_X, far, 0, dict(status=[MATCHED], match12=[2], best_dist=[40], n_candidates=[3], n_geom=[2])))
    c.append(("coarse: the nearest", np.array([[40, 10, 40, 0]]), k1, k2, F_X, far, COARSE, dict(status=[MATCHED], match12=[1], best_dist=[10], n_candidates=[3], n_geom=[3])))
    c.append(("dist == th_low passes, th_low + 1 does not", np.array([[100, 10, 101, 0]]), k1, k2, F_X, far, 0,
              dict(status=[MATCHED], match12=[0], best_dist=[100], n_candidates=[3], n_geom=[2])))
    c.append(("all too far", np.array([[101, 10, 900, 0]]), k1, k2, F_X, far, 0, dict(status=[REJECTED], match12=[-1], best_dist=[100], n_candidates=[3], n_geom=[2])))
    # statuses: a map point, no node, a node KF2 lacks, a node whose only member has a map point; ids above 2^31 compare unsigned
    k1 = kf([5, N, 7, 0x80000001, 9], [[1, 2]] * 5, None, [1, 0, 0, 0, 0]); k2 = kf([9, 5, 0x80000001, N], [[3, 2]] * 4, None, [1, 0, 0, 0])
    c.append(("statuses", np.full((5, 4), 30), k1, k2, F_X, far, 0,
              dict(status=[INACTIVE, NO_NODE, NO_NODE, MATCHED, NO_CANDIDATES], match12=[-1, -1, -1, 2, -1], best_dist=[100, 100, 100, 30, 100],
                   n_candidates=[0, 0, 0, 1, 0], n_geom=[0, 0, 0, 1, 0])))
    # stereo: uright = -1, 0, NaN on both sides under bOnlyStereo, and the epipole radius applies to mono-mono pairs only
    k1 = kf([1, 1, 1], [[0, 5]] * 3, [-1, 0, np.nan], [0, 0, 0]); k2 = kf([1, 1, 1], [[100, 5], [101, 5], [102, 5]], [-1, 0, np.nan], [0, 0, 0])
    ep = np.array([101, 5], F)
    c.append(("only stereo", np.array([[9, 8, 7]] * 3), k1, k2, F_X, far, ONLY_STEREO,
              dict(status=[INACTIVE, MATCHED, INACTIVE], match12=[-1, 1, -1], best_dist=[100, 8, 100], n_candidates=[0, 1, 0], n_geom=[0, 1, 0])))
    c.append(("epipole", np.array([[9, 8, 7]] * 3), k1, k2, F_X, ep, 0,
              dict(status=[MATCHED, MATCHED, MATCHED], match12=[1, 2, 1], best_dist=[8, 7, 8], n_candidates=[3, 3, 3], n_geom=[1, 3, 1])))
    return c
