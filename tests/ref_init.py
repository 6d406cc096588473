"""Restatement of ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:833-948) as include/xfeat_hip.h states it (test infrastructure, no
GPU; shares no code with the library), in two forms:

  literal     the sequential loop transcribed line by line on tests/ref_window.py's grid and the oracle's DescriptorDistance: vMatchedDistance,
              vnMatches21, the retraction (:891-895), the update of vbPrevMatched (:943-945)
  order_free  the rule the device resolves: member (k, d) of query q is skipped iff d == INT_MAX or some accepting j < q with claim[j] == k
              has dist[j] <= d; all queries re-evaluated against the previous round's (claim, dist) until a round changes none.  Returns
              the same outputs and the number of rounds that changed something (`depth`)
  plant       the seeded variants the sequential order exists for, written into copies of both frames' rows and the window centres
  conditions  what a scene must show (counted on the literal form alone)

DescriptorDistance is the oracle's where the fp32 squared norm is below 2^31 / 512 and INT_MAX otherwise (Inf, NaN), as the header says.
"""
import numpy as np

import ref_window as RW

F = np.float32
NONE = 0x7fffffff
INACTIVE, NO_CANDIDATES, REJECTED, MATCHED = range(4)
TH_LOW = 100
DEPTH_MIN = 3                                                         # rounds that change something, at the least, on a seeded scene (tests/test_init_ref.py asserts it)


def distances(O, qrow, tg, c):
    """DescriptorDistance of one query row to the rows tg[c] -> python ints"""
    if len(c) == 0:
        return []
    rows = np.ascontiguousarray(tg[c], F)
    d = O.distance_i32(np.ascontiguousarray(qrow, F).reshape(1, 64), rows)[0].astype(np.int64)
    with np.errstate(all="ignore"):
        nd = ((np.asarray(qrow, F)[None, :] - rows).astype(np.float64) ** 2).sum(1).astype(F)
    d[~(nd < F(4194304.0))] = NONE
    return d.tolist()


def accept(best, second, th_low, nn_ratio):
    """:887-889 in fp32: bestDist <= TH_LOW && bestDist < (float)bestDist2 * mfNNratio (best == INT_MAX: nothing was tested)"""
    return best != NONE and best <= th_low and bool(F(best) < F(second) * F(nn_ratio))


def best2(ds, cs, blocked):
    """:875-884 over the members that are not blocked, in visiting order -> best, second, best_idx, n_tested"""
    best = second = NONE
    bi = -1
    n = 0
    for d, k, b in zip(ds, cs, blocked):
        if b:
            continue
        n += 1
        if d < best:
            second = best; best = d; bi = k
        elif d < second:
            second = d
    return best, second, bi, n


def _members(O, qdesc, prev, window, grid, x, y, bounds, tg, flags):
    """per active query: (member indices in visiting order, their distances); None for an inactive query"""
    out = []
    for q in range(len(qdesc)):
        if flags is not None and not (int(flags[q]) & 1):
            out.append(None)
            continue
        c = RW.features_in_area(grid, x, y, prev[q][0], prev[q][1], window, bounds)
        out.append((c.tolist(), distances(O, qdesc[q], tg, c)))
    return out


def _outputs(nq, nt):
    return dict(status=np.zeros(nq, np.uint8), claim_idx=np.full(nq, -1, np.int32), matches12=np.full(nq, -1, np.int32), best_dist=np.full(nq, NONE, np.int32),
                second_dist=np.full(nq, NONE, np.int32), n_window=np.zeros(nq, np.int32), n_tested=np.zeros(nq, np.int32),
                matches21=np.full(nt, -1, np.int32), matched_distance=np.full(nt, NONE, np.int32), n_matches=0)


def _prev_out(o, prev, txy):
    po = np.array(prev, F).reshape(-1, 2).copy()
    if txy is not None:
        m = o["matches12"]
        po[m >= 0] = np.asarray(txy, F).reshape(-1, 2)[m[m >= 0]]
    o["prev_out"] = po


def literal(O, qdesc, prev, window, grid, x, y, bounds, tg, flags=None, th_low=TH_LOW, nn_ratio=0.9, txy=None, blocking=True, members=None):
    """the loop of :833-948.  blocking = False: the same search with line :872 taken out (what every query would answer alone).  Besides the
    contract's outputs: retractions, blocked_ahead[q] (blocked members before q's answer in (distance, visiting position) order; all blocked
    members where q has no answer), flips[q] (q accepted, and with nothing blocked it has the same best but fails the ratio test)"""
    nq, nt = len(qdesc), len(tg)
    prev = np.asarray(prev, F).reshape(-1, 2)
    mem = members if members is not None else _members(O, qdesc, prev, F(window), grid, x, y, bounds, tg, flags)
    o = _outputs(nq, nt)
    md = [NONE] * nt
    m21 = [-1] * nt
    m12 = [-1] * nq
    nmatches = retractions = 0
    ahead = np.zeros(nq, np.int32); flips = np.zeros(nq, bool)
    for q in range(nq):
        if mem[q] is None:
            o["status"][q] = INACTIVE
            continue
        cs, ds = mem[q]
        o["n_window"][q] = len(cs)
        if not cs:
            o["status"][q] = NO_CANDIDATES
            continue
        blocked = [blocking and md[k] <= d for k, d in zip(cs, ds)] if blocking else [d == NONE for d in ds]
        best, second, bi, n = best2(ds, cs, blocked)
        o["best_dist"][q] = best; o["second_dist"][q] = second; o["n_tested"][q] = n
        key = (best, cs.index(bi)) if bi >= 0 else (NONE, 0)
        ahead[q] = sum(1 for p, (d, b) in enumerate(zip(ds, blocked)) if b and d != NONE and (d, p) < key)
        if not accept(best, second, th_low, nn_ratio):
            o["status"][q] = REJECTED
            continue
        fb, fs, fi, _ = best2(ds, cs, [d == NONE for d in ds])
        flips[q] = fi == bi and not accept(fb, fs, th_low, nn_ratio)
        o["status"][q] = MATCHED; o["claim_idx"][q] = bi
        if blocking:
            if m21[bi] >= 0:
                m12[m21[bi]] = -1
                nmatches -= 1; retractions += 1
            md[bi] = best
        m12[q] = bi; m21[bi] = q
        nmatches += 1
    o["matches12"][:] = m12; o["matches21"][:] = m21; o["matched_distance"][:] = md; o["n_matches"] = nmatches
    _prev_out(o, prev, txy)
    o.update(retractions=retractions, blocked_ahead=ahead, flips=flips, members=mem)
    return o


def order_free(O, qdesc, prev, window, grid, x, y, bounds, tg, flags=None, th_low=TH_LOW, nn_ratio=0.9, txy=None, members=None):
    """the order-free rule iterated to its fixed point -> the contract's outputs and `depth`, the number of rounds that changed something"""
    nq, nt = len(qdesc), len(tg)
    prev = np.asarray(prev, F).reshape(-1, 2)
    mem = members if members is not None else _members(O, qdesc, prev, F(window), grid, x, y, bounds, tg, flags)
    claim = [-1] * nq
    dist = [NONE] * nq
    res = [None] * nq
    depth = 0
    lo = 0
    while True:
        pc, pd = list(claim), list(dist)                              # the previous round's state
        # least distance among the acceptors j < q of every keypoint, grown as q advances: "exists j < q with dist[j] <= d" is `least[k] <= d`
        least = [NONE] * nt
        for j in range(lo):
            if pc[j] >= 0 and pd[j] < least[pc[j]]:
                least[pc[j]] = pd[j]
        changed = None
        for q in range(lo, nq):
            if mem[q] is not None and mem[q][0]:
                cs, ds = mem[q]
                blocked = [d == NONE or least[k] <= d for k, d in zip(cs, ds)]
                best, second, bi, n = best2(ds, cs, blocked)
                acc = accept(best, second, th_low, nn_ratio)
                res[q] = (best, second, bi, n, acc)
                c, d = (bi, best) if acc else (-1, NONE)
                if (c, d) != (claim[q], dist[q]):
                    claim[q], dist[q] = c, d
                    if changed is None:
                        changed = q
            if pc[q] >= 0 and pd[q] < least[pc[q]]:
                least[pc[q]] = pd[q]
        if changed is None:
            break
        depth += 1
        lo = changed + 1                                              # every query up to the smallest one that moved is final
    o = _outputs(nq, nt)
    for q in range(nq):
        if mem[q] is None:
            o["status"][q] = INACTIVE
            continue
        o["n_window"][q] = len(mem[q][0])
        if not mem[q][0]:
            o["status"][q] = NO_CANDIDATES
            continue
        best, second, bi, n, acc = res[q]
        o["best_dist"][q] = best; o["second_dist"][q] = second; o["n_tested"][q] = n
        o["status"][q] = MATCHED if acc else REJECTED
        if acc:
            o["claim_idx"][q] = bi
            o["matches21"][bi] = q                                    # ascending q: the largest acceptor stays
            o["matched_distance"][bi] = best
    for q in range(nq):
        k = o["claim_idx"][q]
        if k >= 0 and o["matches21"][k] == q:
            o["matches12"][q] = k
    o["n_matches"] = int((o["matches21"] >= 0).sum())
    _prev_out(o, prev, txy)
    o["depth"] = depth
    return o


OUT_KEYS = ("status", "claim_idx", "matches12", "best_dist", "second_dist", "n_window", "n_tested", "matches21", "matched_distance", "n_matches")


def same(a, b, keys=OUT_KEYS + ("prev_out",)):
    """the names of the outputs in which two results differ (floats by their bits)"""
    bad = []
    for k in keys:
        x, y = a[k], b[k]
        if np.isscalar(x) or np.isscalar(y):
            ok = int(x) == int(y)
        else:
            ok = np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()
        if not ok:
            bad.append(k)
    return bad


# ---- the seeded variants -----------------------------------------------------------------------------------------------------------------
def _axis(j, s):
    e = np.zeros(64, F); e[j] = s
    return e


def _step(d512):
    """the offset along one axis that is `d512` units of DescriptorDistance away (plus a quarter unit against the truncation)"""
    return float(np.sqrt((d512 + 0.25) / 512.0))


def plant(seed, xy1, d1, xy2, d2, K):
    """-> (query rows, window centres, target rows): copies of F1's rows, of prev_matched = F1's keypoints (Tracking.cc:2486-2488) and of F2's
    rows with seeded correspondences and five seeded structures written in.  Each sits on a cluster of F2 keypoints that are neighbours in the image, its queries are
    slots of F1 in ascending order and their window centres are the cluster's first keypoint, so at window = 100 every query of a structure
    sees its whole cluster:
      run down   12 queries approaching one keypoint with strictly decreasing distance: every one accepts and retracts its predecessor
      stairs     keypoints T0 .. T6 spaced 1.6 times wider each step and queries S, A1 .. A6: Ai is nearer to T(i-1) than to Ti, but T(i-1) is
                 held at no more than that distance by A(i-1) (S for i = 1), which was itself pushed there: a dependence chain 6 deep,
                 every link at a larger distance than the one before
      twins      two queries with the same row on one keypoint: the second is blocked by an EQUAL distance
      pile       K + 4 keypoints each held at distance 0 by a query of its own, then a query at distance 5 of all of them
      flip       a query whose best is free, whose second best is held: it passes the ratio test only because of that"""
    rng = np.random.RandomState(seed)
    q = np.array(d1, F).copy(); pm = np.array(xy1, F).reshape(-1, 2).copy(); tg = np.array(d2, F).copy()
    xy2 = np.asarray(xy2, F).reshape(-1, 2)
    n1, n2 = len(q), len(tg)
    sizes = [1, 7, 1, K + 4, 2]
    used = set()
    clusters = []
    for sz in sizes:
        while True:
            c = int(rng.randint(n2))
            if not (110 < xy2[c, 0] < 530 and 110 < xy2[c, 1] < 370):
                continue
            dd = np.abs(xy2 - xy2[c]).max(1)
            near = np.argsort(dd, kind="stable")[:sz]
            if dd[near[-1]] < 60 and not used.intersection(near.tolist()) and near[0] == c:
                break
        used.update(near.tolist())
        clusters.append(near.tolist())
    # the two views of the synthetic test weights share no descriptor within TH_LOW, so the correspondences are planted too: about 60 % of the
    # queries get the row of a keypoint of F2 that lies within 60 pixels of them plus noise worth 0 .. 110 units of distance.  Several
    # queries draw the same keypoint, at different distances and in no particular slot order
    free = np.array([k not in used for k in range(n2)])
    for s in np.nonzero(rng.rand(n1) < 0.6)[0]:
        near = np.nonzero((np.abs(xy2 - pm[s]).max(1) < 60) & free)[0]
        if len(near) == 0:
            continue
        k = int(near[rng.randint(len(near))])
        e = rng.randn(64)
        q[s] = tg[k] + (e / np.linalg.norm(e) * np.sqrt(rng.uniform(0, 110) / 512.0)).astype(F)
    slots = iter(sorted(rng.choice(np.arange(n1 // 8, n1 - n1 // 8), 12 + 7 + 2 + K + 5 + 2, replace=False).tolist()))
    info = {}
    # run down
    (U,) = clusters[0]
    run = [next(slots) for _ in range(12)]
    for i, s in enumerate(run):
        q[s] = tg[U] + _axis(3, _step(60 - 5 * i)); pm[s] = xy2[U]
    info["run_target"] = U
    # stairs
    T = clusters[1]
    base = tg[T[0]].copy()
    D = [20.0 * 1.6 ** i for i in range(6)]
    for i in range(1, 7):
        tg[T[i]] = tg[T[i - 1]] + _axis(10 + i, float(np.sqrt(D[i - 1] / 512.0)))
    st = [next(slots) for _ in range(7)]
    q[st[0]] = base; pm[st[0]] = xy2[T[0]]
    for i in range(1, 7):
        q[st[i]] = tg[T[i - 1]] + _axis(10 + i, 0.45 * float(np.sqrt(D[i - 1] / 512.0))); pm[st[i]] = xy2[T[0]]
    info["stairs"] = (st, T)
    # twins
    (V,) = clusters[2]
    tw = [next(slots) for _ in range(2)]
    for s in tw:
        q[s] = tg[V] + _axis(20, _step(9)); pm[s] = xy2[V]
    info["twins"] = (tw, V)
    # pile
    P = clusters[3]
    b3 = tg[P[0]].copy()
    for j, k in enumerate(P):
        tg[k] = b3 + _axis(24 + j, 0.1)
    hold = [next(slots) for _ in range(K + 5)]
    for j, k in enumerate(P):
        q[hold[j]] = tg[k]; pm[hold[j]] = xy2[P[0]]
    q[hold[-1]] = b3; pm[hold[-1]] = xy2[P[0]]
    info["pile"] = (hold, P)
    # flip
    Wa, Wb = clusters[4]
    y20, y21 = _step(20), _step(21)
    tg[Wb] = tg[Wa] + _axis(50, y20 + y21)
    fl = [next(slots) for _ in range(2)]
    q[fl[0]] = tg[Wb]; pm[fl[0]] = xy2[Wa]
    q[fl[1]] = tg[Wa] + _axis(50, y20); pm[fl[1]] = xy2[Wa]
    info["flip"] = (fl, (Wa, Wb))
    return q, pm, tg, info


def conditions(seq, free, depth, K):
    """the counts tests/test_init_ref.py asserts on a scene, from the literal form (and the depth of the order-free form)"""
    acc = seq["claim_idx"][seq["claim_idx"] >= 0]
    differs = int(((seq["status"] != free["status"]) | (seq["claim_idx"] != free["claim_idx"]) | (seq["best_dist"] != free["best_dist"]) |
                   (seq["second_dist"] != free["second_dist"])).sum())
    return dict(retractions=int(seq["retractions"]), differs=differs, flips=int(seq["flips"].sum()),
                chain=int(np.bincount(acc).max()) if len(acc) else 0, depth=int(depth), ran_out=int((seq["blocked_ahead"] > K).sum()),
                n_matches=int(seq["n_matches"]))


def warp(img):
    """the second frame of the rig: the first one moved by a few pixels and stretched by under one per cent (nearest neighbour in integers)"""
    H, W = img.shape
    yy = np.clip(np.arange(H) * 127 // 128 + 2, 0, H - 1)
    xx = np.clip(np.arange(W) * 129 // 128 - 3, 0, W - 1)
    return np.ascontiguousarray(img[yy][:, xx])
