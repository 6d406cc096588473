"""Restatement of ORBmatcher::SearchByBoW (reference src/ORBmatcher.cc; the frame form :408-610 and the keyframe form :950-1090, no second
camera; the rotation histogram removes nothing because every XFeat angle is -1) in two forms:

  literal()    the loop transcribed: the two map iterators with lower_bound over dicts built like addFeature, the claim vector
               (vpMapPointMatches[realIdxF] resp. vbMatched2) shared by the whole call, best / second from init_dist with the strict
               `<` / `else if <` update
  per_node()   the contract of xfh_bow_search_device: the nodes treated independently, each with a claim set of its own, in ANY order
               (`order`: a seed for the permutation), with the statuses and counts; claims=False gives the claim-free answer the tests
               compare against, and `stats` receives what the scene is chosen for

`dist` is the n1 x n2 table of DescriptorDistance (the C oracle's distance_i32).  accept() is numpy fp32.  No test lives here."""
import bisect

import numpy as np

from ref_triangulation import NONE, feature_vector

F = np.float32
INACTIVE, NO_NODE, NO_CANDIDATES, REJECTED, MATCHED = range(5)
STRICT_LOW = 1
TH_LOW, INIT = 100, 256
OUT = ("status", "match12", "best_dist", "second_dist", "n_candidates")
K_LIST = 4                # the length of the kernel's candidate lists: only the statistics of per_node know about it


def accept(best_idx, best, second, th_low, nn_ratio, flags):
    """:512-514 resp. :1033-1036 (with the best_idx >= 0 the contract adds for th_low >= init_dist)"""
    low = best < th_low if flags & STRICT_LOW else best <= th_low
    return bool(best_idx >= 0 and low and F(best) < F(F(nn_ratio) * F(second)))


def search(dist, i, members, eligible2, claimed, init_dist):
    """the inner loop: -> (best_idx, best, second, n_candidates)"""
    best, second, bi, nc = init_dist, init_dist, -1, 0
    for k in members:
        if eligible2 is not None and not eligible2[k]:
            continue
        if claimed is not None and claimed[k]:
            continue
        nc += 1
        d = int(dist[i, k])
        if d < best:
            second, best, bi = best, d, k
        elif d < second:
            second = d
    return bi, best, second, nc


def empty(n1, n2, init_dist):
    return dict(status=np.zeros(n1, np.uint8), match12=np.full(n1, -1, np.int32), best_dist=np.full(n1, init_dist, np.int32),
                second_dist=np.full(n1, init_dist, np.int32), n_candidates=np.zeros(n1, np.int32), assigned2=np.full(n2, -1, np.int32), n_matches=0)


def literal(dist, node_of1, active1, node_of2, eligible2=None, flags=0, init_dist=INIT, th_low=TH_LOW, nn_ratio=0.6):
    """-> dict(match12, best_dist, second_dist, n_candidates, assigned2, n_matches): what the reference's loop leaves behind"""
    fv1, fv2 = feature_vector(node_of1), feature_vector(node_of2)
    key1, key2 = list(fv1), list(fv2)
    o = empty(len(node_of1), len(node_of2), init_dist)
    del o["status"]
    claimed = np.zeros(len(node_of2), bool)               # vpMapPointMatches[k] != NULL resp. vbMatched2[k]
    f1, f2 = 0, 0
    while f1 != len(key1) and f2 != len(key2):
        if key1[f1] == key2[f2]:
            for idx1 in fv1[key1[f1]]:
                if not active1[idx1]:
                    continue
                bi, best, second, nc = search(dist, idx1, fv2[key2[f2]], eligible2, claimed, init_dist)
                o["best_dist"][idx1], o["second_dist"][idx1], o["n_candidates"][idx1] = best, second, nc
                if accept(bi, best, second, th_low, nn_ratio, flags):
                    o["match12"][idx1] = bi; o["assigned2"][bi] = idx1; claimed[bi] = True
                    o["n_matches"] += 1
            f1 += 1; f2 += 1
        elif key1[f1] < key2[f2]:
            f1 = bisect.bisect_left(key1, key2[f2])
        else:
            f2 = bisect.bisect_left(key2, key1[f1])
    return o


def new_stats():
    return dict(depth=None, ahead=None, runs_out=0, tie_first_wins=0, single=0, none_eligible=0, none_after_claims=0)


def per_node(dist, node_of1, active1, node_of2, eligible2=None, flags=0, init_dist=INIT, th_low=TH_LOW, nn_ratio=0.6, order=None, claims=True, stats=None):
    """the contract of include/xfeat_hip.h"""
    fv1, fv2 = feature_vector(node_of1), feature_vector(node_of2)
    n1, n2 = len(node_of1), len(node_of2)
    o = empty(n1, n2, init_dist)
    for i in range(n1):
        if active1[i]:
            nd = int(node_of1[i])
            o["status"][i] = NO_NODE if nd == NONE or nd not in fv2 else NO_CANDIDATES
    common = [k for k in fv1 if k in fv2]
    if order is not None:
        common = [common[j] for j in np.random.RandomState(order).permutation(len(common))]
    if stats is not None:
        stats["depth"] = np.zeros(n1, np.int32); stats["ahead"] = np.zeros(n1, np.int32)
    for nd in common:
        claimed = np.zeros(n2, bool) if claims else None  # this node's own
        claimer = {}
        for i in fv1[nd]:
            if not active1[i]:
                continue
            bi, best, second, nc = search(dist, i, fv2[nd], eligible2, claimed, init_dist)
            o["best_dist"][i], o["second_dist"][i], o["n_candidates"][i] = best, second, nc
            ok = accept(bi, best, second, th_low, nn_ratio, flags)
            if ok:
                o["status"][i] = MATCHED; o["match12"][i] = bi; o["assigned2"][bi] = i
                o["n_matches"] += 1
            else:
                o["status"][i] = NO_CANDIDATES if nc == 0 else REJECTED
            if stats is not None and claims:
                fbi, fbest, _, fnc = search(dist, i, fv2[nd], eligible2, None, init_dist)
                # the candidates below init_dist in the order the strict '<' picks them, and how many claimed ones precede the best
                ranked = sorted((int(dist[i, k]), p) for p, k in enumerate(fv2[nd]) if (eligible2 is None or eligible2[k]) and int(dist[i, k]) < init_dist)
                mem = fv2[nd]
                free = [j for j, (d, p) in enumerate(ranked) if not claimed[mem[p]]]
                ahead = free[0] if free else len(ranked)
                stats["ahead"][i] = ahead
                if ahead > 0:                              # a chain: whoever took the candidate just ahead had been pushed there itself
                    stats["depth"][i] = stats["depth"][claimer[mem[ranked[ahead - 1][1]]]] + 1
                if len(ranked) > K_LIST and sum(1 for j in free if j < K_LIST) < 2:
                    stats["runs_out"] += 1
                if ok and sum(1 for d, p in ranked if d == best and not claimed[mem[p]]) > 1 and bi == min(mem[p] for d, p in ranked if d == best and not claimed[mem[p]]):
                    stats["tie_first_wins"] += 1
                stats["single"] += int(nc == 1 and second == init_dist and bi >= 0)
                stats["none_eligible"] += int(fnc == 0)
                stats["none_after_claims"] += int(fnc > 0 and nc == 0)
            if ok and claims:
                claimed[bi] = True; claimer[bi] = i
    return o


def handmade():
    """-> (name, dist, node_of1, active1, node_of2, eligible2, flags, nn_ratio, want) with the answers written out"""
    u32 = lambda a: np.array(a, np.uint32)
    u8 = lambda a: np.array(a, np.uint8)
    N = NONE
    c = []
    # one node, two queries with the same nearest target: the second takes its own second best, and only because the first claimed
    d = np.array([[10, 30, 200], [12, 40, 90]])
    c.append(("claim moves the second query", d, u32([7, 7]), u8([1, 1]), u32([7, 7, 7]), None, 0, 0.6,
              dict(status=[MATCHED, MATCHED], match12=[0, 1], best_dist=[10, 40], second_dist=[30, 90], n_candidates=[3, 2], assigned2=[0, 1, -1])))
    # a chain of depth 3: every query's nearest was taken by the one before
    d = np.array([[5, 20, 60, 250], [6, 21, 61, 250], [7, 22, 62, 250], [8, 23, 63, 250]])
    c.append(("chain", d, u32([1] * 4), u8([1] * 4), u32([1] * 4), None, 0, 0.6,
              dict(status=[MATCHED] * 3 + [REJECTED], match12=[0, 1, 2, -1], best_dist=[5, 21, 62, 250], second_dist=[20, 61, 250, 256], n_candidates=[4, 3, 2, 1],
                   assigned2=[0, 1, 2, -1])))
    # accepted only because the earlier query claimed the second best (20 < 0.6 * 25 fails, 20 < 0.6 * 256 passes); and the opposite
    d = np.array([[300, 1, 300], [20, 25, 300]])
    c.append(("ratio passes after a claim", d, u32([3, 3]), u8([1, 1]), u32([3, 3, 3]), None, 0, 0.6,
              dict(status=[MATCHED, MATCHED], match12=[1, 0], best_dist=[1, 20], second_dist=[256, 256], n_candidates=[3, 2], assigned2=[1, 0, -1])))
    d = np.array([[1, 300, 300], [10, 40, 50]])
    c.append(("ratio fails after a claim", d, u32([3, 3]), u8([1, 1]), u32([3, 3, 3]), None, 0, 0.6,
              dict(status=[MATCHED, REJECTED], match12=[0, -1], best_dist=[1, 40], second_dist=[256, 50], n_candidates=[3, 2], assigned2=[0, -1, -1])))
    # equal distances: rejected for nn_ratio <= 1 (best == second), the FIRST member wins at 1.5; a zero distance never passes (0 < r * 0 is false)
    d = np.array([[30, 30, 30], [0, 0, 0]])
    c.append(("tie at 0.9", d, u32([2, 2]), u8([1, 1]), u32([2, 2, 2]), None, 0, 0.9,
              dict(status=[REJECTED, REJECTED], match12=[-1, -1], best_dist=[30, 0], second_dist=[30, 0], n_candidates=[3, 3], assigned2=[-1, -1, -1])))
    c.append(("tie at 1.5: first wins", d, u32([2, 2]), u8([1, 1]), u32([2, 2, 2]), None, 0, 1.5,
              dict(status=[MATCHED, REJECTED], match12=[0, -1], best_dist=[30, 0], second_dist=[30, 0], n_candidates=[3, 2], assigned2=[0, -1, -1])))
    # best == th_low: the frame form accepts, the keyframe form does not; eligibility; statuses; ids above 2^31 compare unsigned
    d = np.array([[100, 255, 7, 7], [7, 7, 7, 7], [7, 7, 7, 7], [7, 7, 7, 7], [50, 60, 7, 7], [7, 7, 7, 7]])
    n1 = u32([5, 5, N, 8, 0x80000001, 9]); a1 = u8([1, 0, 1, 1, 1, 1]); n2 = u32([5, 5, 0x80000001, 9]); e2 = u8([1, 1, 1, 0])
    c.append(("th_low, frame form", d, n1, a1, n2, None, 0, 0.6,
              dict(status=[MATCHED, INACTIVE, NO_NODE, NO_NODE, MATCHED, MATCHED], match12=[0, -1, -1, -1, 2, 3], best_dist=[100, 256, 256, 256, 7, 7],
                   second_dist=[255, 256, 256, 256, 256, 256], n_candidates=[2, 0, 0, 0, 1, 1], assigned2=[0, -1, 4, 5])))
    c.append(("th_low, keyframe form", d, n1, a1, n2, e2, STRICT_LOW, 0.6,
              dict(status=[REJECTED, INACTIVE, NO_NODE, NO_NODE, MATCHED, NO_CANDIDATES], match12=[-1, -1, -1, -1, 2, -1], best_dist=[100, 256, 256, 256, 7, 256],
                   second_dist=[255, 256, 256, 256, 256, 256], n_candidates=[2, 0, 0, 0, 1, 0], assigned2=[-1, -1, 4, -1])))
    # two nodes: a claim in one never reaches the other, and one target for three queries is gone after the first
    d = np.array([[9, 9], [9, 9], [9, 9], [9, 9]])
    c.append(("none after the claims", d, u32([4, 4, 4, 6]), u8([1] * 4), u32([4, 6]), None, 0, 0.6,
              dict(status=[MATCHED, NO_CANDIDATES, NO_CANDIDATES, MATCHED], match12=[0, -1, -1, 1], best_dist=[9, 256, 256, 9], second_dist=[256] * 4,
                   n_candidates=[1, 0, 0, 1], assigned2=[0, 3])))
    return c
