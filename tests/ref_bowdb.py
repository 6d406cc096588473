"""KeyFrameDatabase::DetectRelocalizationCandidates / DetectNBestCandidates (src/KeyFrameDatabase.cc:733-845, :604-730) and L1Scoring::score
(thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) restated twice.

`literal` transcribes the reference: an inverted file of lists per word filled in `add` order, per-keyframe mutable query / words / score
fields, the walk over the query's words, `score` with its lower_bound hops, the accumulation over the covisibility neighbours, a stable list
sort and the set-based dedupe.  `rule` is the order-free statement include/xfeat_hip.h documents and the kernels implement: intersection sizes,
the list as the scored slots sorted by (first shared word, insertion sequence), the sum over the shared ids in ascending id.  tests/test_bowdb_ref.py
holds the two against each other; the GPU tests compare the device with `rule`.

A database is a dict: vecs = per slot (ids uint32 ascending, vals float64) or None for an empty slot; seq = uint32 [n] or None (= slot index);
neigh = int32 [n][nn] (an entry < 0 or >= n means none).  A query is (ids, vals).  fp32 arithmetic is numpy float32 scalar arithmetic: one
rounding per operation, as the reference's float variables."""
import bisect
import functools

import numpy as np

F = np.float32
RELOC, NBEST = 0, 1
EMPTY, NOT_SHARING, EXCLUDED, BELOW_MIN, SCORED = range(5)
NO_WORD = 0xFFFFFFFF


def min_common(max_common):
    """`int minCommonWords = maxCommonWords*0.8f;`"""
    return int(F(max_common) * F(0.8))


# ---- the literal transcription -----------------------------------------------------------------------------------------------------------
def literal_score(v1, v2):
    """L1Scoring::score(v1, v2): two std::map walked together, lower_bound hops over the ids that are not shared"""
    k1, x1 = [int(i) for i in v1[0]], [float(v) for v in v1[1]]
    k2, x2 = [int(i) for i in v2[0]], [float(v) for v in v2[1]]
    i1 = i2 = 0
    score = 0.0
    while i1 != len(k1) and i2 != len(k2):
        vi, wi = x1[i1], x2[i2]
        if k1[i1] == k2[i2]:
            score += abs(vi - wi) - abs(vi) - abs(wi)
            i1 += 1; i2 += 1
        elif k1[i1] < k2[i2]:
            i1 = bisect.bisect_left(k1, k2[i2])
        else:
            i2 = bisect.bisect_left(k2, k1[i1])
    return -score / 2.0


class _KF:
    def __init__(self, slot, vec):
        self.slot, self.vec = slot, vec
        self.query, self.words = -1, 0                               # mnRelocQuery / mnPlaceRecognitionQuery, mnRelocWords / mnPlaceRecognitionWords


def literal(db, query, form, state, exclude=()):
    """one query, the reference's way.  state: float32 [n], mRelocScore resp. mPlaceRecognitionScore of every keyframe, updated IN PLACE.
    -> dict(listed = lKFsSharingWords as slots, words = {slot: count} of the listed, max_common, min_common, list_slot / list_acc / list_best,
    best_acc, cand_slot, cand_acc)"""
    n = len(db["vecs"])
    seq = np.arange(n) if db["seq"] is None else db["seq"]
    kfs = {s: _KF(s, db["vecs"][s]) for s in range(n) if db["vecs"][s] is not None and len(db["vecs"][s][0]) > 0}
    inverted = {}                                                    # mvInvertedFile: `add` pushes the keyframe to the list of each of its words
    for s in sorted(kfs, key=lambda s: (int(seq[s]), s)):
        for w in kfs[s].vec[0]:
            inverted.setdefault(int(w), []).append(kfs[s])
    connected = set(int(s) for s in exclude)
    qid = 1
    out = dict(listed=[], words={}, max_common=0, min_common=0, list_slot=[], list_acc=[], list_best=[], best_acc=F(0), cand_slot=[], cand_acc=[])
    sharing = []
    for w in query[0]:
        for kf in inverted.get(int(w), []):
            if kf.query != qid:
                kf.words = 0
                if kf.slot not in connected:
                    kf.query = qid
                    sharing.append(kf)
            kf.words += 1
    out["listed"] = [kf.slot for kf in sharing]
    out["words"] = {kf.slot: kf.words for kf in sharing}
    if not sharing:
        return out
    max_common_words = 0
    for kf in sharing:
        if kf.words > max_common_words:
            max_common_words = kf.words
    min_common_words = min_common(max_common_words)
    out["max_common"], out["min_common"] = max_common_words, min_common_words
    score_and_match = []
    for kf in sharing:
        if kf.words > min_common_words:
            si = F(literal_score(query, kf.vec))
            state[kf.slot] = si
            score_and_match.append((si, kf))
    if not score_and_match:
        return out
    acc_and_match = []
    best_acc = F(0)
    for si, kf in score_and_match:
        best_score, acc, best = si, si, kf
        for t in db["neigh"][kf.slot] if db["neigh"].size else ():
            t = int(t)
            if t < 0 or t >= n or t not in kfs:
                continue
            kf2 = kfs[t]
            if kf2.query != qid:
                continue
            acc = F(acc + state[t])
            if state[t] > best_score:
                best, best_score = kf2, state[t]
        acc_and_match.append((acc, best))
        if acc > best_acc:
            best_acc = acc
    out["list_slot"] = [kf.slot for _, kf in score_and_match]
    out["list_acc"] = [a for a, _ in acc_and_match]
    out["list_best"] = [b.slot for _, b in acc_and_match]
    out["best_acc"] = best_acc
    already = set()
    if form == RELOC:
        min_score_to_retain = F(0.75) * best_acc
        for acc, kf in acc_and_match:
            if acc > min_score_to_retain and kf.slot not in already:
                out["cand_slot"].append(kf.slot); out["cand_acc"].append(acc)
                already.add(kf.slot)
    else:
        comp_first = functools.cmp_to_key(lambda a, b: -1 if a[0] > b[0] else (1 if b[0] > a[0] else 0))      # list::sort(compFirst) is stable
        for acc, kf in sorted(acc_and_match, key=comp_first):
            if kf.slot not in already:
                out["cand_slot"].append(kf.slot); out["cand_acc"].append(acc)
                already.add(kf.slot)
    return out


# ---- the order-free rule ------------------------------------------------------------------------------------------------------------------
def shared(v1, v2):
    """positions in v1 and in v2 of the shared ids, in ascending id"""
    i1, i2 = np.asarray(v1[0], np.uint32), np.asarray(v2[0], np.uint32)
    if len(i1) == 0 or len(i2) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    p = np.searchsorted(i1, i2)
    hit = (p < len(i1)) & (i1[np.minimum(p, len(i1) - 1)] == i2)
    return p[hit], np.nonzero(hit)[0]


def terms(v1, v2):
    p1, p2 = shared(v1, v2)
    vi, wi = np.asarray(v1[1], np.float64)[p1], np.asarray(v2[1], np.float64)[p2]
    return (np.abs(vi - wi) - np.abs(vi)) - np.abs(wi)


def rule_score(v1, v2):
    """-> (score, n_common, first_common): the terms of the shared ids added left to right in ascending id from 0.0 (cumsum is sequential)"""
    t = terms(v1, v2)
    p1, _ = shared(v1, v2)
    total = np.cumsum(np.concatenate([[0.0], t]))[-1]
    return -total / 2.0, len(t), int(np.asarray(v1[0])[p1[0]]) if len(t) else NO_WORD


def rule(db, query, form, state, exclude=()):
    """one query by the order-free rule.  state: float32 [n], updated IN PLACE.  -> the outputs of xfh_bowdb_query_device for one problem:
    common, score, status, list_slot / list_acc / list_best, cand_slot / cand_acc (all [n]), n_listed, max_common, min_common, n_scored,
    n_candidates, best_acc; and listed = the listed slots in list order (what `literal` walks)"""
    n = len(db["vecs"])
    seq = np.arange(n, dtype=np.int64) if db["seq"] is None else np.asarray(db["seq"], np.int64)
    common, score, first = np.zeros(n, np.int32), np.full(n, -0.0, np.float64), np.full(n, NO_WORD, np.int64)
    status = np.zeros(n, np.uint8)
    ex = np.zeros(n, bool)
    ex[np.asarray(list(exclude), np.int64)] = True
    for s in range(n):
        v = db["vecs"][s]
        if v is None or len(v[0]) == 0:
            status[s] = EMPTY
            continue
        score[s], common[s], first[s] = rule_score(query, v)
        status[s] = NOT_SHARING if common[s] == 0 else (EXCLUDED if ex[s] else BELOW_MIN)
    listed = status == BELOW_MIN
    o = dict(common=common, score=score, status=status, n_listed=int(listed.sum()), max_common=0, min_common=0)
    if listed.any():
        o["max_common"] = int(common[listed].max())
        o["min_common"] = min_common(o["max_common"])
    status[listed & (common > o["min_common"])] = SCORED
    order = lambda sl: sorted(sl, key=lambda s: (int(first[s]), int(seq[s]), int(s)))
    o["listed"] = order(np.nonzero(listed)[0].tolist())
    lst = order(np.nonzero(status == SCORED)[0].tolist())
    for s in lst:
        state[s] = F(score[s])
    acc, best = [], []
    for s in lst:
        a = bs = F(score[s])
        b = s
        for t in db["neigh"][s] if db["neigh"].size else ():
            t = int(t)
            if t < 0 or t >= n or not listed[t]:
                continue
            a = F(a + state[t])
            if state[t] > bs:
                b, bs = t, state[t]
        acc.append(a); best.append(b)
    best_acc = F(0)
    for a in acc:
        if a > best_acc:
            best_acc = a
    if form == RELOC:
        seq_in = [r for r in range(len(lst)) if acc[r] > F(0.75) * best_acc]
    else:
        seq_in = sorted(range(len(lst)), key=lambda r: (-float(acc[r]) + 0.0, r))         # (+ 0.0: -0.0 and 0.0 are one key)
    cands, seen = [], set()
    for r in seq_in:
        if best[r] not in seen:
            cands.append(r); seen.add(best[r])

    def full(vals, fill, dt):
        a = np.full(n, fill, dt)
        a[:len(vals)] = vals
        return a
    o.update(n_scored=len(lst), n_candidates=len(cands), best_acc=best_acc, list_slot=full(lst, -1, np.int32), list_acc=full(acc, 0, F),
             list_best=full(best, -1, np.int32), cand_slot=full([best[r] for r in cands], -1, np.int32), cand_acc=full([acc[r] for r in cands], 0, F))
    return o
