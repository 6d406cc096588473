"""Restatement of DBoW2's TemplatedVocabulary::transform(features, v, fv, levelsup) (thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1194 and
the per-feature descent :1218-1259) for the TF_IDF / L1_NORM vocabulary, in two forms that tests/test_vocab_ref.py holds against each other:

  literal     a transcription, feature by feature: the `do ... while(!isLeaf())` loop over `m_nodes[final_id].children` with FORB::distance
              (FORB.cpp:81-101: popcount of the XOR of the first 8 int32 of the row) and the strict `d < best_d`, BowVector::addWeight into a
              dict that is read in key order as the std::map is, FeatureVector::addFeature, BowVector::normalize(L1)
  vectorised  the rule of include/xfeat_hip.h: all features one level at a time; the distinct words of the features that are not stopped,
              ascending; val(word) = ((w + w) + ...) with one double add per feature; norm = the left-to-right sum; val / norm when norm > 0

A vocabulary is a dict(L, parent[n] uint32, word_id[n] uint32, weight[n] float64, desc[n][32] uint8) in node-id order: m_nodes flattened.  Node 0
is the root; the children of a node are the nodes that name it as parent in ascending id (loadFromTextFile's push_back order, :1385-1392); a
node is a leaf iff it has no children.  A feature is the first 32 bytes of a row.  One deviation from the reference, as in the library: where
the path is shorter than nid_level = L - levelsup the reference leaves nid uninitialised (:1150-1155, :1251); here it is the leaf.
No test lives here."""
import numpy as np

NONE = 0xFFFFFFFF


def children(voc):
    """per node the list of its children in ascending id"""
    ch = [[] for _ in range(len(voc["parent"]))]
    for i in range(1, len(ch)):
        ch[int(voc["parent"][i])].append(i)
    return ch


def row_bytes(rows):
    """rows (any dtype, >= 32 bytes per row) -> uint8 [n][32]: the bytes DBoW2 reads"""
    r = np.ascontiguousarray(rows)
    return np.ascontiguousarray(r.reshape(len(r), -1).view(np.uint8)[:, :32])


def _ints(b):
    return [int.from_bytes(bytes(x), "little") for x in b]


def literal(voc, rows, levelsup):
    ch = children(voc)
    desc = _ints(voc["desc"])
    feats = _ints(row_bytes(rows))
    L = int(voc["L"])
    dist = lambda a, b: float(bin(a ^ b).count("1"))                   # FORB::distance, compared as double (:1237, :1242)
    n = len(feats)
    word, node_of, weight = np.zeros(n, np.uint32), np.full(n, NONE, np.uint32), np.zeros(n, np.float64)
    v, fv = {}, {}
    for i_feature, feature in enumerate(feats):
        # transform(*fit, id, w, &nid, levelsup)
        nid = None
        nid_level = L - levelsup
        if nid_level <= 0:
            nid = 0                                                    # root
        final_id = 0
        current_level = 0
        while True:
            current_level += 1
            nodes = ch[final_id]
            final_id = nodes[0]
            best_d = dist(feature, desc[final_id])
            for id_ in nodes[1:]:
                d = dist(feature, desc[id_])
                if d < best_d:
                    best_d = d
                    final_id = id_
            if current_level == nid_level:
                nid = final_id
            if not ch[final_id]:                                       # isLeaf()
                break
        if nid is None:
            nid = final_id                                             # (the deviation: the reference's nid is uninitialised here)
        wid, w = int(voc["word_id"][final_id]), float(voc["weight"][final_id])
        word[i_feature], weight[i_feature] = wid, w
        if w > 0:                                                      # not stopped
            if wid in v:                                               # BowVector::addWeight
                v[wid] += w
            else:
                v[wid] = w
            fv.setdefault(nid, []).append(i_feature)                   # FeatureVector::addFeature
            node_of[i_feature] = nid
    keys = sorted(v)                                                   # the std::map is walked in key order
    norm = 0.0
    for k in keys:
        norm += abs(v[k])
    if norm > 0.0:
        for k in keys:
            v[k] /= norm
    return dict(word=word, node_of=node_of, weight=weight, bow_ids=np.array(keys, np.uint32), bow_vals=np.array([v[k] for k in keys], np.float64),
                n_words=len(keys), fv={k: fv[k] for k in sorted(fv)})


def paths(voc, rows):
    """every feature down the tree, all features one level at a time -> path[n][depth + 1] node ids (path[:, 0] = 0, -1 past the leaf)"""
    parent = np.asarray(voc["parent"], np.int64)
    n_nodes = len(parent)
    order = np.argsort(parent[1:], kind="stable") + 1                  # the children lists, concatenated: ascending id inside a parent
    cnt = np.bincount(parent[1:], minlength=n_nodes)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    desc = np.asarray(voc["desc"], np.uint8)
    q = row_bytes(rows)
    n = len(q)
    cur = np.zeros(n, np.int64)
    out = [cur.copy()]
    while True:
        act = np.nonzero(cnt[cur] > 0)[0]
        if len(act) == 0:
            break
        best = np.full(len(act), 1 << 30, np.int64); pick = np.zeros(len(act), np.int64)
        for c in range(int(cnt[cur[act]].max())):
            ok = c < cnt[cur[act]]
            cid = order[np.minimum(start[cur[act]] + c, n_nodes - 2)]
            d = np.unpackbits(desc[cid] ^ q[act], axis=1).sum(1).astype(np.int64)
            better = ok & (d < best)                                   # strict: the first child with the least distance stays
            best[better] = d[better]; pick[better] = cid[better]
        cur = cur.copy(); cur[act] = pick
        col = np.full(n, -1, np.int64); col[act] = pick
        out.append(col)
    return np.stack(out, 1)


def vectorised(voc, rows, levelsup, path=None):
    p = paths(voc, rows) if path is None else path
    n = len(p)
    depth = (p >= 0).sum(1) - 1                                        # the level of the leaf
    leaf = p[np.arange(n), depth]
    nid_level = int(voc["L"]) - levelsup
    if nid_level <= 0:
        nid = np.zeros(n, np.int64)
    else:
        nid = np.where(depth >= nid_level, p[:, min(nid_level, p.shape[1] - 1)], leaf)
    word = np.asarray(voc["word_id"], np.uint32)[leaf]
    weight = np.asarray(voc["weight"], np.float64)[leaf]
    go = weight > 0                                                    # (false for NaN)
    node_of = np.where(go, nid, NONE).astype(np.uint32)
    ids = np.unique(word[go])
    vals = np.zeros(len(ids), np.float64)
    for k, wid in enumerate(ids):                                      # one double add per feature, in feature order
        acc = None
        for w in weight[go & (word == wid)]:
            acc = w if acc is None else acc + w
        vals[k] = acc
    norm = 0.0
    for x in vals:
        norm += abs(x)
    if norm > 0.0:
        vals = vals / norm
    return dict(word=word, node_of=node_of, weight=weight, bow_ids=ids.astype(np.uint32), bow_vals=vals, n_words=len(ids))


def feature_vector(node_of):
    """node_of -> {node id: [feature indices]} in ascending node id: mFeatVec"""
    fv = {}
    for i, nd in enumerate(np.asarray(node_of).tolist()):
        if nd != NONE:
            fv.setdefault(nd, []).append(i)
    return {k: fv[k] for k in sorted(fv)}
