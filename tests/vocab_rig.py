"""The seeded vocabularies and feature sets of the vocabulary-transform tests (tests/test_vocab_ref.py, tests/test_gpu_vocab.py,
tests/test_gpu_vocab_cpp.py) and one guarded run of xfh_bow_transform_device.  Vocabularies (dicts as tests/ref_vocab.py takes them):
  bfs        regular, k = 10, L = 3 (1111 nodes), random descriptor bytes, numbered breadth first as loadFromTextFile numbers ORBvoc.txt
  dfs        the same tree numbered depth first: the ids of siblings are not adjacent
  irregular  L = 3; 1 to 20 children per node and one node with 21 .. 32 (two passes of the 16 lanes); leaves at levels 1, 2 and 3 and a
             chain that ends at depth 10; duplicate sibling descriptors; siblings at equal distance from a planted feature (the first wins);
             leaves with weight 0, a negative weight and NaN; and, last, the phantom child of the root that loadFromTextFile's `while(!f.eof())`
             makes of a trailing newline: a zero descriptor, weight 0, word_id 0, no children.  Below level 1 a descriptor is its parent's with
             a few bits flipped, so a feature that equals a node's descriptor goes down to that node.  irregular() asserts each condition.
Feature sets (float32 [n][64]; only the first 32 bytes of a row matter, the rest is random):
  mixed      zero rows, duplicate rows, rows whose first 32 bytes equal a node's descriptor, rows whose floats are NaN, +-Inf and -0.0
             patterns, random rows
  oneword    every row goes to ONE word (n features on one leaf: the iterated sum of its weight is asserted to differ from n * w)
  stopped    every row is stopped (n_words = 0, the blob of an all-NONE node_of)
No test lives here."""
import functools

import numpy as np

import guarded
import ref_vocab as RV
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context

F = np.float32
GUARD = 4096
SIZES = (1, 5, 257, 4096)
NAMES = ("bfs", "dfs", "irregular")


def levelsups(L):
    return (0, 1, 4, L, L + 1)


def _finish(parent, desc, rng, L, weight=None):
    """word ids: the leaves in node-id order, as loadFromTextFile fills m_words; weights: positive idf-like values"""
    parent = np.asarray(parent, np.uint32)
    n = len(parent)
    has_child = np.zeros(n, bool); has_child[parent[1:]] = True
    word_id = np.zeros(n, np.uint32)
    word_id[~has_child] = np.arange((~has_child).sum(), dtype=np.uint32)
    w = rng.uniform(0.05, 9.0, n) if weight is None else np.asarray(weight, np.float64)
    w = np.where(has_child, 0.0, w)
    return dict(L=L, parent=parent, word_id=word_id, weight=w.astype(np.float64), desc=np.ascontiguousarray(desc, np.uint8))


@functools.lru_cache(maxsize=None)
def regular(depth_first, k=10, L=3, seed=5100):
    rng = np.random.RandomState(seed)
    # breadth first: node i's children are k * i + 1 .. k * i + k
    n = (k ** (L + 1) - 1) // (k - 1)
    parent = np.zeros(n, np.int64); parent[1:] = (np.arange(1, n) - 1) // k
    desc = rng.randint(0, 256, (n, 32)).astype(np.uint8)
    if depth_first:
        ch = [[] for _ in range(n)]
        for i in range(1, n):
            ch[parent[i]].append(i)
        new_of, stack = np.zeros(n, np.int64), [0]
        order = []
        while stack:                                                   # pre-order, children in their order
            x = stack.pop(); new_of[x] = len(order); order.append(x)
            stack.extend(reversed(ch[x]))
        p2 = np.zeros(n, np.int64); p2[new_of[1:]] = new_of[parent[1:]]
        d2 = np.zeros_like(desc); d2[new_of] = desc
        parent, desc = p2, d2
        sib = [i for i in range(1, n) if parent[i] == 0]
        assert np.all(np.diff(sib) > 1) and np.all(parent[1:] < np.arange(1, n))
    return _finish(parent, desc, rng, L)


def _flip(rng, row, bits):
    out = np.unpackbits(row).copy()
    out[rng.choice(256, bits, replace=False)] ^= 1
    return np.packbits(out)


@functools.lru_cache(maxsize=None)
def irregular(seed=5200):
    rng = np.random.RandomState(seed)
    L = 3
    parent, desc, special = [0], [np.zeros(32, np.uint8)], {}

    def add(p, row=None, bits=10):
        parent.append(p)
        desc.append(_flip(rng, desc[p], bits) if row is None else row)
        return len(parent) - 1

    top = [add(0, rng.randint(0, 256, 32).astype(np.uint8)) for _ in range(12)]
    special["leaf1"] = top[0]                                          # a leaf at level 1
    wide = [add(top[1]) for _ in range(25)]                            # 25 children: two passes; the winner may sit in the second
    special["wide_late"] = wide[20]
    mids = [add(top[2]) for _ in range(5)]
    for m in mids:
        for _ in range(int(rng.randint(1, 21))):
            add(m)                                                     # leaves at level L = 3
    x = top[3]
    for _ in range(9):                                                 # a chain: one child per node, down to depth 10
        x = add(x, bits=4)
    special["chain_end"] = x
    dups = [add(top[4]) for _ in range(6)]
    desc[dups[1]] = desc[dups[0]].copy(); desc[dups[4]] = desc[dups[3]].copy()
    special["dup_first"], special["dup_second"] = dups[0], dups[1]
    planted = _flip(rng, desc[top[5]], 6)                              # siblings at distance 1 from a planted feature, and one at distance 2 in front
    ties = [add(top[5], _flip(rng, planted, 2))]
    for b in (3, 77, 200):
        r = np.unpackbits(planted).copy(); r[b] ^= 1
        ties.append(add(top[5], np.packbits(r)))
    special["planted"], special["tie_first"] = planted, ties[1]
    for t in top[6:]:
        kids = [add(t) for _ in range(int(rng.randint(1, 21)))]
        for kid in kids[:2]:
            for _ in range(int(rng.randint(1, 5))):
                add(kid)
    special["w_zero"], special["w_neg"], special["w_nan"] = wide[3], wide[4], wide[5]
    phantom = add(0, np.zeros(32, np.uint8))                           # the last line of the file: a trailing newline
    special["phantom"] = phantom
    n = len(parent)
    w = rng.uniform(0.05, 9.0, n)
    w[special["w_zero"]] = 0.0; w[special["w_neg"]] = -1.5; w[special["w_nan"]] = np.nan; w[phantom] = 0.0
    voc = _finish(parent, np.stack(desc), rng, L, weight=w)
    voc["word_id"][phantom] = 0
    voc["special"] = special
    # the conditions this vocabulary is chosen for
    ch = RV.children(voc)
    counts = [len(c) for c in ch if c]
    level = np.zeros(n, int)
    for i in range(1, n):
        level[i] = level[parent[i]] + 1
    leaves = np.array([not c for c in ch])
    assert min(counts) == 1 and sum(20 < c <= 32 for c in counts) == 1 and max(c for c in counts if c <= 20) >= 12 and len(ch[top[1]]) == 25
    assert {1, 2, L} <= set(level[leaves].tolist()) and level[special["chain_end"]] == 10 and level.max() == 10
    assert all(len(ch[j]) == 1 for j in _ancestors(parent, special["chain_end"])[1:-1])
    assert np.array_equal(voc["desc"][dups[0]], voc["desc"][dups[1]]) and np.array_equal(voc["desc"][dups[3]], voc["desc"][dups[4]])
    pd = lambda a, b: int(np.unpackbits(a ^ b).sum())
    assert [pd(planted, voc["desc"][t]) for t in ties] == [2, 1, 1, 1]
    assert ch[0][-1] == phantom == n - 1 and not ch[phantom] and not voc["desc"][phantom].any() and voc["weight"][phantom] == 0 and voc["word_id"][phantom] == 0
    assert voc["weight"][special["w_zero"]] == 0 and voc["weight"][special["w_neg"]] < 0 and np.isnan(voc["weight"][special["w_nan"]])
    assert all(leaves[special[k]] for k in ("leaf1", "wide_late", "chain_end", "dup_first", "dup_second", "tie_first", "w_zero", "w_neg", "w_nan", "phantom"))
    # a feature that equals a node's descriptor reaches that node -- except the second of two identical siblings: the first wins
    for k in ("leaf1", "wide_late", "chain_end", "dup_first", "tie_first", "w_zero", "w_neg", "w_nan", "phantom"):
        row = planted if k == "tie_first" else voc["desc"][special[k]]
        assert RV.paths(voc, row[None])[0].max() == special[k] and RV.paths(voc, row[None])[0][level[special[k]]] == special[k], k
    assert RV.paths(voc, voc["desc"][dups[1]][None])[0][2] == dups[0]
    return voc


def _ancestors(parent, i):
    out = [i]
    while i:
        i = int(parent[i]); out.append(i)
    return out[::-1]


def vocabulary(name):
    return {"bfs": lambda: regular(False), "dfs": lambda: regular(True), "irregular": irregular}[name]()


@functools.lru_cache(maxsize=None)
def blob(name):
    v = vocabulary(name)
    return Context.vocab_pack(v["parent"], v["word_id"], v["weight"], v["desc"], v["L"])[0]


def _rows(rng, first32):
    """float32 [n][64] rows with the given first 32 bytes and random floats behind them"""
    n = len(first32)
    rows = rng.randn(n, 64).astype(F)
    rows.view(np.uint8).reshape(n, 256)[:, :32] = first32
    return rows


@functools.lru_cache(maxsize=None)
def features(name, kind, n, seed=5300):
    voc = vocabulary(name)
    rng = np.random.RandomState(seed + n + 7 * NAMES.index(name))
    leaves = np.nonzero(~np.isin(np.arange(len(voc["parent"])), voc["parent"][1:]))[0]
    if kind == "oneword":
        live = leaves[voc["weight"][leaves] > 0]
        for target in live[rng.permutation(len(live))]:                # a leaf whose own descriptor goes to it and whose iterated sum is not n * w
            row = voc["desc"][target]
            w = float(voc["weight"][target])
            acc = 0.0
            for _ in range(n):
                acc += w
            if RV.paths(voc, row[None])[0].max() == target and (n < 3 or acc != n * w):
                break
        else:
            raise AssertionError("no leaf fits")
        return _rows(rng, np.repeat(row[None], n, 0))
    if kind == "stopped":
        assert name == "irregular"
        sp = voc["special"]
        pick = np.array([sp["phantom"], sp["w_zero"], sp["w_neg"], sp["w_nan"]])[rng.randint(0, 4, n)]
        return _rows(rng, voc["desc"][pick])
    assert kind == "mixed"
    first = rng.randint(0, 256, (n, 32)).astype(np.uint8)
    pats = np.array([0x7fc00000, 0xffc00001, 0x7f800000, 0xff800000, 0x80000000, 0x7fffffff, 0x00000001, 0x3f800000], np.uint32)
    for i in range(n):
        r = i % 8
        if r == 0:
            first[i] = 0                                               # a zero row: a padding row of the record
        elif r == 1 and i >= 8:
            first[i] = first[i - 8 + 2]                                # a duplicate of an earlier row
        elif r == 2:
            first[i] = voc["desc"][rng.randint(1, len(voc["desc"]))]   # a node's descriptor
        elif r == 3:
            first[i] = pats[rng.randint(0, len(pats), 8)].view(np.uint8)   # NaN, +-Inf, -0.0 ... patterns
        elif r == 4 and "special" in voc:
            sp = voc["special"]
            keys = ("leaf1", "wide_late", "chain_end", "dup_second", "w_zero", "w_neg", "w_nan", "phantom")
            first[i] = sp["planted"] if (i // 8) % 9 == 8 else voc["desc"][sp[keys[(i // 8) % 9]]]
    if n == 5:
        first[4] = first[2]                                            # (the duplicate of the small set)
    return _rows(rng, first)


def cases(name):
    """the feature sets of a vocabulary: (kind, n)"""
    out = [("mixed", n) for n in SIZES] + [("oneword", 4096)]
    if name == "irregular":
        out += [("stopped", 257), ("stopped", 4096)]
    return out


@functools.lru_cache(maxsize=None)
def path(name, kind, n):
    return RV.paths(vocabulary(name), features(name, kind, n))


@functools.lru_cache(maxsize=None)
def want(name, kind, n, levelsup):
    """the restatement's answer (the vectorised form; tests/test_vocab_ref.py holds it against the literal one), computed once"""
    return RV.vectorised(vocabulary(name), features(name, kind, n), levelsup, path(name, kind, n))


def check(res, w, tag):
    """one frame's outputs (full-length arrays) against the restatement: integers equal, doubles equal bit for bit"""
    n = len(w["word"])
    nw = w["n_words"]
    bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)
    assert np.array_equal(res["word"], w["word"]), (tag, "word", np.nonzero(res["word"] != w["word"])[0][:8])
    assert np.array_equal(res["node_of"], w["node_of"]), (tag, "node_of", np.nonzero(res["node_of"] != w["node_of"])[0][:8])
    assert np.array_equal(bits(res["weight"]), bits(w["weight"])), (tag, "weight")
    assert res["n_words"] == nw, (tag, res["n_words"], nw)
    assert np.array_equal(res["bow_ids"][:nw], w["bow_ids"]) and np.all(res["bow_ids"][nw:] == 0xFFFFFFFF), (tag, "bow_ids")
    assert np.array_equal(bits(res["bow_vals"][:nw]), bits(w["bow_vals"])) and np.all(bits(res["bow_vals"][nw:]) == 0), (tag, "bow_vals")
    assert len(res["word"]) == n and np.array_equal(res["nodes"], Context.nodes_pack(w["node_of"])[:Context.nodes_bytes(n)]), (tag, "nodes")


class VocabRig:
    def __init__(self, L):
        self.L, self.ctx = L, Context(nfeatures=1, max_height=32, max_width=32)
        self.dev = {}

    def close(self):
        for b, _ in self.dev.values():
            b.free()
        self.ctx.close()

    def vocab(self, name):
        """the uploaded blob of a vocabulary: (device buffer, bytes)"""
        if name not in self.dev:
            b = blob(name)
            nb = Context.vocab_bytes(len(vocabulary(name)["parent"]))
            self.dev[name] = (capi.DeviceBuffer(nb).upload(b[:nb]), nb)
        return self.dev[name]

    def run(self, name, frames, levelsup, records=False):
        """frames: B arrays float32 [n][64].  records: the rows sit in the descriptor blocks of record-sized buffers, xfh_record_bytes(n)
        apart; otherwise (n + 1) * 256 bytes apart.  Guard bytes round every output and the workspace are checked.
        -> (outputs per frame, raw bytes of the output buffer, the device buffer that holds them (the caller frees it), the layout)"""
        L, ctx = self.L, self.ctx
        B, n = len(frames), len(frames[0])
        dv, nb = self.vocab(name)
        if records:
            stride, off = int(L.xfh_record_bytes(n)), int(L.xfh_record_desc_offset(n))
        else:
            stride, off = (n + 1) * 256, 0
        host = np.full(B * stride + 64, 0x5A, np.uint8)
        for b, f in enumerate(frames):
            host[b * stride + off: b * stride + off + n * 256] = np.ascontiguousarray(f, F).view(np.uint8).ravel()
        rows = capi.DeviceBuffer(host.nbytes).upload(host)
        lay = Context.bow_transform_layout(B, n, GUARD)
        ws = guarded.Guarded(Context.bow_transform_workspace_bytes(n, B), GUARD)
        out = guarded.outputs(lay)
        ctx.bow_transform_device(B, n, dv.ptr, nb, rows.ptr + off, stride, ws.ptr, out.ptr, levelsup=levelsup, guard=GUARD)
        ctx.synchronize()
        raw = guarded.download(out, lay)
        ws.download()
        res = guarded.problems(lay.parse(raw), B)
        rows.free(); ws.free()
        return res, raw, out, lay
