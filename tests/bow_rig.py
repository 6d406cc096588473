"""The synthetic scene of the SearchByBoW tests (tests/test_bow_ref.py, tests/test_gpu_bow.py, tests/test_gpu_bow_cpp.py) and one guarded run
of xfh_bow_search_device.  Not an extraction: side 1 (n1 = 390 keypoints, the keyframe whose map points are matched) and three versions
of side 2 (n2 = 515) that keep fewer and fewer of its rows; a true correspondence is a row at a chosen DescriptorDistance from the query's
unit row, the other rows are random (distance about 1000, above init_dist).  The node ids and side-2 sizes are those of
triangulation_rig.NODES (1, 63, 64, 65, 150 members, ids at the ends of the uint32 range, one-sided nodes, keypoints in no node); the
side-1 sizes are 1, 64, 65 and 135 among others.  Planted on purpose, with the queries of a group taken in stored order:
  chains      four queries on one spot and four targets at distances about 6, 14, 30, 65 from it: each query is pushed one target on
  second      a query whose two nearest are about 20 and 25 apart, and an earlier query that sits on the second: the ratio test passes
              only after that claim
  first       a query with targets at about 10, 40 and 50 and an earlier query that sits on the first: matched becomes rejected
  pile-up     45 queries of the 150-member node on one spot, 30 targets at distances about 7 .. 82 from it: the i-th query finds about i
              claimed entries ahead (with nn_ratio = 1.5, where every one of them is accepted)
  duplicates  pairs of identical target rows at about 10 from their query
The problems of a batch: side-1 block p is block 0 rotated by p * ROLL places with its own active bytes.  No test lives here."""
import struct

import numpy as np

import guarded
import ref_bow as RB
import triangulation_rig as TR
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context

F = np.float32
N1, N2 = 390, TR.N2
GUARD = 4096
ROLL = 37
M1 = {0: 3, 1: 64, 5: 65, 9: 1, TR.BIG: 135, (1 << 31) + 7: 30, 0xFFFFFFFE: 20, 77: 0, 1000: 15, 123456: 15, 3: 10, 4: 8, 42: 0}
NODES = [(nid, m2, M1[nid]) for nid, m2, _ in TR.NODES]   # (node id, members on side 2, members on side 1)
INELIGIBLE = 123456                                        # the node whose side-2 members have no map point (keyframe form)


def unit(v):
    return v / np.linalg.norm(v)


def at_distance(rng, row, d):
    """a unit row whose DescriptorDistance from `row` is about d: 512 * |s u|^2 = d for a unit direction u"""
    return unit(row.astype(np.float64) + np.sqrt(d / 512.0) * unit(rng.randn(64))).astype(F)


def side1(seed):
    rng = np.random.RandomState(seed)
    node_of = np.full(N1, RB.NONE, np.uint32)
    perm = rng.permutation(N1)
    p = 0
    for nid, _, m1 in NODES:
        node_of[perm[p:p + m1]] = nid; p += m1
    return dict(node_of=node_of, desc=TR.unit_rows(rng, N1), active=(rng.rand(N1) < 0.9).astype(np.uint8))


def plant(rng, s1, desc2, q, t, what):
    """q: queries of one node in stored order (their rows are rewritten), t: free targets of the node -> the targets used"""
    d1 = s1["desc"]
    if what == "chain":
        spot = d1[q[0]].copy()
        for j, i in enumerate(q[:4]):
            d1[i] = at_distance(rng, spot, 0.3)
        for j, d in enumerate((6, 14, 30, 65)):
            desc2[t[j]] = at_distance(rng, spot, d)
        return 4, 4
    if what == "second":                                   # q[0] sits on the second best of q[1]
        desc2[t[0]] = at_distance(rng, d1[q[1]], 20); desc2[t[1]] = at_distance(rng, d1[q[1]], 25)
        d1[q[0]] = at_distance(rng, desc2[t[1]], 0.3)
        return 2, 2
    if what == "first":                                    # q[0] sits on the best of q[1]
        for j, d in enumerate((10, 40, 50)):
            desc2[t[j]] = at_distance(rng, d1[q[1]], d)
        d1[q[0]] = at_distance(rng, desc2[t[0]], 0.3)
        return 2, 3
    if what == "pileup":
        spot = d1[q[0]].copy()
        for i in q[:45]:
            d1[i] = at_distance(rng, spot, 0.5)
        for j in range(30):
            desc2[t[j]] = at_distance(rng, spot, 7 + 75.0 * j / 29)
        return 45, 30
    if what == "dup":
        desc2[t[0]] = at_distance(rng, d1[q[0]], 10); desc2[t[1]] = desc2[t[0]]
        return 1, 2
    raise ValueError(what)


PLAN = {1: ["chain", "second", "dup"], 5: ["first", "chain", "dup", "dup"], TR.BIG: ["pileup", "second", "first"], (1 << 31) + 7: ["dup", "chain"]}


def side2(seed, s1, frac_true, first):
    """a version of side 2 for side-1 block 0 (`first`: the one that also rewrites the planted queries' rows)"""
    rng = np.random.RandomState(seed)
    node_of = np.full(N2, RB.NONE, np.uint32)
    desc = TR.unit_rows(rng, N2)
    has = (rng.rand(N2) < 0.85).astype(np.uint8)
    perm = rng.permutation(N2)
    p = 0
    prng = np.random.RandomState(991)                      # the planted groups are the same in every version
    for nid, m2, _ in NODES:
        mem2 = np.sort(perm[p:p + m2]); p += m2
        node_of[mem2] = nid
        q = list(np.nonzero(s1["node_of"] == nid)[0]); t = list(mem2)
        for what in PLAN.get(nid, []):
            scratch = dict(s1, desc=s1["desc"] if first else s1["desc"].copy())
            nq, nt = plant(prng, scratch, desc, q, t, what)
            s1["active"][q[:nq]] = 1; has[t[:nt]] = 1
            q, t = q[nq:], t[nt:]
        for i, k in list(zip(q, t))[:int(frac_true * min(len(q), len(t)))]:
            desc[k] = at_distance(rng, s1["desc"][i], rng.uniform(5, 120))
        if nid == 0:
            has[mem2] = 1
            desc[mem2[0]] = at_distance(rng, s1["desc"][np.nonzero(s1["node_of"] == 0)[0][0]], 12)
            s1["active"][s1["node_of"] == 0] = 1
        if nid == INELIGIBLE:
            has[mem2] = 0
    return dict(node_of=node_of, desc=desc, has=has)


class Scene:
    def __init__(self, seed=8200):
        self.s1 = side1(seed)
        self.s2 = [side2(seed + 1 + b, self.s1, frac, b == 0) for b, frac in enumerate((0.9, 0.55, 0.25))]
        rng = np.random.RandomState(seed + 9)
        self.blocks = [self.s1]
        for p, keep in ((1, 0.6), (2, 0.35)):              # own side-1 blocks: rotations of block 0 with fewer active queries
            blk = {k: np.roll(v, p * ROLL, 0) for k, v in self.s1.items()}
            blk["active"] = (blk["active"] & (rng.rand(N1) < keep)).astype(np.uint8)
            self.blocks.append(blk)
        self._dist = {}

    def dist(self, O, p, b):
        """DescriptorDistance table of side-1 block p against side-2 version b, from the C oracle, computed once per version"""
        if b not in self._dist:
            self._dist[b] = O.distance_i32(self.s1["desc"], self.s2[b]["desc"])
        return np.roll(self._dist[b], p * ROLL, 0) if p else self._dist[b]

    def want(self, O, p, b, keyframe=False, **kw):
        """the restatement's answer for (block p, version b) in the frame or the keyframe form"""
        s1, s2 = self.blocks[p], self.s2[b]
        return RB.per_node(self.dist(O, p, b), s1["node_of"], s1["active"], s2["node_of"], s2["has"] if keyframe else None, RB.STRICT_LOW if keyframe else 0, **kw)

    def th_low(self, O):
        """a th_low taken from the scene's own distances: the largest best distance of a query that is matched in both forms at th_low = 100"""
        a, k = self.want(O, 0, 0, False), self.want(O, 0, 0, True)
        both = np.nonzero((a["status"] == RB.MATCHED) & (k["status"] == RB.MATCHED) & (a["best_dist"] == k["best_dist"]) & (a["best_dist"] >= 40))[0]
        return int(a["best_dist"][both].max())


def write_in(path, s1, s2, keyframe, ratio):
    """the in.bin of tests/cpp/bow_test.cpp (and of tests/cpp/threads_test.cpp) for one problem: side 1 with its active bytes, side 2 with its
    has-a-map-point bytes"""
    with open(path, "wb") as f:
        f.write(struct.pack("<4if", len(s1["node_of"]), len(s2["node_of"]), int(keyframe), 0, ratio))
        for k, flag in ((s1, "active"), (s2, "has")):
            for a in (k["desc"].astype(F), k["node_of"].astype(np.uint32), k[flag].astype(np.uint8)):
                f.write(np.ascontiguousarray(a).tobytes())


class BowRig:
    def __init__(self, L):
        self.L, self.ctx = L, Context(nfeatures=1, max_height=32, max_width=32)

    def close(self):
        self.ctx.close()

    @staticmethod
    def side(blocks, flag, blobs=None):
        """B keyframes -> the device layouts of one side: blobs, flag bytes (None: the pointer is NULL), descriptor rows a row MORE than
        n * 256 bytes apart, and that stride"""
        n = len(blocks[0]["node_of"])
        nb = Context.nodes_bytes(n)
        blob = np.concatenate([Context.nodes_pack(k["node_of"])[:nb] if blobs is None else blobs[j] for j, k in enumerate(blocks)])
        stride = (n + 1) * 256
        desc = np.zeros((len(blocks), stride // 4), F)
        for j, k in enumerate(blocks):
            desc[j, :n * 64] = k["desc"].ravel()
        fl = None if flag is None else np.concatenate([np.asarray(k[flag], np.uint8) for k in blocks])
        return dict(n=n, blob=blob, flag=fl, desc=desc, stride=stride)

    def run(self, side1, side2, B=None, eligible=None, strict=False, nn_ratio=0.6, th_low=RB.TH_LOW, init_dist=RB.INIT, blobs1=None, blobs2=None):
        """side1 / side2: lists of ONE block (shared by all problems) or B of them; eligible: None (NULL), "has" or "ones".
        -> (outputs per problem, raw bytes of the output buffer, workspace counters [B][4])"""
        B = B or max(len(side1), len(side2))
        assert len(side1) in (1, B) and len(side2) in (1, B)
        shared = 0 if len(side1) == len(side2) == B else (1 if len(side1) == 1 else 2)
        if eligible == "ones":
            side2 = [dict(k, ones=np.ones(len(k["node_of"]), np.uint8)) for k in side2]
        s1, s2 = self.side(side1, "active", blobs1), self.side(side2, eligible, blobs2)
        n1, n2, ctx = s1["n"], s2["n"], self.ctx
        lay = Context.bow_search_layout(B, n1, n2, GUARD)
        bufs = []

        def dev(a):
            if a is None:
                return None
            b = capi.DeviceBuffer(max(np.ascontiguousarray(a).nbytes, 16)).upload(a)
            bufs.append(b)
            return b.ptr

        ws = guarded.Guarded(Context.bow_search_workspace_bytes(n1, n2, B), GUARD)
        out = guarded.outputs(lay)
        d1 = [dev(s1[k]) for k in ("blob", "flag", "desc")]; d2 = [dev(s2[k]) for k in ("blob", "flag", "desc")]
        ctx.bow_search_device(B, n1, n2, shared, *d1, s1["stride"], *d2, s2["stride"], ws.ptr, out.ptr, strict_low=strict, init_dist=init_dist,
                              th_low=th_low, nn_ratio=nn_ratio, guard=GUARD)
        ctx.synchronize()
        raw = guarded.download(out, lay)
        counters = ws.download()[:16 * B].view(np.int32).reshape(B, 4)
        res = guarded.problems(lay.parse(raw), B)
        out.free(); ws.free()
        for b in bufs:
            b.free()
        return res, raw, counters
