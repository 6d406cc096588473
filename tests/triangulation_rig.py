"""The synthetic scene of the SearchForTriangulation tests (tests/test_triangulation_ref.py, tests/test_gpu_triangulation.py,
tests/test_gpu_triangulation_cpp.py, tools/time_triangulation.py) and one guarded run of xfh_triangulation_search_device.  Not an
extraction: KF1 (n1 = 301 keypoints) sees seeded 3-D points, each neighbour KF2_b (n2 = 515) sees some of them again from its own pose,
with the descriptor row of a true correspondence a small perturbation of KF1's unit row; the other keypoints are random.  A dozen
vocabulary nodes with the sizes the kernel can go wrong at (1, 63, 64, 65, 150 members in KF2), nodes that exist on one side only and
keypoints in no node.  Planted on purpose: duplicate rows (a tie the LATER member must win), exact copies of the query row far off the
epipolar line (the nearest candidate fails the gate), monocular and stereo keypoints within the epipole radius.  F12 and the epipole
are computed in float64 and rounded once.  No test lives here."""
import struct

import numpy as np

import guarded
import ref_frame as RF
import ref_triangulation as RT
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context

F = np.float32
N1, N2 = 301, 515
GUARD = 4096
ROLL = 37                 # (odd: a problem's own side-1 block is no multiple of the four queries of a workgroup away from the next one's)
K = dict(fx=517.3, fy=516.5, cx=318.6, cy=255.3, bf=40.0, width=640, height=480)
# (node id, members in KF2, members in KF1): ids 0, 1, above 2^21, above 2^31 and 0xFFFFFFFE; 35 resp. 20 keypoints are in no node
NODES = [(0, 1, 3), (1, 63, 40), (5, 64, 40), (9, 65, 40), ((1 << 21) + 5, 150, 60), ((1 << 31) + 7, 40, 30), (0xFFFFFFFE, 30, 20), (77, 25, 0), (1000, 0, 15),
         (123456, 20, 15), (3, 12, 10), (4, 0, 8), (42, 10, 0)]
BIG = (1 << 21) + 5       # the node that holds the keypoints planted round the epipole


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def project(X):
    return np.stack([K["fx"] * X[:, 0] / X[:, 2] + K["cx"], K["fy"] * X[:, 1] / X[:, 2] + K["cy"]], 1)


def unit_rows(rng, n):
    d = rng.randn(n, 64)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)


def uright_of(rng, xy, z, frac=1 / 3):
    """about a third of the keypoints have depth: uright = x - bf / z, the others -1"""
    ur = np.full(len(xy), -1, F)
    m = rng.rand(len(xy)) < frac
    ur[m] = (xy[m, 0] - F(K["bf"]) / z[m].astype(F)).astype(F)
    ur[m & (ur < 0)] = -1
    return ur


def keyframe1(seed):
    """KF1 at the origin: dict(node_of, xy, ur, has, desc) and the 3-D points its keypoints see"""
    rng = np.random.RandomState(seed)
    X = np.stack([rng.uniform(-2.2, 2.2, N1), rng.uniform(-1.6, 1.6, N1), rng.uniform(3.5, 9.0, N1)], 1)
    xy = project(X).astype(F)
    node_of = np.full(N1, RT.NONE, np.uint32)
    perm = rng.permutation(N1)
    p = 0
    for nid, _, m1 in NODES:
        node_of[perm[p:p + m1]] = nid; p += m1
    has = (rng.rand(N1) < 0.15).astype(np.uint8)
    return dict(node_of=node_of, xy=xy, ur=uright_of(rng, xy, X[:, 2]), has=has, desc=unit_rows(rng, N1)), X


def neighbour(seed, k1, X, frac_true):
    """KF2 with pose X2 = R X1 + t -> (dict(node_of, xy, ur, has, desc), F12[9], ep[2])"""
    rng = np.random.RandomState(seed)
    R = rot(*rng.uniform(-0.04, 0.04, 3))
    t = np.array([rng.uniform(0.25, 0.4), rng.uniform(-0.05, 0.05), rng.uniform(0.9, 1.3)])          # forward motion: the epipole is inside the image
    Km = np.array([[K["fx"], 0, K["cx"]], [0, K["fy"], K["cy"]], [0, 0, 1.0]])
    R12, t12 = R.T, -R.T @ t                                                                           # T12 = T1w * Tw2 with T1w = identity
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    F12 = (np.linalg.inv(Km.T) @ tx @ R12 @ np.linalg.inv(Km)).astype(F).reshape(9)                    # Pinhole.cpp:112, rounded once
    ep = np.array([K["fx"] * t[0] / t[2] + K["cx"], K["fy"] * t[1] / t[2] + K["cy"]]).astype(F)        # :1103-1105: C2 = T2w * Cw = t
    node_of = np.full(N2, RT.NONE, np.uint32)
    xy = np.stack([rng.uniform(10, 630, N2), rng.uniform(10, 470, N2)], 1)
    z = rng.uniform(3.0, 9.0, N2)
    desc = unit_rows(rng, N2)
    perm = rng.permutation(N2)
    p = 0
    for nid, m2, _ in NODES:
        mem2 = perm[p:p + m2]; p += m2
        node_of[mem2] = nid
        mem1 = np.nonzero(k1["node_of"] == nid)[0]
        pairs = list(zip(mem1[:int(frac_true * min(len(mem1), len(mem2)))], mem2))                    # true correspondences inside the node
        for j, (i, k) in enumerate(pairs):
            X2 = R @ X[i] + t
            xy[k] = project(X2[None])[0] + rng.uniform(-0.4, 0.4, 2)                                  # (well inside 1.96 px of the epipolar line)
            z[k] = X2[2]
            row = k1["desc"][i].astype(np.float64) + rng.uniform(0.015, 0.06) * rng.randn(64)         # DescriptorDistance about 7 .. 120
            desc[k] = (row / np.linalg.norm(row)).astype(F)
        free = [k for k in mem2[len(pairs):]]
        for j, (i, k) in enumerate(pairs[:24]):
            if not free:
                break
            f = free.pop()
            if j % 2 == 0:                                                                             # a duplicate of the true partner: equal distance, both on the line
                xy[f] = xy[k]; z[f] = z[k]; desc[f] = desc[k]
            else:                                                                                      # the query's own row, far off its epipolar line
                desc[f] = k1["desc"][i]
                xy[f] = xy[k] + np.array([7.0, 60.0])
        if nid == BIG:                                                                                 # keypoints within the epipole radius (10 px)
            for f in free[:10]:
                xy[f] = ep.astype(np.float64) + rng.uniform(-5, 5, 2)
    xy = xy.astype(F)
    ur = uright_of(rng, xy, z)
    dup = {}
    for k in range(N2):                                                                                # a duplicate keeps its original's right coordinate
        dup.setdefault((float(xy[k, 0]), float(xy[k, 1])), k)
        ur[k] = ur[dup[(float(xy[k, 0]), float(xy[k, 1]))]]
    has = (rng.rand(N2) < 0.1).astype(np.uint8)
    has[node_of == 0] = 1                                                                              # node 0's only member has a map point: NO_CANDIDATES
    return dict(node_of=node_of, xy=xy, ur=ur, has=has, desc=desc), F12, ep


class Scene:
    """KF1 and three neighbours that keep fewer and fewer of its points (n_matches differs between the problems)"""

    def __init__(self, seed=7100):
        self.k1, self.X = keyframe1(seed)
        self.k2, self.F12, self.ep = [], [], []
        for b, frac in enumerate((0.8, 0.5, 0.3)):
            k2, Fm, ep = neighbour(seed + 1 + b, self.k1, self.X, frac)
            self.k2.append(k2); self.F12.append(Fm); self.ep.append(ep)
        self._dist = {}

    def dist(self, O, b, roll=0):
        """DescriptorDistance table of KF1 (rotated by `roll` places) against neighbour b, from the C oracle, computed once"""
        if b not in self._dist:
            self._dist[b] = O.distance_i32(self.k1["desc"], self.k2[b]["desc"])
        return np.roll(self._dist[b], roll, 0) if roll else self._dist[b]

    def block(self, p):
        """problem p's OWN side-1 block: every array of KF1 rotated by p * ROLL places"""
        return {k: np.roll(v, p * ROLL, 0) for k, v in self.k1.items()}


def mono(k):
    return dict(k, ur=None)


def rgbd(cam, k):
    """the keyframe as the RGB-D constructor sees it: a depth image that holds the scene's depth under every stereo keypoint, and mvuRight
    recomputed FROM that image (ComputeStereoFromRGBD), so that the host arrays and the device's own are the same numbers"""
    img = np.zeros((int(cam["height"]), int(cam["width"])), F)
    for (x, y), ur in zip(k["xy"], k["ur"]):
        if ur >= 0 and 0 <= int(x) < img.shape[1] and 0 <= int(y) < img.shape[0] and x > ur:
            img[int(y), int(x)] = F(cam["bf"]) / (F(x) - F(ur))
    return dict(k, ur=RF.stereo(cam, k["xy"], k["xy"], img)[1]), img


def write_in(path, cam, k1, img1, k2, img2, F12, ep, flags):
    """the in.bin of tests/cpp/triangulation_test.cpp (and of tests/cpp/threads_test.cpp) for one keyframe pair from rgbd()"""
    with open(path, "wb") as f:
        f.write(struct.pack("<4i", len(k1["xy"]), len(k2["xy"]), flags, 0))
        f.write(struct.pack("<10f6i", *[float(cam[c]) for c in "fx fy cx cy k1 k2 p1 p2 k3 bf".split()], int(cam["width"]), int(cam["height"]), 0, 0, 0, 0))
        f.write(np.asarray(F12).astype(F).tobytes()); f.write(np.asarray(ep).astype(F).tobytes())
        for k, img in ((k1, img1), (k2, img2)):
            kp = np.zeros(len(k["xy"]), capi.KP_DTYPE); kp["x"] = k["xy"][:, 0]; kp["y"] = k["xy"][:, 1]; kp["size"] = 1; kp["angle"] = -1
            for a in (kp, k["desc"].astype(F), k["ur"].astype(F), k["has"].astype(np.uint8), k["node_of"].astype(np.uint32), img):
                f.write(np.ascontiguousarray(a).tobytes())


class TriRig:
    def __init__(self, L):
        self.L, self.ctx = L, Context(nfeatures=1, max_height=32, max_width=32)

    def close(self):
        self.ctx.close()

    @staticmethod
    def side(blocks, blobs=None):
        """B keyframes -> the device layouts of one side: blobs, xy, uright (None when the keyframes have none), has, descriptor rows a
        row MORE than n * 256 bytes apart, and that stride"""
        n = len(blocks[0]["xy"])
        nb = Context.nodes_bytes(n)
        blob = np.concatenate([Context.nodes_pack(k["node_of"])[:nb] if blobs is None else blobs[j] for j, k in enumerate(blocks)])
        stride = (n + 1) * 256
        desc = np.zeros((len(blocks), stride // 4), F)
        for j, k in enumerate(blocks):
            desc[j, :n * 64] = k["desc"].ravel()
        ur = None if blocks[0]["ur"] is None else np.concatenate([k["ur"] for k in blocks]).astype(F)
        return dict(n=n, blob=blob, xy=np.concatenate([k["xy"] for k in blocks]).astype(F), ur=ur, has=np.concatenate([k["has"] for k in blocks]).astype(np.uint8),
                    desc=desc, stride=stride)

    def run(self, side1, side2, F12, ep, only_stereo=False, coarse=False, th_low=RT.TH_LOW, r2=100.0, unc=1.0, blobs1=None, blobs2=None):
        """side1: ONE keyframe (shared by all problems) or B of them; side2: B keyframes; F12 / ep: B of each.
        -> (outputs per problem, raw bytes of the output buffer)"""
        B, ctx = len(side2), self.ctx
        shared = len(side1) == 1 and B >= 1
        s1, s2 = self.side(side1, blobs1), self.side(side2, blobs2)
        n1 = s1["n"]
        lay = Context.triangulation_search_layout(B, n1, GUARD)
        bufs = []

        def dev(a):
            if a is None:
                return None
            b = capi.DeviceBuffer(max(np.ascontiguousarray(a).nbytes, 16)).upload(a)
            bufs.append(b)
            return b.ptr

        out = guarded.outputs(lay)
        d1 = [dev(s1[k]) for k in ("blob", "xy", "ur", "has", "desc")]; d2 = [dev(s2[k]) for k in ("blob", "xy", "ur", "has", "desc")]
        dF, de = dev(np.stack(F12).astype(F)), dev(np.stack(ep).astype(F))
        ctx.triangulation_search_device(B, n1, s2["n"], shared, *d1, s1["stride"], *d2, s2["stride"], dF, de, out.ptr, only_stereo=only_stereo, coarse=coarse,
                                        th_low=th_low, epipole_r2=r2, unc=unc, guard=GUARD)
        ctx.synchronize()
        raw = guarded.download(out, lay)
        res = guarded.problems(lay.parse(raw), B)
        out.free()
        for b in bufs:
            b.free()
        return res, raw
