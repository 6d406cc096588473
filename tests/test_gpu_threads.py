"""The library under the reference's threading model (src/System.cc:197,214,233: LocalMapping, LoopClosing and the Viewer run beside Tracking and
enter the matcher concurrently): several host threads inside libxfeat_hip at the same time, each on a ctx of its own, and a ctx that is handed
from one thread to another.  The contract is include/xfeat_hip.h (head comment) and INTEGRATION.md section 4.

Every expected answer is built on the main thread BEFORE a thread starts, by the restatements (tests/ref_*.py) or the C oracle on the rigs' own
scenes -- the calls the first test of each tests/test_gpu_*.py makes -- and a thread compares each of its results with it field by field,
integers and bit patterns, after every iteration.  No answer is an earlier GPU result.

How the threads are run (Lanes): capi.lib() is replaced, for the duration of a run, by a proxy that (1) looks at a shared stop flag before EVERY
library call of a lane and makes none once it is set, and (2) records the time.perf_counter() interval of every library call -- ctypes releases
the GIL inside it.  The first mismatch or error stores the exception and sets the flag.  The main thread joins with a timeout; a thread that is
still alive fails the test and nothing more is run on the GPU.  For every pair of lanes at least one call of the one must intersect in time with
a call of the other, otherwise the test ran serially and fails."""
import threading
import time

import numpy as np
import pytest

import bow_rig as BR
import ref_frame as RF
import ref_fuse as RU
import ref_projection as RP
import ref_triangulation as RT
import ref_window as RW
import triangulation_rig as TR
from fuse_rig import NL, SF, FuseRig
from projection_rig import BIG, F, OUT_INT, SCALE, TUM1, cam_struct
from xfeatslam_amd import capi, synth
from xfeatslam_amd.extractor import Context

pytestmark = pytest.mark.gpu

R_ROLES, R_SAME, R_MOVE = 30, 10, 10          # iterations per thread: the three roles + extractor, one entry point from four threads, the handed-over ctx
JOIN_TIMEOUT = 180.0
NF, SEED = 1000, 901
DESC_TOL = 1e-4
HUNG = []                                     # a thread that never came back: the fixtures then leave the GPU alone


# ---- running lanes ----------------------------------------------------------------------------------------------------------
class Stopped(Exception):
    pass


class TimedLib:
    """stands in for the ctypes library while lanes run: stop flag before, interval around every call of a thread that is a lane"""

    def __init__(self, L):
        self._L, self._tl = L, threading.local()

    def enter(self, lane):
        self._tl.lane = lane

    def __getattr__(self, name):
        fn = getattr(self._L, name)
        tl = self._tl

        def call(*a):
            lane = getattr(tl, "lane", None)
            if lane is None:
                return fn(*a)
            if lane.stop.is_set():
                raise Stopped(name)
            t0 = time.perf_counter()
            r = fn(*a)
            lane.calls.append((t0, time.perf_counter()))
            return r
        setattr(self, name, call)
        return call


class Lane:
    def __init__(self, name, steps, rounds):
        self.name, self.steps, self.rounds = name, steps, rounds
        self.calls, self.error, self.done, self.stop = [], None, 0, None

    def run(self, proxy, gate):
        proxy.enter(self)
        try:
            gate.wait(JOIN_TIMEOUT)
            for _ in range(self.rounds):
                for tag, step in self.steps:
                    if self.stop.is_set():
                        return
                    step()
                self.done += 1
        except Stopped:
            pass
        except BaseException as e:                                   # a mismatch (AssertionError), an XfhError, anything else
            self.error = e
            self.stop.set()
        finally:
            proxy.enter(None)


def overlaps(a, b):
    """pairs (call of a, call of b) whose intervals intersect; both lists are in start order and the calls of one lane do not overlap each other"""
    n = j = 0
    for s, e in a:
        while j < len(b) and b[j][1] < s:
            j += 1
        k = j
        while k < len(b) and b[k][0] <= e:
            n += 1
            k += 1
    return n


def run_lanes(lanes, inline=None):
    """lanes: each on a thread of its own; inline: one more lane, run by the calling thread.  -> the smallest overlap count over all pairs"""
    every = lanes + ([inline] if inline else [])
    assert 2 <= len(every) <= 8
    stop, gate = threading.Event(), threading.Barrier(len(every))
    for ln in every:
        ln.stop = stop
    real = capi.lib()
    proxy = TimedLib(real)
    threads = [threading.Thread(target=ln.run, args=(proxy, gate), name=ln.name, daemon=True) for ln in lanes]
    capi._lib = proxy
    t0 = time.perf_counter()
    try:
        for t in threads:
            t.start()
        if inline:
            inline.run(proxy, gate)
        deadline = time.perf_counter() + JOIN_TIMEOUT
        for t in threads:
            t.join(max(0.0, deadline - time.perf_counter()))
        alive = [t.name for t in threads if t.is_alive()]
        if alive:
            stop.set()
            HUNG.append(alive)
            pytest.fail(f"threads still inside the library after {JOIN_TIMEOUT} s: {alive}; nothing more is run on the GPU")
    finally:
        capi._lib = real
    wall = time.perf_counter() - t0
    for ln in every:
        if ln.error is not None:
            raise AssertionError(f"lane {ln.name} after {ln.done} full iterations") from ln.error
    for ln in every:
        assert ln.done == ln.rounds and not stop.is_set(), (ln.name, ln.done)
    pairs = {(a.name, b.name): overlaps(a.calls, b.calls) for i, a in enumerate(every) for b in every[i + 1:]}
    print(f"{len(every)} threads, wall {wall:.2f} s, library calls per thread {[len(ln.calls) for ln in every]}, overlapping call pairs {pairs}")
    assert min(pairs.values()) >= 1, f"a pair of threads was never inside the library at the same time: {pairs}"
    return min(pairs.values())


# ---- the comparisons of tests/test_gpu_{projection,fuse,triangulation,bow}.py ---------------------------------------------------
def same_proj(res, m, tag):
    for k in OUT_INT + ("assigned", "status"):
        assert np.array_equal(res[k], m[k]), (tag, k, np.nonzero(res[k] != m[k])[0][:8])
    assert res["n_matches"] == m["n_matches"], tag


def same_fuse(res, m, tag):
    for k in ("status", "best_idx", "best_dist", "n_window", "n_tested"):
        assert np.array_equal(res[k], m[k]), (tag, k, np.nonzero(res[k] != m[k])[0][:8])
    assert res["n_fused"] == m["n_fused"], tag


def same_tri(res, m, tag):
    for k in RT.OUT:
        assert np.array_equal(res[k], m[k]), (tag, k, np.nonzero(res[k] != m[k])[0][:8])
    assert res["n_matches"] == m["n_matches"], tag


def same_bow(res, m, tag):
    for k in BR.RB.OUT + ("assigned2",):
        assert np.array_equal(res[k], m[k]), (tag, k, np.nonzero(res[k] != m[k])[0][:8])
    assert res["n_matches"] == m["n_matches"], tag


def same_proj_bits(pj, w, tag):
    act = w["act"]
    for j, a in enumerate(w["proj"]):
        assert RF.same_bits(np.ascontiguousarray(pj[act, j]), np.ascontiguousarray(a[act])), (tag, "proj", j)
    assert np.all(pj[~act] == 0), (tag, "proj of inactive queries")


# ---- expected answers: restatements on a rig's scene, computed once -----------------------------------------------------------
def want_points(rig, O, r, **kw):
    """POINTS mode on problem 0 as tests/test_gpu_projection.py::check_points models it (the device's proj equals the model's by bits)"""
    u, v, ur, st = RP.project(rig.poses[0], TUM1, rig.bounds, rig.xyz)
    act = (rig.flags & 1) != 0
    st = np.where(act, st, RP.INACTIVE).astype(np.uint8)
    return dict(act=act, proj=(u, v, ur), m=rig.model(O, 0, st, u, v, F(r), ur, **kw))


def want_given(rig, O, r):
    """GIVEN mode as tests/test_gpu_projection.py::test_given_mode: (u, v) of the model's projection, a radius per query"""
    nf = rig.nf
    u, v, ur, _ = RP.project(rig.poses[0], TUM1, rig.bounds, rig.xyz)
    rq = (F(r) + (np.random.RandomState(5).rand(nf) < 0.3).astype(F) * F(2.5)).astype(F)
    act = (rig.flags & 1) != 0
    st = np.where(act, RP.VISIBLE, RP.INACTIVE).astype(np.uint8)
    return dict(uvr=np.stack([u, v, rq], 1).astype(F), act=act, proj=(u, v, np.zeros(nf, F)), m=rig.model(O, 0, st, u, v, rq, ur))


def want_fuse(fr, O, f, th, p=0):
    """frame f with pose f and the query block of problem p, as tests/test_gpu_fuse.py::check models it"""
    blk = fr.block(p)
    u, v, ur, r, lv, st = RU.project(fr.poses[f], fr.Ow[f], TUM1, fr.bounds, th, SF, NL, blk["xyz"], blk["normals"], blk["dist"])
    act = (blk["flags"] & 1) != 0
    st = np.where(act, st, RU.INACTIVE).astype(np.uint8)
    level = np.where(act, lv, -1).astype(np.int32)
    return dict(act=act, proj=(u, v, ur), level=level, m=fr.model(O, f, st, level, u, v, r, ur, qdesc=blk["qdesc"]))


def check_fuse(res, w, tag):
    same_proj_bits(res["proj"], w, tag)
    assert np.array_equal(res["level"], w["level"]), (tag, "level")
    same_fuse(res, w["m"], tag)


def check_mnn(got, want, tag):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2], equal_nan=True), tag


def distinctive_problem(sizes, seed=8):
    rng = np.random.RandomState(seed)
    tb, _ = synth.descriptor_sets(2000, 1, noise=0.3)
    tb[11] = tb[4]; tb[12] = tb[4]; tb[100:110] = 0
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    ind = rng.randint(0, 2000, off[-1]).astype(np.int32)
    ind[off[3]:off[3] + 3] = [4, 11, 12]
    return tb, off, ind


def kp_set(kps):
    v = kps["size"] > 0
    return set(zip(kps["x"][v].astype(int).tolist(), kps["y"][v].astype(int).tolist()))


def check_extract(rec, want, tag):
    """one record against Oracle.extract, as tests/test_gpu_extract.py::test_extract_matches_oracle compares them"""
    from conftest import joined_desc_diff
    hk, hd, hnv, hmono, _ = rec
    ok, od, onv, omono = want
    assert (hnv, hmono) == (onv, omono) and kp_set(hk) == kp_set(ok), tag
    dd, ds, n = joined_desc_diff(hk, hd, ok, od)
    assert n == onv and dd < DESC_TOL and ds < 1e-6, (tag, n, onv, dd, ds)
    pad = hk["size"] == 0
    assert np.array_equal(pad, ok["size"] == 0) and np.all(hd[pad] == 0) and np.array_equal(hk[pad], ok[pad]), tag


# ---- the pool: four ctx of every kind, one per thread, and the scenes ------------------------------------------------------------
class Pool:
    def __init__(self, L, O, blob):
        self.L, self.O, self.blob = L, O, blob
        self.frs = [FuseRig(L, blob, NF, SEED) for _ in range(4)]          # each holds a projection Rig (.rig) with a ctx of its own
        self.rigs = [fr.rig for fr in self.frs]
        self.bows = [BR.BowRig(L) for _ in range(4)]
        self.tris = [TR.TriRig(L) for _ in range(4)]
        self.bscene, self.tscene = BR.Scene(), TR.Scene()
        for b in range(3):                                                 # the lazy distance tables, before any thread
            self.bscene.dist(O, 0, b); self.tscene.dist(O, b)
        a = self.rigs[0]
        for r in self.rigs[1:]:                                            # four rigs of one seed hold one scene: the answers of rig 0 are everyone's
            assert np.array_equal(a.xy, r.xy) and RF.same_bits(a.ur, r.ur) and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a.recs, r.recs))
        for fr in self.frs[1:]:
            assert np.array_equal(self.frs[0].xyz, fr.xyz) and np.array_equal(self.frs[0].qdesc, fr.qdesc) and np.array_equal(self.frs[0].flags, fr.flags)
        self._want = {}

    def want(self, key, make):
        if key not in self._want:
            self._want[key] = make()
        return self._want[key]

    def close(self):
        if HUNG:
            return
        for x in self.frs + self.bows + self.tris:
            x.close()

    # -- one step per entry point: (build the expected answer now, return the callable a thread runs) --
    def bow_device(self, t, keyframe, ratio):
        s, rig = self.bscene, self.bows[t]
        want = self.want(("bow", keyframe, ratio), lambda: s.want(self.O, 0, 0, keyframe, nn_ratio=ratio))

        def step():
            res, _, _ = rig.run([s.s1], [s.s2[0]], eligible="has" if keyframe else None, strict=keyframe, nn_ratio=ratio)
            same_bow(res[0], want, ("bow device", keyframe, ratio))
        return step

    def bow_host(self, t, keyframe, ratio):
        s, ctx = self.bscene, self.bows[t].ctx
        s1, s2 = s.s1, s.s2[0]
        want = self.want(("bow", keyframe, ratio), lambda: s.want(self.O, 0, 0, keyframe, nn_ratio=ratio))

        def step():
            h = ctx.bow_search(s1["node_of"], s1["active"], s1["desc"], s2["node_of"], s2["desc"], eligible2=s2["has"] if keyframe else None, strict_low=keyframe, nn_ratio=ratio)
            same_bow(h, want, ("bow host", keyframe, ratio))
        return step

    def tri_device(self, t, b=0):
        s, rig = self.tscene, self.tris[t]
        want = self.want(("tri", b), lambda: RT.order_free(s.dist(self.O, b), s.k1, s.k2[b], s.F12[b], s.ep[b], 0))

        def step():
            res, _ = rig.run([s.k1], [s.k2[b]], [s.F12[b]], [s.ep[b]])
            same_tri(res[0], want, ("triangulation device", b))
        return step

    def tri_host(self, t, b=1):
        s, ctx = self.tscene, self.tris[t].ctx
        k1, k2 = s.k1, s.k2[b]
        want = self.want(("tri", b), lambda: RT.order_free(s.dist(self.O, b), k1, k2, s.F12[b], s.ep[b], 0))

        def step():
            h = ctx.triangulation_search(k1["node_of"], k1["xy"], k1["has"], k1["desc"], k2["node_of"], k2["xy"], k2["has"], k2["desc"], s.F12[b], s.ep[b],
                                         uright1=k1["ur"], uright2=k2["ur"])
            same_tri(h, want, ("triangulation host", b))
        return step

    def fuse_device(self, t, B, th=3.0):
        fr = self.frs[t]
        want = [self.want(("fuse", p, th, p), lambda p=p: want_fuse(self.frs[0], self.O, p, th, p)) for p in range(B)]

        def step():
            res, _ = fr.run(B, False, th)
            for p in range(B):
                check_fuse(res[p], want[p], ("fuse device", B, p))
        return step

    def fuse_host(self, t, th=7.0):
        fr = self.frs[t]
        rg = fr.rig
        want = self.want(("fuse", 1, th, 0), lambda: want_fuse(self.frs[0], self.O, 1, th, 0))
        k = np.zeros(fr.nf, capi.KP_DTYPE); k["x"] = rg.xy[1][:, 0]; k["y"] = rg.xy[1][:, 1]

        def step():
            h = fr.ctx.fuse_search(fr.xyz, fr.normals, fr.dist, fr.qdesc, fr.flags, fr.poses[1], fr.Ow[1], cam_struct(TUM1), fr.bounds, th, fr.sf, fr.rmax, k, rg.recs[1][1],
                                   uright=rg.ur[1])
            check_fuse(h, want, "fuse host")
        return step

    def points_device(self, t, r=15.0):
        rig = self.rigs[t]
        want = self.want(("points", r), lambda: want_points(self.rigs[0], self.O, r, uright=True))

        def step():
            res, _, pj, _ = rig.run(1, capi.PROJ_POINTS, rig.xyz, rig.flags, radius=r, uright=True)
            same_proj_bits(pj[0], want, "projection points")
            same_proj(res[0], want["m"], "projection points")
        return step

    def given_device(self, t, r=15.0):
        rig = self.rigs[t]
        want = self.want(("given", r), lambda: want_given(self.rigs[0], self.O, r))

        def step():
            res, _, pj, _ = rig.run(1, capi.PROJ_GIVEN, want["uvr"], rig.flags)
            same_proj_bits(pj[0], want, "projection given")
            same_proj(res[0], want["m"], "projection given")
        return step

    def points_host(self, t, r=15.0):
        rig = self.rigs[t]
        want = self.want(("points host", r), lambda: want_points(self.rigs[0], self.O, r, skip=True, uright=True, ratio=0.9))
        k = np.zeros(rig.nf, capi.KP_DTYPE); k["x"] = rig.xy[1][:, 0]; k["y"] = rig.xy[1][:, 1]

        def step():
            h = rig.ctx.search_projection(capi.PROJ_POINTS, rig.xyz, rig.recs[0][1], rig.flags, k, rig.bounds, rig.recs[1][1], radius=r, Tcw=rig.poses[0], cam=cam_struct(TUM1),
                                          skip=rig.skip[0], uright=rig.ur[1], init_dist=BIG, nn_ratio=0.9)
            same_proj_bits(h["proj"], want, "xfh_search_projection")
            same_proj(h, want["m"], "xfh_search_projection")
        return step

    def window_host(self, t, r=15.0):
        """xfh_search_window: frame 0's descriptors at the model's projections against frame 1, with the skip mask and the right coordinates"""
        rig, a = self.rigs[t], self.rigs[0]

        def make():
            u, v, ur, _ = RP.project(a.poses[0], TUM1, a.bounds, a.xyz)
            uvr = np.stack([u, v, np.full(a.nf, r, F)], 1).astype(F)
            x, y = a.xy[1][:, 0].copy(), a.xy[1][:, 1].copy()
            off, ind = RW.csr(a.grids[1], x, y, uvr, a.bounds, skip=a.skip[0], uright=a.ur[1], ur_query=ur)
            assert np.mean(np.diff(off) >= 2) > 0.3
            return dict(uvr=uvr, urq=ur, best=self.O.best2_csr(a.recs[0][1], a.recs[1][1], off, ind, 256), n=np.diff(off))
        want = self.want(("window", r), make)
        k = np.zeros(rig.nf, capi.KP_DTYPE); k["x"] = rig.xy[1][:, 0]; k["y"] = rig.xy[1][:, 1]

        def step():
            res = rig.ctx.search_window(rig.recs[0][1], want["uvr"], k, rig.bounds, rig.recs[1][1], 256, skip=rig.skip[0], uright=rig.ur[1], ur_query=want["urq"])
            for i in range(4):
                assert np.array_equal(res[i], want["best"][i]), ("xfh_search_window", i, np.nonzero(res[i] != want["best"][i])[0][:8])
            assert np.array_equal(res[4], want["n"]), "xfh_search_window n_candidates"
        return step

    def finish_host(self, t):
        """xfh_frame_finish: frame 1's extracted keypoints through the TUM1 distortion and a seeded 16-bit depth image"""
        rig, a = self.rigs[t], self.rigs[0]
        rng = np.random.RandomState(77)
        img = rng.randint(1, 6000, (480, 640)).astype(np.uint16)
        img[rng.rand(480, 640) < 1 / 3] = 0                                 # no depth under a third of the pixels
        kps = a.recs[1][0]

        def make():
            raw = np.stack([kps["x"], kps["y"]], 1).astype(F)
            xy = RF.undistort(TUM1, raw)
            dz, ur = RF.stereo(TUM1, raw, xy, img, SCALE)
            assert (dz > 0).any() and (dz < 0).any()
            return xy, ur, dz
        want = self.want("finish", make)

        def step():
            got = rig.ctx.frame_finish(kps, cam_struct(TUM1), img, SCALE)
            for g, w, name in zip(got, want, ("xy_un", "uright", "depth")):
                assert RF.same_bits(np.ascontiguousarray(g), np.ascontiguousarray(w)), ("xfh_frame_finish", name)
        return step

    def mnn_host(self, t, n1=300, n2=260):
        ctx = self.bows[t].ctx
        d1, d2 = synth.descriptor_sets(n1, n2, noise=0.3, zero_rows=3)
        want = self.want(("mnn", n1, n2), lambda: self.O.match_mnn(d1, d2))
        assert len(want[0]) > 20
        return lambda: check_mnn(ctx.match_mnn(d1, d2), want, "xfh_match_mnn")

    def distance_host(self, t):
        ctx = self.bows[t].ctx
        d1, d2 = synth.descriptor_sets(129, 127, noise=0.5)
        want = self.want("distance", lambda: self.O.distance_i32(d1, d2))

        def step():
            got = ctx.distance_i32(d1, d2)
            assert np.array_equal(got, want), ("xfh_distance_i32", np.argwhere(got != want)[:4])
        return step

    def best2_host(self, t):
        ctx = self.bows[t].ctx
        rng = np.random.RandomState(3)
        q, tg = synth.descriptor_sets(200, 1000, noise=0.25)
        tg[7] = tg[3]
        off = np.concatenate([[0], np.cumsum(rng.randint(0, 81, 200))]).astype(np.int32)
        ind = rng.randint(0, 1000, off[-1]).astype(np.int32)
        want = self.want("best2", lambda: self.O.best2_csr(q, tg, off, ind, 256))

        def step():
            got = ctx.best2_csr(q, tg, off, ind, 256)
            for i in range(4):
                assert np.array_equal(got[i], want[i]), ("xfh_best2_csr", i)
        return step

    def distinctive_host(self, t, sizes=(0, 1, 2, 3, 63, 64, 65, 128)):
        ctx = self.bows[t].ctx
        tb, off, ind = distinctive_problem(list(sizes))
        want = self.want(("distinctive", sizes), lambda: self.O.distinctive_csr(tb, off, ind))

        def step():
            got = ctx.distinctive_csr(tb, off, ind)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "xfh_distinctive_csr"
        return step


@pytest.fixture(scope="module")
def pool(gpu_lib, oracle_mod, weights_dense):
    p = Pool(gpu_lib, oracle_mod, weights_dense[1])
    yield p
    p.close()


# ---- a. Tracking, LocalMapping, LoopClosing and an extractor -------------------------------------------------------------------
def test_three_slam_threads_and_an_extractor(pool, oracle_mod, weights_std):
    """Four threads leave one barrier, each with rigs and ctx of its own, R_ROLES iterations each:
    Tracking     SearchByProjection (POINTS, radius 15, with right coordinates), match (300 x 260 rows, three of them zero), SearchByBoW in the frame form
    LocalMapping SearchForTriangulation on the first neighbour, Fuse on two keyframes at once, ComputeDistinctiveDescriptors on groups of 0 .. 128 rows
    LoopClosing  SearchByBoW in the keyframe form (nn_ratio 0.9), SearchByProjection (GIVEN), SearchByBoW through the host-pointer form
    Extractor    extract_batch of 8 frames of 96 x 128, 256 features, against Oracle.extract frame by frame"""
    p = pool
    H, W, nf, B = 96, 128, 256, 8
    frames = synth.frames(B, H, W, seed=42)
    orc = oracle_mod.Oracle(weights_std[1])
    want_recs = [orc.extract(frames[b], nf) for b in range(B)]
    assert all(w[2] > 0 for w in want_recs)
    ectx = Context(nfeatures=nf, max_height=H, max_width=W, max_batch=B)
    ectx.load_weights(weights_std[1])

    def extract():
        recs = ectx.extract_batch(frames)
        for b in range(B):
            check_extract(recs[b], want_recs[b], ("extract", b))

    lanes = [Lane("Tracking", [("projection", p.points_device(0)), ("match", p.mnn_host(0)), ("bow frame", p.bow_device(0, False, 0.6))], R_ROLES),
             Lane("LocalMapping", [("triangulation", p.tri_device(1)), ("fuse", p.fuse_device(1, 2)), ("distinctive", p.distinctive_host(1))], R_ROLES),
             Lane("LoopClosing", [("bow keyframe", p.bow_device(2, True, 0.9)), ("projection given", p.given_device(2)), ("bow host", p.bow_host(2, False, 0.6))], R_ROLES),
             Lane("Extractor", [("extract", extract)], R_ROLES)]
    try:
        run_lanes(lanes)
    finally:
        if not HUNG:
            ectx.close()


# ---- b. one entry point from four threads ----------------------------------------------------------------------------------------
ENTRY_POINTS = {
    "xfh_bow_search_device": lambda p, t: p.bow_device(t, False, 0.6),
    "xfh_triangulation_search_device": lambda p, t: p.tri_device(t),
    "xfh_fuse_search_device": lambda p, t: p.fuse_device(t, 1),
    "xfh_search_projection_device": lambda p, t: p.points_device(t),
    "xfh_match_mnn": lambda p, t: p.mnn_host(t),
    "xfh_distance_i32": lambda p, t: p.distance_host(t),
    "xfh_best2_csr": lambda p, t: p.best2_host(t),
    "xfh_search_window": lambda p, t: p.window_host(t),
    "xfh_frame_finish": lambda p, t: p.finish_host(t),
    "xfh_search_projection": lambda p, t: p.points_host(t),
    "xfh_distinctive_csr": lambda p, t: p.distinctive_host(t),
    "xfh_bow_search": lambda p, t: p.bow_host(t, True, 0.9),
    "xfh_triangulation_search": lambda p, t: p.tri_host(t),
    "xfh_fuse_search": lambda p, t: p.fuse_host(t),
}


@pytest.mark.parametrize("entry", list(ENTRY_POINTS))
def test_same_entry_point_from_four_threads(pool, entry):
    """four threads, four ctx, the SAME problem R_SAME times each: state that one capi_*.cpp kept per process rather than per ctx (a static
    buffer, a counter, an error read on the wrong thread) is shared by exactly these calls, and every result still equals the restatement"""
    run_lanes([Lane(f"{entry}#{t}", [(entry, ENTRY_POINTS[entry](pool, t))], R_SAME) for t in range(4)])


# ---- c. a ctx that moves between threads ---------------------------------------------------------------------------------------
def test_ctx_moves_between_threads(pool, weights_dense):
    """System constructs the extractor on one thread and calls it from another: one caller at a time, not always the same thread.  A ctx is
    created, loaded and used once on the main thread; a worker then runs SearchByBoW and SearchForTriangulation (device forms) on it R_MOVE
    times while the main thread works on a second ctx; after the join the main thread uses the first ctx again."""
    p = pool
    bow, tri = BR.BowRig(p.L), TR.TriRig(p.L)
    tri.ctx.close()
    tri.ctx = bow.ctx                                                      # ONE ctx under both rigs
    moved = Pool.__new__(Pool)
    moved.__dict__.update(L=p.L, O=p.O, bscene=p.bscene, tscene=p.tscene, bows=[bow], tris=[tri], _want=p._want)
    try:
        bow.ctx.load_weights(weights_dense[1])
        steps = [("bow", moved.bow_device(0, True, 0.9)), ("triangulation", moved.tri_device(0, 2))]
        for _, step in steps:                                              # used once where it was made
            step()
        run_lanes([Lane("worker on the moved ctx", steps, R_MOVE)],
                  inline=Lane("main on a second ctx", [("bow", p.bow_device(3, False, 0.6)), ("triangulation", p.tri_device(3, 1))], R_MOVE))
        for _, step in steps:                                              # and back on the main thread
            step()
    finally:
        if not HUNG:
            bow.close()
