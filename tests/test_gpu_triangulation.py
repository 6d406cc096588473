"""xfh_triangulation_search_device (k_triangulation_search) against the restatement tests/ref_triangulation.py on the scene and with the
guarded runs of tests/triangulation_rig.py.  Every comparison is equality of integers, field by field.  The conditions the scene is
chosen for (every status, ties the later member wins, a nearest candidate that fails the gate, epipole rejections, the node sizes) are
asserted where the seeds are chosen, on the CPU (tests/test_triangulation_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import ref_triangulation as RT
import triangulation_rig as TR
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context, ORBmatcher

pytestmark = pytest.mark.gpu

F = np.float32
KEYS = RT.OUT + ("n_matches",)


def same(res, m, tag, only=None):
    for k in RT.OUT:
        a, b = (res[k], m[k]) if only is None else (res[k][only], m[k][only])
        assert np.array_equal(a, b), (tag, k, np.nonzero(a != b)[0][:8])
    if only is None:
        assert res["n_matches"] == m["n_matches"], tag


@pytest.fixture(scope="module")
def scene():
    return TR.Scene()


@pytest.fixture(scope="module")
def rig(gpu_lib):
    r = TR.TriRig(gpu_lib)
    yield r
    r.close()


def test_one_problem_every_flag(rig, scene, oracle_mod):
    s = scene
    for b in (0, 2):
        for only_stereo, coarse in ((False, False), (True, False), (False, True), (True, True)):
            flags = (RT.ONLY_STEREO if only_stereo else 0) | (RT.COARSE if coarse else 0)
            res, raw = rig.run([s.k1], [s.k2[b]], [s.F12[b]], [s.ep[b]], only_stereo=only_stereo, coarse=coarse)
            m = RT.order_free(s.dist(oracle_mod, b), s.k1, s.k2[b], s.F12[b], s.ep[b], flags)
            same(res[0], m, (b, flags))
            print(f"neighbour {b} flags {flags}: statuses {np.bincount(res[0]['status'], minlength=5).tolist()}, candidates {int(res[0]['n_candidates'].sum())}, "
                  f"geom {int(res[0]['n_geom'].sum())}, matches {res[0]['n_matches']}")
            assert np.array_equal(rig.run([s.k1], [s.k2[b]], [s.F12[b]], [s.ep[b]], only_stereo=only_stereo, coarse=coarse)[1], raw)      # two runs: identical bytes
    res, _ = rig.run([TR.mono(s.k1)], [TR.mono(s.k2[0])], [s.F12[0]], [s.ep[0]])                # both uright NULL
    same(res[0], RT.order_free(s.dist(oracle_mod, 0), TR.mono(s.k1), TR.mono(s.k2[0]), s.F12[0], s.ep[0], 0), "mono")
    res, _ = rig.run([s.k1], [s.k2[0]], [s.F12[0]], [s.ep[0]], th_low=40, r2=400.0, unc=0.25)   # other scalars
    same(res[0], RT.order_free(s.dist(oracle_mod, 0), s.k1, s.k2[0], s.F12[0], s.ep[0], 0, th_low=40, r2=400.0, unc=0.25), "scalars")


def test_three_problems(rig, scene, oracle_mod):
    s = scene
    res, raw = rig.run([s.k1], s.k2, s.F12, s.ep)                                              # side1_shared = 1
    lay1 = Context.triangulation_search_layout(1, TR.N1, TR.GUARD)
    for p in range(3):
        one, _ = rig.run([s.k1], [s.k2[p]], [s.F12[p]], [s.ep[p]])                             # ... equals three B = 1 calls byte for byte
        for k in KEYS:
            assert np.asarray(res[p][k]).tobytes() == np.asarray(one[0][k]).tobytes(), (p, k)
        same(res[p], RT.order_free(s.dist(oracle_mod, p), s.k1, s.k2[p], s.F12[p], s.ep[p], 0), ("shared", p))
    assert len({r["n_matches"] for r in res}) == 3
    assert np.array_equal(rig.run([s.k1], s.k2, s.F12, s.ep)[1], raw)                          # (the n_matches atomics and their memset too)
    blocks = [s.block(p) for p in range(3)]                                                    # own side-1 blocks, each a rotation of block 0
    own, _ = rig.run(blocks, s.k2, s.F12, s.ep)
    for p in range(3):
        same(own[p], RT.order_free(s.dist(oracle_mod, p, p * TR.ROLL), blocks[p], s.k2[p], s.F12[p], s.ep[p], 0), ("own", p))
        for k in RT.OUT:
            assert np.array_equal(np.roll(res[p][k], p * TR.ROLL), own[p][k]), (p, k)
    assert lay1["bytes"] > 0


def test_hostile_input(rig, scene, oracle_mod):
    """NaN / Inf / 1e30 in F12, ep, both xy and both uright: every output still equals the restatement, which does the same fp32
    operations.  Node blobs whose items, node_start and n_nodes were overwritten with out-of-range values: the call returns, the guard
    bytes are intact (TriRig.run checks them) and the queries of the nodes that were left alone still equal the restatement."""
    s = scene
    vals = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0, -0.0, 3.4e38], F)
    k1 = {k: v.copy() for k, v in s.k1.items()}; k2 = {k: v.copy() for k, v in s.k2[0].items()}
    for j in range(40):
        k1["xy"][7 * j + 1, j % 2] = vals[j % 8]; k2["xy"][11 * j + 3, j % 2] = vals[(j + 3) % 8]
        k1["ur"][7 * j + 2] = vals[(j + 1) % 8]; k2["ur"][11 * j + 5] = vals[(j + 5) % 8]
    d = s.dist(oracle_mod, 0)
    for t, (Fm, ep) in enumerate(((s.F12[0], s.ep[0]), (np.full(9, np.nan, F), s.ep[0]), (np.full(9, np.inf, F), np.full(2, 1e30, F)), (np.full(9, 1e30, F), np.full(2, np.nan, F)),
                                  (np.zeros(9, F), np.array([np.inf, 0], F)), (s.F12[0] * F(1e30), s.ep[0]))):
        for coarse in (False, True):
            res, _ = rig.run([k1], [k2], [Fm], [ep], coarse=coarse)
            same(res[0], RT.order_free(d, k1, k2, Fm, ep, RT.COARSE if coarse else 0), ("floats", t, coarse))
    # blobs: bounds-checked positions only, inside the caller's buffer
    n2 = TR.N2
    nb, cap = Context.nodes_bytes(n2), (n2 + 4) & ~3
    good = Context.nodes_pack(s.k2[0]["node_of"])[:nb]
    nid, ns, items = Context.nodes_unpack(good, n2)
    want = RT.order_free(d, s.k1, s.k2[0], s.F12[0], s.ep[0], 0)
    NS, IT = 16 + cap, 16 + 2 * cap
    hit, last = int(np.nonzero(nid == 9)[0][0]), len(nid) - 1                                  # node 9 (65 members) and the node with the largest id
    bad = good.copy(); w = bad.view(np.int32)
    w[IT + ns[hit]: IT + ns[hit + 1]] = np.resize(np.array([n2, -1, 1 << 30, -(1 << 31), n2 + 5, 0x7fffffff], np.int64), ns[hit + 1] - ns[hit]).astype(np.int32)
    w[NS + last + 1] = 1 << 30                                                                 # the last node's end: clamped to n2
    res, _ = rig.run([s.k1], [s.k2[0]], [s.F12[0]], [s.ep[0]], blobs2=[bad])
    touched = np.isin(s.k1["node_of"], [9, int(nid[last])])
    assert touched.sum() >= 40 and (~touched).sum() >= 200
    same(res[0], want, "blob items", only=~touched)
    assert np.all(res[0]["n_candidates"][s.k1["node_of"] == 9] == 0)                           # every item of node 9 is out of range: none is a candidate
    for val in (1 << 30, -5, n2 + 1):                                                          # n_nodes itself: clamped; the id list is then no longer what was searched
        bad = good.copy(); bad.view(np.int32)[2] = val
        res, _ = rig.run([s.k1], [s.k2[0]], [s.F12[0]], [s.ep[0]], blobs2=[bad])
        inactive = want["status"] == RT.INACTIVE
        assert np.array_equal(res[0]["status"][inactive], want["status"][inactive]) and np.all(res[0]["status"] <= RT.MATCHED)
        assert np.all((res[0]["match12"] >= -1) & (res[0]["match12"] < n2))
    bad1 = Context.nodes_pack(s.k1["node_of"])[:Context.nodes_bytes(TR.N1)].copy()             # side 1: only node_of is read; garbage elsewhere changes nothing
    bad1.view(np.int32)[2:16 + 3 * ((TR.N1 + 4) & ~3)] = 1 << 30
    res, _ = rig.run([s.k1], [s.k2[0]], [s.F12[0]], [s.ep[0]], blobs1=[bad1])
    same(res[0], want, "blob 1")


def test_host_form_and_hand_made_cases(rig, scene, oracle_mod):
    s = scene
    for b, kw in ((1, dict()), (0, dict(only_stereo=True)), (2, dict(coarse=True, th_low=60, epipole_r2=50.0, unc=2.0))):
        k1, k2 = s.k1, s.k2[b]
        h = rig.ctx.triangulation_search(k1["node_of"], k1["xy"], k1["has"], k1["desc"], k2["node_of"], k2["xy"], k2["has"], k2["desc"], s.F12[b], s.ep[b],
                                         uright1=k1["ur"], uright2=k2["ur"], **kw)
        dk = dict(kw); r2 = dk.pop("epipole_r2", 100.0)
        res, _ = rig.run([k1], [k2], [s.F12[b]], [s.ep[b]], r2=r2, **dk)
        for k in KEYS:
            assert np.array_equal(h[k], res[0][k]), (b, k)
    k1, k2 = s.k1, s.k2[0]
    h = rig.ctx.triangulation_search(k1["node_of"], k1["xy"], k1["has"], k1["desc"], k2["node_of"], k2["xy"], k2["has"], k2["desc"], s.F12[0], s.ep[0])   # monocular
    same(h, RT.order_free(s.dist(oracle_mod, 0), TR.mono(k1), TR.mono(k2), s.F12[0], s.ep[0], 0), "host mono")
    n, pairs, r = ORBmatcher(ctx=rig.ctx).search_for_triangulation(k1["node_of"], k1["xy"], k1["has"], k1["desc"], k2["node_of"], k2["xy"], k2["has"], k2["desc"],
                                                                    s.F12[0], s.ep[0], uright1=k1["ur"], uright2=k2["ur"])
    lit = RT.literal(s.dist(oracle_mod, 0), k1, k2, s.F12[0], s.ep[0], 0)
    assert n == lit["n_matches"] and pairs == lit["pairs"]
    # the written-out answers of tests/test_triangulation_ref.py on the device: descriptors on one axis give the table's distances exactly
    for name, dist, k1, k2, Fm, ep, flags, want in RT.handmade():
        n1, n2 = dist.shape
        d1 = np.zeros((n1, 64), F); d2 = np.zeros((n2, 64), F)
        rows = [dist[i].tolist() for i in range(n1)]
        assert all(r == rows[0] for r in rows), name                                            # (every query sees the same distances: d2 = sqrt(dist / 512) on axis 0)
        d2[:, 0] = np.sqrt(np.array(rows[0], np.float64) / 512.0 + 1e-6).astype(F)
        assert oracle_mod.distance_i32(d1, d2).tolist() == dist.tolist(), name
        h = rig.ctx.triangulation_search(k1["node_of"], k1["xy"], k1["has"], d1, k2["node_of"], k2["xy"], k2["has"], d2, Fm, ep, uright1=k1["ur"], uright2=k2["ur"],
                                         only_stereo=bool(flags & RT.ONLY_STEREO), coarse=bool(flags & RT.COARSE))
        for key, val in want.items():
            assert h[key].tolist() == val, (name, key, h[key].tolist(), val)
        assert h["n_matches"] == want["status"].count(RT.MATCHED), name


def test_invalid_arguments_launch_nothing(rig, scene):
    L, ctx, s = rig.L, rig.ctx, scene
    n1, n2 = TR.N1, TR.N2
    lay = Context.triangulation_search_layout(1, n1)
    sent = np.full(lay["bytes"], 0xA5, np.uint8)
    out = capi.DeviceBuffer(lay["bytes"]).upload(sent)
    mk = lambda a: capi.DeviceBuffer(np.ascontiguousarray(a).nbytes + 32).upload(a)
    s1, s2 = rig.side([s.k1]), rig.side([s.k2[0]])
    bufs = {k + "1": mk(s1[k]) for k in ("blob", "xy", "ur", "has", "desc")}
    bufs.update({k + "2": mk(s2[k]) for k in ("blob", "xy", "ur", "has", "desc")})
    bufs["F"], bufs["ep"] = mk(s.F12[0]), mk(s.ep[0])
    base = dict(ctx=ctx.h, B=1, n1=n1, n2=n2, shared=1, flags=0, low=100, r2=100.0, unc=1.0, blob1=bufs["blob1"].ptr, xy1=bufs["xy1"].ptr, ur1=bufs["ur1"].ptr,
                has1=bufs["has1"].ptr, desc1=bufs["desc1"].ptr, st1=s1["stride"], blob2=bufs["blob2"].ptr, xy2=bufs["xy2"].ptr, ur2=bufs["ur2"].ptr, has2=bufs["has2"].ptr,
                desc2=bufs["desc2"].ptr, st2=s2["stride"], F=bufs["F"].ptr, ep=bufs["ep"].ptr, st=out.ptr + lay["status"], m=out.ptr + lay["match12"],
                bd=out.ptr + lay["best_dist"], nc=out.ptr + lay["n_candidates"], ng=out.ptr + lay["n_geom"], nm=out.ptr + lay["n_matches"])

    def call(**kw):
        a = dict(base); a.update(kw)
        return L.xfh_triangulation_search_device(*[a[k] for k in base])

    nan, inf = float("nan"), float("inf")
    bad = [dict(B=0), dict(B=-1), dict(B=65536), dict(n1=0), dict(n1=-1), dict(n1=capi.GRID_MAX_N + 1), dict(n2=0), dict(n2=capi.GRID_MAX_N + 1), dict(shared=2), dict(shared=-1),
           dict(flags=4), dict(flags=-1), dict(flags=8), dict(r2=nan), dict(r2=inf), dict(r2=-inf), dict(unc=nan), dict(unc=inf),
           dict(desc1=base["desc1"] + 4), dict(desc2=base["desc2"] + 8), dict(st1=s1["stride"] + 4), dict(st2=s2["stride"] + 8), dict(blob1=base["blob1"] + 8),
           dict(blob2=base["blob2"] + 4), dict(xy1=base["xy1"] + 2), dict(xy2=base["xy2"] + 1), dict(ur1=base["ur1"] + 2), dict(ur2=base["ur2"] + 2), dict(F=base["F"] + 2),
           dict(ep=base["ep"] + 1), dict(m=base["m"] + 2), dict(bd=base["bd"] + 1), dict(nc=base["nc"] + 2), dict(ng=base["ng"] + 2), dict(nm=base["nm"] + 2),
           dict(ctx=None), dict(blob1=None), dict(xy1=None), dict(has1=None), dict(desc1=None), dict(blob2=None), dict(xy2=None), dict(has2=None), dict(desc2=None),
           dict(F=None), dict(ep=None), dict(st=None), dict(m=None), dict(bd=None), dict(nc=None), dict(ng=None), dict(nm=None)]
    ctx.synchronize()
    ctx.timing_enable(capi.K["TRIANGULATION_SEARCH"])
    for kw in bad:
        assert call(**kw) == 1, kw
    ctx.synchronize()
    assert ctx.timing_read()[0] == 0 and np.array_equal(out.download(np.uint8, lay["bytes"]), sent)
    assert call() == 0 and call(shared=0) == 0 and call(ur1=None) == 0 and call(ur2=None, flags=3) == 0        # the valid calls still work afterwards
    ctx.synchronize()
    assert ctx.timing_read()[0] == 4 and not np.array_equal(out.download(np.uint8, lay["bytes"]), sent)
    ctx.timing_enable(capi.K["NONE"])
    # the host form refuses the same classes before it stages anything
    k1, k2 = s.k1, s.k2[0]
    keep = [np.ascontiguousarray(a) for a in (k1["node_of"], k1["xy"], k1["ur"], k1["has"], k1["desc"], k2["node_of"], k2["xy"], k2["ur"], k2["has"], k2["desc"], s.F12[0], s.ep[0])]
    houts = {n: np.full(n1 * w, 0xA5, np.uint8) for n, w in (("st", 1), ("m", 4), ("bd", 4), ("nc", 4), ("ng", 4))}
    houts["nm"] = np.full(4, 0xA5, np.uint8)
    names = ("no1", "xy1", "ur1", "has1", "desc1", "no2", "xy2", "ur2", "has2", "desc2", "F", "ep")
    hb = dict(ctx=ctx.h, n1=n1, n2=n2, flags=0, low=100, r2=100.0, unc=1.0, **{n: a.ctypes.data for n, a in zip(names, keep)}, **{n: a.ctypes.data for n, a in houts.items()})

    def hcall(**kw):
        a = dict(hb); a.update(kw)
        return L.xfh_triangulation_search(*[a[k] for k in hb])

    hbad = [dict(ctx=None), dict(n1=0), dict(n1=capi.GRID_MAX_N + 1), dict(n2=0), dict(n2=-3), dict(flags=4), dict(flags=-1), dict(r2=nan), dict(unc=inf)] + \
           [{n: None} for n in names if n not in ("ur1", "ur2")] + [{n: None} for n in houts]
    ctx.timing_enable(capi.K["TRIANGULATION_SEARCH"])
    for kw in hbad:
        assert hcall(**kw) == 1, kw
    assert ctx.timing_read()[0] == 0 and all(np.all(a == 0xA5) for a in houts.values())
    assert hcall() == 0 and hcall(ur1=None, ur2=None) == 0
    assert ctx.timing_read()[0] == 2 and not any(np.all(a == 0xA5) for a in houts.values())
    ctx.timing_enable(capi.K["NONE"])
    for x in [out] + list(bufs.values()):
        x.free()
