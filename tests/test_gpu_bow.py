"""xfh_bow_search_device (k_bow_candidates, k_bow_resolve) against the restatement tests/ref_bow.py on the scene and with the guarded runs
of tests/bow_rig.py.  Every comparison is equality of integers, field by field, assigned2 and n_matches included.  The conditions the
scene is chosen for (claims that move a query, chains, ratio tests that flip after a claim, the pile-up that exhausts the candidate
lists, duplicates, best == th_low, single candidates, nodes without eligible targets) are asserted where the seeds are chosen, on the CPU
(tests/test_bow_ref.py)."""
import numpy as np
import pytest

import bow_rig as BR
import ref_bow as RB
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context, ORBmatcher

pytestmark = pytest.mark.gpu

F = np.float32
KEYS = RB.OUT + ("assigned2", "n_matches")
RATIOS = (0.6, 0.9, 1.5)


def same(res, m, tag, only=None):
    for k in RB.OUT:
        a, b = (res[k], m[k]) if only is None else (res[k][only], m[k][only])
        assert np.array_equal(a, b), (tag, k, np.nonzero(a != b)[0][:8])
    if only is None:
        assert np.array_equal(res["assigned2"], m["assigned2"]), (tag, "assigned2", np.nonzero(res["assigned2"] != m["assigned2"])[0][:8])
        assert res["n_matches"] == m["n_matches"], tag


@pytest.fixture(scope="module")
def scene():
    return BR.Scene()


@pytest.fixture(scope="module")
def rig(gpu_lib):
    r = BR.BowRig(gpu_lib)
    yield r
    r.close()


def test_both_forms_every_ratio(rig, scene, oracle_mod):
    s = scene
    for keyframe in (False, True):
        for ratio in RATIOS:
            st = RB.new_stats()
            want = s.want(oracle_mod, 0, 0, keyframe, nn_ratio=ratio, stats=st)
            res, raw, cnt = rig.run([s.s1], [s.s2[0]], eligible="has" if keyframe else None, strict=keyframe, nn_ratio=ratio)
            same(res[0], want, (keyframe, ratio))
            print(f"keyframe form {keyframe} nn_ratio {ratio}: statuses {np.bincount(res[0]['status'], minlength=5).tolist()}, matches {res[0]['n_matches']}, "
                  f"full re-searches {int(cnt[0, 0])} (the restatement expects {st['runs_out']}), queries resolved {int(cnt[0, 1])}, nodes {int(cnt[0, 2])}")
            assert int(cnt[0, 0]) == st["runs_out"] and int(cnt[0, 1]) == int((want["status"] >= RB.NO_CANDIDATES).sum())
            assert np.array_equal(rig.run([s.s1], [s.s2[0]], eligible="has" if keyframe else None, strict=keyframe, nn_ratio=ratio)[1], raw)    # two runs: identical bytes
    # eligible2 = NULL against all-ones, in both threshold forms
    for strict in (False, True):
        a, _, _ = rig.run([s.s1], [s.s2[1]], eligible=None, strict=strict, nn_ratio=0.9)
        b, _, _ = rig.run([s.s1], [s.s2[1]], eligible="ones", strict=strict, nn_ratio=0.9)
        for k in KEYS:
            assert np.array_equal(a[0][k], b[0][k]), (strict, k)
        same(a[0], RB.per_node(s.dist(oracle_mod, 0, 1), s.s1["node_of"], s.s1["active"], s.s2[1]["node_of"], None, int(strict), nn_ratio=0.9), ("null", strict))
    # a th_low that IS a best distance of the scene: matched in the frame form, rejected under XFH_BOW_STRICT_LOW; and other scalars
    th = s.th_low(oracle_mod)
    for keyframe in (False, True):
        res, _, _ = rig.run([s.s1], [s.s2[0]], eligible="has" if keyframe else None, strict=keyframe, th_low=th)
        same(res[0], s.want(oracle_mod, 0, 0, keyframe, th_low=th), ("th_low", th, keyframe))
    res, _, _ = rig.run([s.s1], [s.s2[0]], nn_ratio=0.75, th_low=40, init_dist=120)
    same(res[0], s.want(oracle_mod, 0, 0, False, nn_ratio=0.75, th_low=40, init_dist=120), "scalars")
    res, _, _ = rig.run([s.s1], [s.s2[0]], eligible="has", strict=True, nn_ratio=1.5, th_low=300, init_dist=0x7fffffff)
    same(res[0], s.want(oracle_mod, 0, 0, True, nn_ratio=1.5, th_low=300, init_dist=0x7fffffff), "no initial bound")


def test_three_problems_every_sharing(rig, scene, oracle_mod):
    s = scene
    for shared, side1, side2, pairs in ((1, [s.blocks[0]], s.s2, ((0, 0), (0, 1), (0, 2))), (2, s.blocks, [s.s2[0]], ((0, 0), (1, 0), (2, 0))),
                                        (0, s.blocks, s.s2, ((0, 0), (1, 1), (2, 2)))):
        for keyframe, ratio in ((False, 0.6), (True, 1.5)):
            kw = dict(eligible="has" if keyframe else None, strict=keyframe, nn_ratio=ratio)
            res, raw, _ = rig.run(side1, side2, B=3, **kw)
            for j, (p, b) in enumerate(pairs):
                one, _, _ = rig.run([s.blocks[p]], [s.s2[b]], **kw)                            # ... equals three B = 1 calls byte for byte
                for k in KEYS:
                    assert np.asarray(res[j][k]).tobytes() == np.asarray(one[0][k]).tobytes(), (shared, j, k)
                same(res[j], s.want(oracle_mod, p, b, keyframe, nn_ratio=ratio), (shared, j))
            assert len({r["n_matches"] for r in res}) == 3, shared
            assert np.array_equal(rig.run(side1, side2, B=3, **kw)[1], raw)                    # (the n_matches atomics and the memsets too)


def test_hostile_blobs(rig, scene, oracle_mod):
    """Node blobs whose items, node_start and n_nodes were overwritten with out-of-range values -- the blobs tests/cpp/asan_bow_test.cpp
    walks on the CPU through the kernels' own clamping lines: the call returns, the guard bytes round the outputs and the workspace are
    intact (BowRig.run checks them) and the queries of the nodes that were left alone still equal the restatement."""
    s = scene
    n1, n2 = BR.N1, BR.N2
    want = s.want(oracle_mod, 0, 0, False, nn_ratio=0.9)
    vals = np.array([0, -1, 1 << 30, -(1 << 31), 5, 0x7fffffff], np.int64)
    for side, n, no in ((2, n2, s.s2[0]["node_of"]), (1, n1, s.s1["node_of"])):
        nb, cap = Context.nodes_bytes(n), (n + 4) & ~3
        good = Context.nodes_pack(no)[:nb]
        nid, ns, items = Context.nodes_unpack(good, n)
        NS, IT = 16 + cap, 16 + 2 * cap
        hit, last = int(np.nonzero(nid == 5)[0][0]), len(nid) - 1                              # node 5 and the node with the largest id
        bad = good.copy(); w = bad.view(np.int32)
        w[IT + ns[hit]: IT + ns[hit + 1]] = np.resize(vals + np.array([n, 0, 0, 0, n, 0]), ns[hit + 1] - ns[hit]).astype(np.int32)
        w[NS + last + 1] = 1 << 30                                                             # the last node's end: clamped to n
        touched = np.isin(s.s1["node_of"], [5, int(nid[last])])
        assert touched.sum() >= 60 and (~touched).sum() >= 250
        res, _, _ = rig.run([s.s1], [s.s2[0]], nn_ratio=0.9, **{f"blobs{side}": [bad]})
        same(res[0], want, ("items", side), only=~touched)
        if side == 2:
            assert np.all(res[0]["n_candidates"][s.s1["node_of"] == 5] == 0)                   # every item of node 5 is out of range: none is a candidate
        bad = good.copy(); bad.view(np.int32)[NS + 1] = -7                                     # a negative node_start: the first two nodes change, the others do not
        res, _, _ = rig.run([s.s1], [s.s2[0]], nn_ratio=0.9, **{f"blobs{side}": [bad]})
        same(res[0], want, ("node_start", side), only=~np.isin(s.s1["node_of"], [int(nid[0]), int(nid[1])]))
        for val in (1 << 30, -5, n + 1):                                                       # n_nodes itself: clamped; the id list is then no longer what was searched
            bad = good.copy(); bad.view(np.int32)[2] = val
            res, _, _ = rig.run([s.s1], [s.s2[0]], nn_ratio=0.9, **{f"blobs{side}": [bad]})
            inactive = want["status"] == RB.INACTIVE
            assert np.array_equal(res[0]["status"][inactive], want["status"][inactive]) and np.all(res[0]["status"] <= RB.MATCHED)
            assert np.all((res[0]["match12"] >= -1) & (res[0]["match12"] < n2)) and np.all((res[0]["assigned2"] >= -1) & (res[0]["assigned2"] < n1))
    rng = np.random.RandomState(17)                                                            # blobs of random words on both sides at once
    junk = [rng.randint(-(1 << 31), 1 << 31, Context.nodes_bytes(n) // 4, dtype=np.int64).astype(np.int32).view(np.uint8) for n in (n1, n2)]
    res, _, _ = rig.run([s.s1], [s.s2[0]], blobs1=[junk[0]], blobs2=[junk[1]])
    assert np.all(res[0]["status"] <= RB.MATCHED) and np.all((res[0]["match12"] >= -1) & (res[0]["match12"] < n2))


def test_host_form_hand_made_cases_and_matcher(rig, scene, oracle_mod):
    s = scene
    s1, s2 = s.s1, s.s2[0]
    for keyframe, ratio in ((False, 0.6), (True, 0.9), (False, 1.5)):
        h = rig.ctx.bow_search(s1["node_of"], s1["active"], s1["desc"], s2["node_of"], s2["desc"], eligible2=s2["has"] if keyframe else None, strict_low=keyframe,
                               nn_ratio=ratio)
        res, _, _ = rig.run([s1], [s2], eligible="has" if keyframe else None, strict=keyframe, nn_ratio=ratio)
        for k in KEYS:
            assert np.array_equal(h[k], res[0][k]), (keyframe, k)
    m = ORBmatcher(nnratio=0.7, ctx=rig.ctx)
    n, m12, r = m.search_by_bow(s1["node_of"], s1["active"], s1["desc"], s2["node_of"], s2["desc"])
    lit = RB.literal(s.dist(oracle_mod, 0, 0), s1["node_of"], s1["active"], s2["node_of"], None, 0, nn_ratio=0.7)
    assert n == lit["n_matches"] and np.array_equal(m12, lit["match12"]) and np.array_equal(r["assigned2"], lit["assigned2"])
    n, m12, r = m.search_by_bow_keyframes(s1["node_of"], s1["active"], s1["desc"], s2["node_of"], s2["has"], s2["desc"])
    lit = RB.literal(s.dist(oracle_mod, 0, 0), s1["node_of"], s1["active"], s2["node_of"], s2["has"], RB.STRICT_LOW, nn_ratio=0.7)
    assert n == lit["n_matches"] and np.array_equal(m12, lit["match12"]) and n != m.search_by_bow(s1["node_of"], s1["active"], s1["desc"], s2["node_of"], s2["desc"])[0]
    # tiny problems (n1, n2 < 4, one and two nodes): the shapes of the hand-made cases with descriptors on one axis per query; the table the
    # device sees is the C oracle's, and the answer is the restatement's for that table
    for name, dist, no1, a1, no2, e2, flags, ratio, _ in RB.handmade():
        n1, n2 = dist.shape
        d1 = np.zeros((n1, 64), F); d2 = np.zeros((n2, 64), F)
        for i in range(n1):
            d2[:, i] = np.sqrt(np.array(dist[i], np.float64) / 2048.0).astype(F)
        table = oracle_mod.distance_i32(d1, d2)
        h = rig.ctx.bow_search(no1, a1, d1, no2, d2, eligible2=e2, strict_low=bool(flags & RB.STRICT_LOW), nn_ratio=ratio)
        lit = RB.per_node(table, no1, a1, no2, e2, flags, nn_ratio=ratio)
        for key in KEYS:
            assert np.array_equal(h[key], lit[key]), (name, key)


def test_invalid_arguments_launch_nothing(rig, scene):
    L, ctx, s = rig.L, rig.ctx, scene
    n1, n2 = BR.N1, BR.N2
    lay = Context.bow_search_layout(1, n1, n2)
    sent = np.full(lay["bytes"], 0xA5, np.uint8)
    out = capi.DeviceBuffer(lay["bytes"]).upload(sent)
    mk = lambda a: capi.DeviceBuffer(np.ascontiguousarray(a).nbytes + 32).upload(a)
    a1, a2 = rig.side([s.s1], "active"), rig.side([s.s2[0]], "has")
    bufs = {k + "1": mk(a1[k]) for k in ("blob", "flag", "desc")}
    bufs.update({k + "2": mk(a2[k]) for k in ("blob", "flag", "desc")})
    ws = capi.DeviceBuffer(Context.bow_search_workspace_bytes(n1, n2, 1) + 32)
    base = dict(ctx=ctx.h, B=1, n1=n1, n2=n2, shared=0, flags=0, init=256, low=100, ratio=0.6, blob1=bufs["blob1"].ptr, act1=bufs["flag1"].ptr, desc1=bufs["desc1"].ptr,
                st1=a1["stride"], blob2=bufs["blob2"].ptr, el2=bufs["flag2"].ptr, desc2=bufs["desc2"].ptr, st2=a2["stride"], ws=ws.ptr, st=out.ptr + lay["status"],
                m=out.ptr + lay["match12"], bd=out.ptr + lay["best_dist"], sd=out.ptr + lay["second_dist"], nc=out.ptr + lay["n_candidates"], as2=out.ptr + lay["assigned2"],
                nm=out.ptr + lay["n_matches"])

    def call(**kw):
        a = dict(base); a.update(kw)
        return L.xfh_bow_search_device(*[a[k] for k in base])

    nan, inf = float("nan"), float("inf")
    bad = [dict(B=0), dict(B=-1), dict(B=65536), dict(n1=0), dict(n1=-1), dict(n1=capi.GRID_MAX_N + 1), dict(n2=0), dict(n2=capi.GRID_MAX_N + 1), dict(shared=3), dict(shared=-1),
           dict(flags=2), dict(flags=-1), dict(flags=3), dict(ratio=nan), dict(ratio=inf), dict(ratio=-inf), dict(ratio=-0.1), dict(low=-1), dict(init=-1),
           dict(desc1=base["desc1"] + 4), dict(desc2=base["desc2"] + 8), dict(st1=a1["stride"] + 4), dict(st2=a2["stride"] + 8), dict(blob1=base["blob1"] + 8),
           dict(blob2=base["blob2"] + 4), dict(ws=base["ws"] + 8), dict(ws=base["ws"] + 1), dict(m=base["m"] + 2), dict(bd=base["bd"] + 1), dict(sd=base["sd"] + 2),
           dict(nc=base["nc"] + 2), dict(as2=base["as2"] + 2), dict(nm=base["nm"] + 2),
           dict(ctx=None), dict(blob1=None), dict(act1=None), dict(desc1=None), dict(blob2=None), dict(desc2=None), dict(ws=None), dict(st=None), dict(m=None), dict(bd=None),
           dict(sd=None), dict(nc=None), dict(as2=None), dict(nm=None)]
    ctx.synchronize()
    for kid in ("BOW_CANDIDATES", "BOW_RESOLVE"):
        ctx.timing_enable(capi.K[kid])
        for kw in bad:
            assert call(**kw) == 1, kw
        ctx.synchronize()
        assert ctx.timing_read()[0] == 0 and np.array_equal(out.download(np.uint8, lay["bytes"]), sent)
        assert call() == 0 and call(shared=1) == 0 and call(shared=2) == 0 and call(el2=None, flags=1) == 0 and call(ratio=0.0) == 0   # the valid calls still work afterwards
        ctx.synchronize()
        assert ctx.timing_read()[0] == 5 and not np.array_equal(out.download(np.uint8, lay["bytes"]), sent)
        ctx.timing_enable(capi.K["NONE"])
        out.upload(sent)
    # the host form refuses the same classes before it stages anything
    s1, s2 = s.s1, s.s2[0]
    keep = [np.ascontiguousarray(a) for a in (s1["node_of"], s1["active"], s1["desc"], s2["node_of"], s2["has"], s2["desc"])]
    houts = {n: np.full(n1 * w, 0xA5, np.uint8) for n, w in (("st", 1), ("m", 4), ("bd", 4), ("sd", 4), ("nc", 4))}
    houts["as2"] = np.full(4 * n2, 0xA5, np.uint8); houts["nm"] = np.full(4, 0xA5, np.uint8)
    names = ("no1", "act1", "desc1", "no2", "el2", "desc2")
    hb = dict(ctx=ctx.h, n1=n1, n2=n2, flags=0, init=256, low=100, ratio=0.6, **{n: a.ctypes.data for n, a in zip(names, keep)}, **{n: a.ctypes.data for n, a in houts.items()})

    def hcall(**kw):
        a = dict(hb); a.update(kw)
        return L.xfh_bow_search(*[a[k] for k in hb])

    hbad = [dict(ctx=None), dict(n1=0), dict(n1=capi.GRID_MAX_N + 1), dict(n2=0), dict(n2=-3), dict(flags=2), dict(flags=-1), dict(ratio=nan), dict(ratio=-1.0), dict(low=-1),
            dict(init=-5)] + [{n: None} for n in names if n != "el2"] + [{n: None} for n in houts]
    ctx.timing_enable(capi.K["BOW_RESOLVE"])
    for kw in hbad:
        assert hcall(**kw) == 1, kw
    assert ctx.timing_read()[0] == 0 and all(np.all(a == 0xA5) for a in houts.values())
    assert hcall() == 0 and hcall(el2=None, flags=1) == 0
    assert ctx.timing_read()[0] == 2 and not any(np.all(a == 0xA5) for a in houts.values())
    ctx.timing_enable(capi.K["NONE"])
    for x in [out, ws] + list(bufs.values()):
        x.free()
