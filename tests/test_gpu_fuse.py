"""xfh_fuse_search_device (k_fuse_search) against the sequential restatement tests/ref_fuse.py on the scene and with the guarded runs of
tests/fuse_rig.py, stage by stage: proj against the model's projection of the same points by bits, then the cull statuses, then the
level, then the search of the model evaluated on the DEVICE's own (u, v, ur) -- so one failure names one stage.  Every comparison is
equality of bits and integers.  The conditions the scene is chosen for (every status, every level class, both chi-square branches) are
asserted where the seeds are chosen, on the CPU (tests/test_fuse_ref.py); here they are printed."""
import ctypes as C

import numpy as np
import pytest

import ref_frame as RF
import ref_fuse as RU
from fuse_rig import NL, OUT_INT, ROLL, SF, FuseRig
from projection_rig import F, TUM1, cam_struct
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context

pytestmark = pytest.mark.gpu

FORMS = [("se3", dict(chi2=True, init=256)), ("sim3", dict(chi2=False, init=RU.INT_MAX))]


def same(res, m, tag):
    for k in ("status", "best_idx", "best_dist", "n_window", "n_tested"):
        assert np.array_equal(res[k], m[k]), (tag, k, np.nonzero(res[k] != m[k])[0][:8])
    assert res["n_fused"] == m["n_fused"], tag


def check(fr, O, res, f, th, tag, xyz=None, normals=None, dist=None, flags=None, poses=None, Ow=None, p=None, qdesc=None, **kw):
    """one problem's outputs, stage by stage; frame f, pose p (default f)"""
    p = f if p is None else p
    pick = lambda a, d: d if a is None else a
    flags = pick(flags, fr.flags)
    u, v, ur, r, lv, st = RU.project(pick(poses, fr.poses)[p], pick(Ow, fr.Ow)[p], TUM1, fr.bounds, th, SF, NL, pick(xyz, fr.xyz), pick(normals, fr.normals), pick(dist, fr.dist))
    act = (flags & 1) != 0
    pj = res["proj"]
    for j, a in enumerate((u, v, ur)):                                               # stage 1: proj
        assert RF.same_bits(pj[act, j], a[act]), (tag, "proj", j)
    assert np.all(pj[~act] == 0)
    st = np.where(act, st, RU.INACTIVE).astype(np.uint8)
    dst = res["status"]
    assert np.array_equal(dst >= RU.VISIBLE, st == RU.VISIBLE) and np.array_equal(dst[st != RU.VISIBLE], st[st != RU.VISIBLE]), (tag, "cull")      # stage 2
    assert np.array_equal(res["level"], np.where(act, lv, -1)), (tag, "level")           # stage 3
    st_dev = np.where(dst >= RU.VISIBLE, RU.VISIBLE, dst).astype(np.uint8)
    m = fr.model(O, f, st_dev, res["level"], pj[:, 0].copy(), pj[:, 1].copy(), r, pj[:, 2].copy(), qdesc=qdesc, **kw)       # stage 4, on the DEVICE's proj (r = th * sf[level]: checked by 3)
    same(res, m, tag)
    print(f"{tag} frame {f} th {th}: statuses {np.bincount(dst, minlength=8).tolist()}, levels {np.bincount(res['level'][dst >= RU.VISIBLE], minlength=NL).tolist()}, "
          f"tested {int(res['n_tested'].sum())} of {int(res['n_window'].sum())} window members, fused {res['n_fused']}")
    return m


@pytest.fixture(scope="module", params=[(900, 4096), (901, 1000)])
def fr(request, gpu_lib, weights_dense):
    r = FuseRig(gpu_lib, weights_dense[1], request.param[1], request.param[0])
    yield r
    r.close()


@pytest.mark.parametrize("th", [3.0, 7.0])
def test_one_problem_both_forms(fr, oracle_mod, th):
    for name, kw in FORMS:
        res, raw = fr.run(1, False, th, **kw)
        check(fr, oracle_mod, res[0], 0, th, name, **kw)
        res2, raw2 = fr.run(1, True, th, **kw)                                         # two runs (and stride 0 at B = 1) give identical bytes
        assert np.array_equal(raw, raw2)
    assert res[0]["n_fused"] > 0
    res, _ = fr.run(1, False, th, uright=False)                                        # a monocular keyframe: d_uright = NULL
    check(fr, oracle_mod, res[0], 0, th, "mono", uright=False)


@pytest.mark.parametrize("th", [3.0, 7.0])
def test_four_problems(fr, oracle_mod, th):
    res, raw = fr.run(4, False, th)                                                    # own poses AND own queries, query_problem_stride = nq
    for p in range(4):
        check(fr, oracle_mod, res[p], p, th, f"B=4 p={p}", **fr.block(p))              # each problem against its own block
    assert len({r["n_fused"] for r in res}) > 1
    assert np.array_equal(fr.run(4, False, th)[1], raw)                                # two runs give identical bytes (the n_fused atomics and their memset too)
    res0, raw0 = fr.run(4, True, th)                                                   # stride 0: four B = 1 calls, byte for byte
    assert np.array_equal(fr.run(4, True, th)[1], raw0)
    for p in range(4):
        one, _ = fr.run(1, False, th, first=p)
        for k in OUT_INT + ("status",):                                                # (problem p's own block is block 0 rotated: so are its answers)
            assert np.array_equal(res0[p][k], one[0][k]) and np.array_equal(np.roll(res0[p][k], p * ROLL), res[p][k]), (p, k)
        assert res0[p]["proj"].tobytes() == one[0]["proj"].tobytes() and res0[p]["n_fused"] == one[0]["n_fused"] == res[p]["n_fused"]


def test_hostile_input(fr, oracle_mod):
    """NaN / Inf / 1e30 in points, Ow, normals, distances and poses: the call returns, every output matches the restatement, guard
    bytes are intact (FuseRig.run checks them)"""
    nf = fr.nf
    vals = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0, -0.0, 3.4e38], F)
    xyz, nr, dd = fr.xyz.copy(), fr.normals.copy(), fr.dist.copy()
    for j in range(nf // 4):
        (xyz, nr, dd)[j % 3][4 * j + 1, (j // 3) % 3] = vals[(j // 9) % len(vals)]
    flags = fr.flags | 1
    for T, O in ((fr.poses[0], fr.Ow[0]), (np.full(12, np.nan, F), fr.Ow[0]), (np.full(12, np.inf, F), np.full(3, 1e30, F)), (np.full(12, 1e30, F), np.full(3, np.nan, F)),
                 (fr.poses[0], np.array([np.inf, 0, 0], F))):
        poses, Ow = fr.poses.copy(), fr.Ow.copy()
        poses[0] = T; Ow[0] = O
        for name, kw in FORMS:
            res, _ = fr.run(1, False, 7.0, xyz=xyz, normals=nr, dist=dd, flags=flags, poses=poses, Ow=Ow, **kw)
            check(fr, oracle_mod, res[0], 0, 7.0, "hostile " + name, xyz=xyz, normals=nr, dist=dd, flags=flags, poses=poses, Ow=Ow, **kw)


def test_host_form_and_hand_made_cases(fr, oracle_mod):
    rg = fr.rig
    res, _ = fr.run(1, False, 7.0, first=1)
    k = np.zeros(fr.nf, capi.KP_DTYPE); k["x"] = rg.xy[1][:, 0]; k["y"] = rg.xy[1][:, 1]
    h = fr.ctx.fuse_search(fr.xyz, fr.normals, fr.dist, fr.qdesc, fr.flags, fr.poses[1], fr.Ow[1], cam_struct(TUM1), fr.bounds, 7.0, fr.sf, fr.rmax, k, rg.recs[1][1],
                           uright=rg.ur[1])
    for key in OUT_INT + ("status",):
        assert np.array_equal(h[key], res[0][key]), key
    assert RF.same_bits(h["proj"].ravel(), res[0]["proj"].ravel()) and h["n_fused"] == res[0]["n_fused"]
    matcher = __import__("xfeatslam_amd.extractor", fromlist=["ORBmatcher"]).ORBmatcher(ctx=fr.ctx)
    n, w = matcher.fuse(fr.xyz, fr.normals, fr.dist, fr.qdesc, fr.flags, fr.poses[1], fr.Ow[1], cam_struct(TUM1), fr.bounds, 7.0, fr.sf, k, rg.recs[1][1], uright=rg.ur[1])
    assert n == res[0]["n_fused"] and np.array_equal(w["best_idx"], res[0]["best_idx"])
    for name, c, want in RU.handmade():                                                # the written-out answers of tests/test_fuse_ref.py, on the device
        kp = np.zeros(len(c["x"]), capi.KP_DTYPE); kp["x"] = c["x"]; kp["y"] = c["y"]
        h = fr.ctx.fuse_search(c["xyz"], c["normals"], c["dist"], c["qdesc"], c["flags"], c["T"], c["Ow"], cam_struct(c["cam"]), c["bounds"], c["th"],
                               RU.scale_factors(c["scale_factor"], c["nlevels"]), Context.scale_level_thresholds(c["scale_factor"], c["nlevels"]), kp, c["tg"],
                               uright=c["uright"], chi2=c["chi2"], init_dist=c["init_dist"])
        for key, val in want.items():
            assert h[key].tolist() == val, (name, key, h[key].tolist(), val)
        assert h["n_fused"] == want["status"].count(RU.FUSED), name


def test_invalid_arguments_launch_nothing(fr):
    L, ctx, nf, rg = fr.rig.L, fr.ctx, fr.nf, fr.rig
    lay = Context.fuse_search_layout(1, nf)
    sent = np.full(lay["bytes"], 0xA5, np.uint8)
    out = capi.DeviceBuffer(lay["bytes"]).upload(sent)
    mk = lambda a: capi.DeviceBuffer(np.ascontiguousarray(a).nbytes + 16).upload(a)
    pts, nr, dd, fl, T, O = mk(fr.xyz), mk(fr.normals), mk(fr.dist), mk(fr.flags), mk(fr.poses[0]), mk(np.concatenate([fr.Ow[0], [0]]).astype(F))
    cam, gb = cam_struct(TUM1), capi.GridBounds(*fr.bounds)
    sf, rm = fr.sf.copy(), fr.rmax.copy()
    base = dict(ctx=ctx.h, B=1, nq=nf, stride=nf, pts=pts.ptr, nr=nr.ptr, dd=dd.ptr, qd=rg.rec.ptr + ctx.desc_off, fl=fl.ptr, T=T.ptr, O=O.ptr, cam=C.byref(cam), b=C.byref(gb),
                th=3.0, sf=sf.ctypes.data, rm=rm.ctypes.data, nl=NL, grids=rg.fin[3].ptr, tg=rg.rec.ptr + ctx.desc_off, tstride=ctx.rec_bytes, nt=nf, ur=rg.fin[1].ptr,
                flags=capi.FUSE_CHI2, init=256, low=100, st=out.ptr + lay["status"], bi=out.ptr + lay["best_idx"], bd=out.ptr + lay["best_dist"], nw=out.ptr + lay["n_window"],
                ntst=out.ptr + lay["n_tested"], lv=out.ptr + lay["level"], pj=out.ptr + lay["proj"], nfu=out.ptr + lay["n_fused"])

    def call(**kw):
        a = dict(base); a.update(kw)
        return L.xfh_fuse_search_device(*[a[k] for k in base])

    nan, inf = float("nan"), float("inf")
    bad = [dict(B=0), dict(B=-1), dict(B=65536), dict(nq=0), dict(nq=(1 << 20) + 1), dict(nt=0), dict(nt=capi.GRID_MAX_N + 1), dict(nl=0), dict(nl=17), dict(nl=-1),
           dict(stride=1), dict(stride=nf + 1), dict(stride=2 * nf), dict(th=nan), dict(th=inf), dict(th=-inf), dict(flags=2), dict(flags=-1),
           dict(qd=base["qd"] + 4), dict(tg=base["tg"] + 8), dict(tstride=ctx.rec_bytes + 4), dict(grids=base["grids"] + 8), dict(pts=pts.ptr + 2), dict(nr=nr.ptr + 1),
           dict(dd=dd.ptr + 2), dict(T=T.ptr + 2), dict(O=O.ptr + 2), dict(ur=base["ur"] + 2), dict(bi=base["bi"] + 2), dict(lv=base["lv"] + 1), dict(pj=base["pj"] + 2),
           dict(nfu=base["nfu"] + 2), dict(ctx=None), dict(cam=None), dict(b=None), dict(sf=None), dict(rm=None), dict(pts=None), dict(nr=None), dict(dd=None), dict(qd=None),
           dict(fl=None), dict(T=None), dict(O=None), dict(grids=None), dict(tg=None), dict(st=None), dict(bi=None), dict(bd=None), dict(nw=None), dict(ntst=None),
           dict(lv=None), dict(nfu=None)]
    for kw in bad:
        assert call(**kw) == 1, kw
    ctx.synchronize()
    assert np.array_equal(out.download(np.uint8, lay["bytes"]), sent)
    assert call() == 0 and call(stride=0) == 0 and call(ur=None) == 0 and call(pj=None) == 0           # the valid calls still work afterwards
    ctx.synchronize()
    assert not np.array_equal(out.download(np.uint8, lay["bytes"]), sent)
    for x in (out, pts, nr, dd, fl, T, O):
        x.free()


def test_host_form_invalid_arguments_stage_and_launch_nothing(fr):
    """xfh_fuse_search refuses every class of argument the device form refuses BEFORE it stages or launches: the grid build, its first
    launch, is counted by the library's timers and stays at zero, and no output array is written"""
    L, ctx, nf, rg = fr.rig.L, fr.ctx, fr.nf, fr.rig
    k = np.zeros(nf, capi.KP_DTYPE); k["x"] = rg.xy[0][:, 0]; k["y"] = rg.xy[0][:, 1]
    keep = [np.ascontiguousarray(a, t) for a, t in ((fr.xyz, F), (fr.normals, F), (fr.dist, F), (fr.qdesc, F), (fr.flags, np.uint8), (fr.poses[0], F), (fr.Ow[0], F),
                                                    (fr.sf, F), (fr.rmax, F), (rg.recs[0][1], F), (rg.ur[0], F))]
    pts, nr, dd, qd, fl, T, O, sf, rm, tg, ur = keep
    out = {n: np.full(nf * w, 0xA5, np.uint8) for n, w in (("st", 1), ("bi", 4), ("bd", 4), ("nw", 4), ("ntst", 4), ("lv", 4), ("pj", 12))}
    out["nfu"] = np.full(4, 0xA5, np.uint8)
    cam, gb = cam_struct(TUM1), capi.GridBounds(*fr.bounds)
    badb = [capi.GridBounds(*b) for b in ((0, 0, 0, 480), (0, 480, 640, 0), (float("nan"), 0, 640, 480), (0, 0, float("inf"), 480))]   # empty, reversed, NaN, Inf
    base = dict(ctx=ctx.h, nq=nf, pts=pts.ctypes.data, nr=nr.ctypes.data, dd=dd.ctypes.data, qd=qd.ctypes.data, fl=fl.ctypes.data, T=T.ctypes.data, O=O.ctypes.data,
                cam=C.byref(cam), b=C.byref(gb), th=3.0, sf=sf.ctypes.data, rm=rm.ctypes.data, nl=NL, kps=k.ctypes.data, tg=tg.ctypes.data, nt=nf, ur=ur.ctypes.data,
                flags=capi.FUSE_CHI2, init=256, low=100, **{n: a.ctypes.data for n, a in out.items()})

    def call(**kw):
        a = dict(base); a.update(kw)
        return L.xfh_fuse_search(*[a[n] for n in base])

    nan, inf = float("nan"), float("inf")
    bad = [dict(ctx=None), dict(nq=0), dict(nq=-1), dict(nq=(1 << 20) + 1), dict(nt=0), dict(nt=capi.GRID_MAX_N + 1), dict(nl=0), dict(nl=17), dict(nl=-1), dict(th=nan),
           dict(th=inf), dict(th=-inf), dict(flags=2), dict(flags=-1), dict(cam=None), dict(b=None), dict(sf=None), dict(rm=None), dict(pts=None), dict(nr=None),
           dict(dd=None), dict(qd=None), dict(fl=None), dict(T=None), dict(O=None), dict(kps=None), dict(tg=None), dict(st=None), dict(bi=None), dict(bd=None),
           dict(nw=None), dict(ntst=None), dict(lv=None), dict(nfu=None)] + [dict(b=C.byref(x)) for x in badb]
    ctx.synchronize()
    ctx.timing_enable(capi.K["GRID_BUILD"])
    for kw in bad:
        assert call(**kw) == 1, kw
    assert ctx.timing_read()[0] == 0 and all(np.all(a == 0xA5) for a in out.values())
    assert call() == 0 and call(ur=None) == 0 and call(pj=None) == 0                    # the valid calls still work afterwards
    assert ctx.timing_read()[0] == 3 and not any(np.all(a == 0xA5) for a in out.values())
    ctx.timing_enable(capi.K["NONE"])
