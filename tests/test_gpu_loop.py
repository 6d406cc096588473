"""xfh_map_projection_search_device (k_mapproj_candidates + the resolver of the projection search) and xfh_sim3_search_device (k_sim3_search,
k_sim3_agree) against the sequential restatements of tests/ref_loop.py on the scenes and with the guarded runs of tests/loop_rig.py, stage by
stage: proj against the model's projection of the same points by bits, then the cull statuses, then the level, then the search of the
model evaluated on the DEVICE's own (u, v, r) -- so one failure names one stage.  Every comparison is equality of bits and integers.
The conditions the scenes are chosen for are asserted where the seeds are chosen, on the CPU (tests/test_loop_ref.py); here they are
printed."""
import ctypes as C

import numpy as np
import pytest

import ref_frame as RF
import ref_fuse as RU
import ref_loop as RL
from loop_rig import MAP_INT, NL, SF, SIM3_INT, LoopRig
from projection_rig import F, TUM1, cam_struct
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context, ORBmatcher

pytestmark = pytest.mark.gpu

ACCEPT_SIM3 = float(F(RL.TH_LOW) * F(1.5))
FORMS = [("sim3", RL.FORM_SIM3, ACCEPT_SIM3), ("sim3_kf", RL.FORM_SIM3_KF, ACCEPT_SIM3), ("reloc", RL.FORM_RELOC, 100.0)]


@pytest.fixture(scope="module", params=[(900, 4096), (901, 1000)])
def lr(request, gpu_lib, weights_dense, oracle_mod):
    r = LoopRig(gpu_lib, weights_dense[1], request.param[1], request.param[0], oracle_mod)
    yield r
    r.close()


def check_map(lr, res, f, p, th, form, accept, tag, blk=None, poses=None, Ow=None, taken=True):
    """one problem's outputs, stage by stage; frame f, pose and block p"""
    blk = lr.block(p) if blk is None else blk
    T = (lr.poses if poses is None else poses)[p]; O = (lr.Ow if Ow is None else Ow)[p]
    u, v, r, lv, st = RL.map_project(T, O, TUM1, lr.bounds, th, SF, NL, form, blk["xyz"], blk["normals"], blk["dist"])
    act = (blk["flags"] & 1) != 0
    pj = res["proj"]
    for j, a in enumerate((u, v, r)):                                                # stage 1: proj
        assert RF.same_bits(pj[act, j], a[act]), (tag, "proj", j)
    assert np.all(pj[~act] == 0)
    st = np.where(act, st, RL.INACTIVE).astype(np.uint8)
    dst = res["status"]
    assert np.array_equal(dst >= RL.VISIBLE, st == RL.VISIBLE) and np.array_equal(dst[st != RL.VISIBLE], st[st != RL.VISIBLE]), (tag, "cull")      # stage 2
    assert np.array_equal(res["level"], np.where(act, lv, -1)), (tag, "level")           # stage 3
    st_dev = np.where(dst >= RL.VISIBLE, RL.VISIBLE, dst).astype(np.uint8)
    m = lr.model_map(f, st_dev, res["level"], pj[:, 0].copy(), pj[:, 1].copy(), pj[:, 2].copy(), blk, accept, taken)      # stage 4, on the DEVICE's proj
    for k in ("status", "match_idx", "best_dist", "n_window", "n_tested", "assigned"):
        assert np.array_equal(res[k], m[k]), (tag, k, np.nonzero(res[k] != m[k])[0][:8])
    assert res["n_matches"] == m["n_matches"], tag
    print(f"{tag} frame {f} th {th}: statuses {np.bincount(dst, minlength=8).tolist()}, levels {np.bincount(res['level'][dst >= RL.VISIBLE], minlength=NL).tolist()}, "
          f"tested {int(res['n_tested'].sum())} of {int(res['n_window'].sum())} window members, matches {res['n_matches']}, four best taken {int(m['redo'].sum())}")
    return m


def check_sim3(lr, res, p, th, tag, shared=False, th_high=RL.TH_HIGH, **over):
    """one pair's outputs, stage by stage and direction by direction, then the agreement"""
    s1, s2, T1, T2, M21, M12 = lr.problem(p, shared, **over)
    for s, q, T, M, f in (("1", s1, T1, M21, p), ("2", s2, T2, M12, 0)):
        u, v, r, lv, st = RL.sim3_project(T, M, TUM1, lr.bounds, th, SF, NL, q["points"], q["dist"])
        act = (q["flags"] & 1) != 0
        pj = res["proj" + s]
        for j, a in enumerate((u, v, r)):
            assert RF.same_bits(pj[act, j], a[act]), (tag, s, "proj", j)
        assert np.all(pj[~act] == 0)
        st = np.where(act, st, RL.INACTIVE).astype(np.uint8)
        dst = res["status" + s]
        assert np.array_equal(dst >= RL.VISIBLE, st == RL.VISIBLE) and np.array_equal(dst[st != RL.VISIBLE], st[st != RL.VISIBLE]), (tag, s, "cull")
        assert np.array_equal(res["level" + s], np.where(act, lv, -1)), (tag, s, "level")
        st_dev = np.where(dst >= RL.VISIBLE, RL.VISIBLE, dst).astype(np.uint8)
        m = lr.model_sim3(f, st_dev, res["level" + s], pj[:, 0].copy(), pj[:, 1].copy(), pj[:, 2].copy(), q["mp_desc"], th_high)
        for k in ("status", "match", "best_dist", "n_window", "n_tested"):
            assert np.array_equal(res[k + s], m[k]), (tag, s, k, np.nonzero(res[k + s] != m[k])[0][:8])
        print(f"{tag} side {s} th {th}: statuses {np.bincount(dst, minlength=8).tolist()}, tested {int(res['n_tested' + s].sum())} of {int(res['n_window' + s].sum())} window members")
    m12, nfound = RL.sim3_agree(res["match1"], res["match2"])
    assert np.array_equal(res["match12"], m12) and res["n_found"] == nfound, tag
    print(f"{tag}: agreed {nfound}, one-sided matches of side 1 dropped {int(((res['match1'] >= 0) & (m12 < 0)).sum())}")


# ---- map projection ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("th", [4.0, 15.0])
def test_map_projection_one_problem_every_form(lr, th):
    for name, form, accept in FORMS:
        res, raw, hdr = lr.run_map(1, th, form, accept)
        m = check_map(lr, res[0], 0, 0, th, form, accept, name)
        assert np.array_equal(lr.run_map(1, th, form, accept)[1], raw)                 # two runs give identical bytes
        assert res[0]["n_matches"] > 0
        print(f"{name} th {th}: resolver rounds {hdr[0, 0]}, queries searched again in full {hdr[0, 1]}")
        if th == 15.0:
            assert hdr[0, 1] >= 1 and m["redo"].sum() >= 1
    res, _, _ = lr.run_map(1, th, RL.FORM_SIM3, ACCEPT_SIM3, taken=False)              # d_taken = NULL
    check_map(lr, res[0], 0, 0, th, RL.FORM_SIM3, ACCEPT_SIM3, "no taken", blk=dict(lr.block(0), taken=None), taken=False)


@pytest.mark.parametrize("th", [4.0, 15.0])
def test_map_projection_four_problems(lr, th):
    name, form, accept = FORMS[int(th) % 3]
    res, raw, _ = lr.run_map(4, th, form, accept)                                      # own frame, pose, query block and taken bytes each
    for p in range(4):
        check_map(lr, res[p], p, p, th, form, accept, f"{name} B=4 p={p}")
    assert len({r["n_matches"] for r in res}) > 1
    assert np.array_equal(lr.run_map(4, th, form, accept)[1], raw)                     # two runs give identical bytes
    sh, raws, _ = lr.run_map(4, th, form, accept, shared=True)                         # every problem searches frame 0 ...
    assert np.array_equal(lr.run_map(4, th, form, accept, shared=True)[1], raws)
    for p in range(4):
        check_map(lr, sh[p], 0, p, th, form, accept, f"{name} shared p={p}")
        one, _, _ = lr.run_map(1, th, form, accept, shared=True, first=p)              # ... as four single calls do, byte for byte
        for k in MAP_INT + ("assigned", "status"):
            assert np.array_equal(sh[p][k], one[0][k]), (p, k)
        assert sh[p]["proj"].tobytes() == one[0]["proj"].tobytes() and sh[p]["n_matches"] == one[0]["n_matches"]


def test_map_projection_hostile_input(lr):
    """NaN / Inf / 1e30 in points, normals, distances, poses and camera centres: the call returns, every output matches the restatement,
    guard bytes are intact (LoopRig.run_map checks them)"""
    nf, sc = lr.nf, lr.scene
    vals = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0, -0.0, 3.4e38], F)
    xyz, nr, dd = sc["xyz"].copy(), sc["normals"].copy(), sc["dist"].copy()
    for j in range(nf // 4):
        (xyz, nr, dd)[j % 3][4 * j + 1, (j // 3) % 3] = vals[(j // 9) % len(vals)]
    flags = sc["flags"] | 1
    over = dict(xyz=xyz, normals=nr, dist=dd, flags=flags)
    cases = ((lr.poses[0], lr.Ow[0]), (np.full(12, np.nan, F), lr.Ow[0]), (np.full(12, np.inf, F), np.full(3, 1e30, F)), (np.full(12, 1e30, F), np.full(3, np.nan, F)),
             (lr.poses[0], np.array([np.inf, 0, 0], F)))
    for i, (T, O) in enumerate(cases):
        poses, Ow = lr.poses.copy(), lr.Ow.copy()
        poses[0] = T; Ow[0] = O
        name, form, accept = FORMS[i % 3]
        res, _, _ = lr.run_map(1, 15.0, form, accept, poses=poses, Ow=Ow, **over)
        check_map(lr, res[0], 0, 0, 15.0, form, accept, "hostile " + name, blk=lr.block(0, **over), poses=poses, Ow=Ow)


def test_map_projection_host_form_matcher_and_hand_made_cases(lr):
    sc, cam = lr.scene, cam_struct(TUM1)
    matcher = ORBmatcher(ctx=lr.ctx)
    for name, form, accept in FORMS:
        res, _, _ = lr.run_map(1, 4.0, form, accept, first=1)
        blk = lr.block(1)
        h = lr.ctx.map_projection_search(form, blk["xyz"], blk["normals"], blk["dist"], blk["qdesc"], blk["flags"], lr.poses[1], lr.Ow[1], cam, lr.bounds, 4.0, lr.sf,
                                         lr.rmax, lr.kps(1), lr.rig.recs[1][1], taken=blk["taken"], accept_max=accept)
        for key in MAP_INT + ("status", "assigned"):
            assert np.array_equal(h[key], res[0][key]), (name, key)
        assert RF.same_bits(h["proj"].ravel(), res[0]["proj"].ravel()) and h["n_matches"] == res[0]["n_matches"]
        args = (blk["xyz"], blk["normals"], blk["dist"], blk["qdesc"], blk["flags"], lr.poses[1], lr.Ow[1], cam, lr.bounds, 4.0)
        if form == RL.FORM_RELOC:
            n, w = matcher.searchByProjectionReloc(*args, 100, lr.sf, lr.kps(1), lr.rig.recs[1][1], taken=blk["taken"])
        else:
            n, w = matcher.searchByProjectionSim3(*args, 1.5, lr.sf, lr.kps(1), lr.rig.recs[1][1], taken=blk["taken"], with_keyframes=form == RL.FORM_SIM3_KF)
        assert n == res[0]["n_matches"] and np.array_equal(w["match_idx"], res[0]["match_idx"]) and np.array_equal(w["assigned"], res[0]["assigned"])
    for name, c, want in RL.handmade_map():                                            # the written-out answers of tests/test_loop_ref.py, on the device
        kp = np.zeros(len(c["x"]), capi.KP_DTYPE); kp["x"] = c["x"]; kp["y"] = c["y"]
        h = lr.ctx.map_projection_search(c["form"], c["xyz"], c["normals"], c["dist"], c["qdesc"], c["flags"], c["T"], c["Ow"], cam_struct(c["cam"]), c["bounds"], c["th"],
                                         RU.scale_factors(c["scale_factor"], c["nlevels"]), Context.scale_level_thresholds(c["scale_factor"], c["nlevels"]), kp, c["tg"],
                                         taken=c["taken"], accept_max=c["accept_max"])
        h["proj_u"] = h["proj"][:, 0]
        for key, val in want.items():
            got = h[key] if np.isscalar(h[key]) else h[key].tolist()
            assert got == val, (name, key, got, val)


def test_map_projection_invalid_arguments_launch_nothing(lr):
    L, ctx, nf, rg, sc = lr.rig.L, lr.ctx, lr.nf, lr.rig, lr.scene
    lay = Context.map_projection_search_layout(1, nf, nf)
    sent = np.full(lay["bytes"], 0xA5, np.uint8)
    out = capi.DeviceBuffer(lay["bytes"]).upload(sent)
    mk = lambda a: capi.DeviceBuffer(np.ascontiguousarray(a).nbytes + 16).upload(a)
    pts, nr, dd, qd, fl, T, O, tk = (mk(a) for a in (sc["xyz"], sc["normals"], sc["dist"], sc["qdesc"], sc["flags"], lr.poses[0], np.concatenate([lr.Ow[0], [0]]).astype(F),
                                                     sc["taken"]))
    ws = capi.DeviceBuffer(Context.map_projection_search_workspace_bytes(nf, nf, 1))
    cam, gb = cam_struct(TUM1), capi.GridBounds(*lr.bounds)
    sf, rm = lr.sf.copy(), lr.rmax.copy()
    base = dict(ctx=ctx.h, form=RL.FORM_SIM3, B=1, nq=nf, pts=pts.ptr, nr=nr.ptr, dd=dd.ptr, qd=qd.ptr, fl=fl.ptr, T=T.ptr, O=O.ptr, cam=C.byref(cam), b=C.byref(gb), th=4.0,
                sf=sf.ctypes.data, rm=rm.ctypes.data, nl=NL, grids=rg.fin[3].ptr, tg=rg.rec.ptr + ctx.desc_off, tstride=ctx.rec_bytes, shared=0, nt=nf, tk=tk.ptr, init=256,
                acc=100.0, ws=ws.ptr, st=out.ptr + lay["status"], mi=out.ptr + lay["match_idx"], bd=out.ptr + lay["best_dist"], nw=out.ptr + lay["n_window"],
                ntst=out.ptr + lay["n_tested"], lv=out.ptr + lay["level"], pj=out.ptr + lay["proj"], asg=out.ptr + lay["assigned"], nm=out.ptr + lay["n_matches"])

    def call(**kw):
        a = dict(base); a.update(kw)
        return L.xfh_map_projection_search_device(*[a[k] for k in base])

    nan, inf = float("nan"), float("inf")
    bad = [dict(B=0), dict(B=-1), dict(B=65536), dict(nq=0), dict(nq=capi.GRID_MAX_N + 1), dict(nt=0), dict(nt=capi.GRID_MAX_N + 1), dict(nl=0), dict(nl=17), dict(nl=-1),
           dict(form=16), dict(form=-1), dict(form=32 | 3), dict(shared=2), dict(shared=-1), dict(th=nan), dict(th=inf), dict(th=-inf), dict(acc=nan), dict(acc=inf),
           dict(acc=-1.0), dict(qd=qd.ptr + 4), dict(tg=base["tg"] + 8), dict(tstride=ctx.rec_bytes + 4), dict(grids=base["grids"] + 8), dict(ws=ws.ptr + 8),
           dict(pts=pts.ptr + 2), dict(nr=nr.ptr + 1), dict(dd=dd.ptr + 2), dict(T=T.ptr + 2), dict(O=O.ptr + 2), dict(mi=base["mi"] + 2), dict(lv=base["lv"] + 1),
           dict(pj=base["pj"] + 2), dict(asg=base["asg"] + 2), dict(nm=base["nm"] + 2), dict(ctx=None), dict(cam=None), dict(b=None), dict(sf=None), dict(rm=None),
           dict(pts=None), dict(nr=None), dict(dd=None), dict(qd=None), dict(fl=None), dict(T=None), dict(O=None), dict(grids=None), dict(tg=None), dict(ws=None),
           dict(st=None), dict(mi=None), dict(bd=None), dict(nw=None), dict(ntst=None), dict(lv=None), dict(asg=None), dict(nm=None)]
    for kw in bad:
        assert call(**kw) == 1, kw
    ctx.synchronize()
    assert np.array_equal(out.download(np.uint8, lay["bytes"]), sent)
    # the valid calls still work afterwards (a shared target ignores its stride)
    assert call() == 0 and call(shared=1, tstride=4) == 0 and call(tk=None) == 0 and call(pj=None) == 0 and call(form=15) == 0 and call(form=0, acc=0.0) == 0
    ctx.synchronize()
    assert not np.array_equal(out.download(np.uint8, lay["bytes"]), sent)
    for x in (out, pts, nr, dd, qd, fl, T, O, tk, ws):
        x.free()


def test_map_projection_host_form_invalid_arguments_stage_and_launch_nothing(lr):
    """xfh_map_projection_search refuses every class of argument the device form refuses BEFORE it stages or launches: the grid build, its
    first launch, is counted by the library's timers and stays at zero, and no output array is written"""
    L, ctx, nf, rg, sc = lr.rig.L, lr.ctx, lr.nf, lr.rig, lr.scene
    k = lr.kps(0)
    keep = [np.ascontiguousarray(a, t) for a, t in ((sc["xyz"], F), (sc["normals"], F), (sc["dist"], F), (sc["qdesc"], F), (sc["flags"], np.uint8), (lr.poses[0], F), (lr.Ow[0], F),
                                                    (lr.sf, F), (lr.rmax, F), (rg.recs[0][1], F), (sc["taken"], np.uint8))]
    pts, nr, dd, qd, fl, T, O, sf, rm, tg, tk = keep
    out = {n: np.full(nf * w, 0xA5, np.uint8) for n, w in (("st", 1), ("mi", 4), ("bd", 4), ("nw", 4), ("ntst", 4), ("lv", 4), ("pj", 12), ("asg", 4))}
    out["nm"] = np.full(4, 0xA5, np.uint8)
    cam, gb = cam_struct(TUM1), capi.GridBounds(*lr.bounds)
    badb = [capi.GridBounds(*b) for b in ((0, 0, 0, 480), (0, 480, 640, 0), (float("nan"), 0, 640, 480), (0, 0, float("inf"), 480))]   # empty, reversed, NaN, Inf
    base = dict(ctx=ctx.h, form=RL.FORM_RELOC, nq=nf, pts=pts.ctypes.data, nr=nr.ctypes.data, dd=dd.ctypes.data, qd=qd.ctypes.data, fl=fl.ctypes.data, T=T.ctypes.data,
                O=O.ctypes.data, cam=C.byref(cam), b=C.byref(gb), th=4.0, sf=sf.ctypes.data, rm=rm.ctypes.data, nl=NL, kps=k.ctypes.data, tg=tg.ctypes.data, nt=nf,
                tk=tk.ctypes.data, init=256, acc=100.0, **{n: a.ctypes.data for n, a in out.items()})

    def call(**kw):
        a = dict(base); a.update(kw)
        return L.xfh_map_projection_search(*[a[n] for n in base])

    nan, inf = float("nan"), float("inf")
    bad = [dict(ctx=None), dict(nq=0), dict(nq=-1), dict(nq=capi.GRID_MAX_N + 1), dict(nt=0), dict(nt=capi.GRID_MAX_N + 1), dict(nl=0), dict(nl=17), dict(nl=-1), dict(th=nan),
           dict(th=inf), dict(form=16), dict(form=-1), dict(acc=nan), dict(acc=inf), dict(acc=-0.5), dict(cam=None), dict(b=None), dict(sf=None), dict(rm=None), dict(pts=None),
           dict(nr=None), dict(dd=None), dict(qd=None), dict(fl=None), dict(T=None), dict(O=None), dict(kps=None), dict(tg=None), dict(st=None), dict(mi=None), dict(bd=None),
           dict(nw=None), dict(ntst=None), dict(lv=None), dict(asg=None), dict(nm=None)] + [dict(b=C.byref(x)) for x in badb]
    ctx.synchronize()
    ctx.timing_enable(capi.K["GRID_BUILD"])
    for kw in bad:
        assert call(**kw) == 1, kw
    assert ctx.timing_read()[0] == 0 and all(np.all(a == 0xA5) for a in out.values())
    assert call() == 0 and call(tk=None) == 0 and call(pj=None) == 0                    # the valid calls still work afterwards
    assert ctx.timing_read()[0] == 3 and not any(np.all(a == 0xA5) for a in out.values())
    ctx.timing_enable(capi.K["NONE"])


# ---- SearchBySim3 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("th", [4.0, 15.0])
def test_sim3_one_pair(lr, th):
    res, raw = lr.run_sim3(1, th)
    check_sim3(lr, res[0], 0, th, "B=1")
    assert res[0]["n_found"] > 0
    assert np.array_equal(lr.run_sim3(1, th)[1], raw)                                  # two runs give identical bytes
    res, _ = lr.run_sim3(1, th, th_high=60)                                            # a threshold that rejects
    check_sim3(lr, res[0], 0, th, "th_high 60", th_high=60)


@pytest.mark.parametrize("th", [4.0, 15.0])
def test_sim3_four_pairs(lr, th):
    res, raw = lr.run_sim3(4, th)                                                      # own side 2, own Sim3 and poses, own flags on side 1
    for p in range(4):
        check_sim3(lr, res[p], p, th, f"B=4 p={p}")
    assert len({r["n_found"] for r in res}) > 1
    assert np.array_equal(lr.run_sim3(4, th)[1], raw)                                  # two runs give identical bytes (the n_found atomics and their memset too)
    sh, raws = lr.run_sim3(4, th, shared=True)                                         # every pair reads problem 0's side 1 ...
    assert np.array_equal(lr.run_sim3(4, th, shared=True)[1], raws)
    for p in range(4):
        check_sim3(lr, sh[p], p, th, f"shared p={p}", shared=True)
        one, _ = lr.run_sim3(1, th, shared=True, first=p)                              # ... as four single calls do, byte for byte
        for k in [n + s for n in SIM3_INT + ("status",) for s in "12"] + ["match12"]:
            assert np.array_equal(sh[p][k], one[0][k]), (p, k)
        assert all(sh[p]["proj" + s].tobytes() == one[0]["proj" + s].tobytes() for s in "12") and sh[p]["n_found"] == one[0]["n_found"]


def test_sim3_hostile_input(lr):
    """NaN / Inf / 1e30 in points, distances, poses, M21 and M12: the call returns, every output matches the restatement, guard bytes intact"""
    nf = lr.nf
    vals = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0, -0.0, 3.4e38], F)
    over = {}
    for s, side in (("1", lr.s1[0]), ("2", lr.s2[0])):
        p, dd = side["points"].copy(), side["dist"].copy()
        for j in range(nf // 4):
            (p, dd)[j % 2][4 * j + 1, (j // 2) % 3] = vals[(j // 6) % len(vals)]
        over.update({"points" + s: p, "dist" + s: dd, "flags" + s: side["flags"] | 1})
    T1, T2, M21, M12 = lr.pairs[0]
    bad21 = M21.copy(); bad21[2] = np.nan; bad21[11] = np.inf
    for extra in (dict(), dict(T1w=np.full(12, np.nan, F)), dict(M21=bad21, M12=np.full(12, 1e30, F)), dict(T2w=np.full(12, np.inf, F), M21=np.full(12, -np.inf, F))):
        kw = dict(over); kw.update(extra)
        res, _ = lr.run_sim3(1, 15.0, **kw)
        check_sim3(lr, res[0], 0, 15.0, "hostile", **kw)


def test_sim3_host_form_matcher_and_hand_made_cases(lr):
    cam = cam_struct(TUM1)
    res, _ = lr.run_sim3(1, 4.0, first=1)
    s1, s2, T1, T2, M21, M12 = lr.problem(1)
    side = lambda s, f, T: dict(kps=lr.kps(f), desc=lr.rig.recs[f][1], points=s["points"], dist=s["dist"], mp_desc=s["mp_desc"], flags=s["flags"], Tw=T)
    h = lr.ctx.sim3_search(side(s1, 0, T1), side(s2, 1, T2), M21, M12, cam, lr.bounds, 4.0, lr.sf, lr.rmax)
    for key in [n + s for n in SIM3_INT + ("status",) for s in "12"] + ["match12"]:
        assert np.array_equal(h[key], res[0][key]), key
    assert all(RF.same_bits(h["proj" + s].ravel(), res[0]["proj" + s].ravel()) for s in "12") and h["n_found"] == res[0]["n_found"]
    n, m12, w = ORBmatcher(ctx=lr.ctx).searchBySim3(side(s1, 0, T1), side(s2, 1, T2), M21, M12, cam, lr.bounds, 4.0, lr.sf)
    assert n == res[0]["n_found"] and np.array_equal(m12, res[0]["match12"])
    for name, c, want in RL.handmade_sim3():
        def hs(s):
            kp = np.zeros(len(s["x"]), capi.KP_DTYPE); kp["x"] = s["x"]; kp["y"] = s["y"]
            return dict(kps=kp, desc=s["desc"], points=s["points"], dist=s["dist"], mp_desc=s["mp_desc"], flags=s["flags"], Tw=s["Tw"])
        h = lr.ctx.sim3_search(hs(c["s1"]), hs(c["s2"]), c["M21"], c["M12"], cam_struct(c["cam"]), c["bounds"], c["th"], RU.scale_factors(c["scale_factor"], c["nlevels"]),
                               Context.scale_level_thresholds(c["scale_factor"], c["nlevels"]))
        for key, val in want.items():
            got = h[key] if np.isscalar(h[key]) else h[key].tolist()
            assert got == val, (name, key, got, val)


def sim3_sides(lr, dev):
    """side structs for the argument tests: device buffers (dev) or host arrays, the outputs filled with 0xA5"""
    nf, rg, ctx = lr.nf, lr.rig, lr.ctx
    keep, sides = [], []
    lay = Context.sim3_search_layout(1, nf, nf)
    sent = np.full(lay["bytes"], 0xA5, np.uint8)
    out = capi.DeviceBuffer(lay["bytes"]).upload(sent) if dev else sent.copy()
    optr = out.ptr if dev else out.ctypes.data
    for s, sd, T in (("1", lr.s1[0], lr.pairs[0][0]), ("2", lr.s2[0], lr.pairs[0][1])):
        arrs = [np.ascontiguousarray(a, t) for a, t in ((sd["points"], F), (sd["dist"], F), (sd["mp_desc"], F), (sd["flags"], np.uint8), (T, F))]
        if dev:
            bufs = [capi.DeviceBuffer(a.nbytes + 16).upload(a) for a in arrs]
            ptrs = [b.ptr for b in bufs]
            sides.append(Context.sim3_side(nf, rg.fin[3].ptr, rg.rec.ptr + ctx.desc_off, ctx.rec_bytes, *ptrs, optr, lay, s))
        else:
            bufs = arrs + [lr.kps(0), np.ascontiguousarray(rg.recs[0][1], F)]
            sides.append(Context.sim3_side(nf, None, bufs[6].ctypes.data, 0, *[a.ctypes.data for a in arrs], optr, lay, s, kps=bufs[5].ctypes.data))
        keep.append(bufs)
    return sides, out, lay, sent, keep


SIDE_FIELDS = ("grid", "desc", "points", "dist", "mp_desc", "flags", "Tw", "status", "match", "best_dist", "n_window", "n_tested", "level", "proj_out")


def with_field(side, name, val):
    s = capi.Sim3Side.from_buffer_copy(side)
    setattr(s, name, val)
    return s


def test_sim3_invalid_arguments_launch_nothing(lr):
    L, ctx, nf = lr.rig.L, lr.ctx, lr.nf
    (s1, s2), out, lay, sent, keep = sim3_sides(lr, True)
    M = capi.DeviceBuffer(2 * 48 + 16).upload(np.concatenate([lr.pairs[0][2], lr.pairs[0][3]]))
    cam, gb = cam_struct(TUM1), capi.GridBounds(*lr.bounds)
    sf, rm = lr.sf.copy(), lr.rmax.copy()
    base = dict(ctx=ctx.h, B=1, shared=0, s1=C.byref(s1), s2=C.byref(s2), M21=M.ptr, M12=M.ptr + 48, cam=C.byref(cam), b=C.byref(gb), th=4.0, sf=sf.ctypes.data,
                rm=rm.ctypes.data, nl=NL, high=1000, m12=out.ptr + lay["match12"], nfo=out.ptr + lay["n_found"])

    def call(**kw):
        a = dict(base); a.update(kw)
        return L.xfh_sim3_search_device(*[a[k] for k in base])

    nan, inf = float("nan"), float("inf")
    bad = [dict(B=0), dict(B=-1), dict(B=65536), dict(shared=2), dict(shared=-1), dict(nl=0), dict(nl=17), dict(th=nan), dict(th=inf), dict(th=-inf), dict(ctx=None),
           dict(s1=None), dict(s2=None), dict(M21=None), dict(M12=None), dict(cam=None), dict(b=None), dict(sf=None), dict(rm=None), dict(m12=None), dict(nfo=None),
           dict(M21=M.ptr + 2), dict(m12=base["m12"] + 2), dict(nfo=base["nfo"] + 1)]
    held = []
    for which, side in (("s1", s1), ("s2", s2)):
        for n in (0, -1, capi.GRID_MAX_N + 1):
            held.append(with_field(side, "n", n)); bad.append({which: C.byref(held[-1])})
        for f in SIDE_FIELDS:
            if f != "proj_out":
                held.append(with_field(side, f, None)); bad.append({which: C.byref(held[-1])})
            if f != "flags" and f != "status":
                held.append(with_field(side, f, getattr(side, f) + (8 if f in ("grid", "desc", "mp_desc") else 2))); bad.append({which: C.byref(held[-1])})
        held.append(with_field(side, "desc_stride_bytes", ctx.rec_bytes + 4)); bad.append({which: C.byref(held[-1])})
    for kw in bad:
        assert call(**kw) == 1, kw
    ctx.synchronize()
    assert np.array_equal(out.download(np.uint8, lay["bytes"]), sent)
    nop = with_field(s1, "proj_out", None)
    assert call() == 0 and call(shared=1) == 0 and call(s1=C.byref(nop)) == 0           # the valid calls still work afterwards
    ctx.synchronize()
    assert not np.array_equal(out.download(np.uint8, lay["bytes"]), sent)
    for x in [out, M] + [b for bufs in keep for b in bufs]:
        x.free()


def test_sim3_host_form_invalid_arguments_stage_and_launch_nothing(lr):
    L, ctx, nf = lr.rig.L, lr.ctx, lr.nf
    (s1, s2), out, lay, sent, keep = sim3_sides(lr, False)
    M21, M12 = np.ascontiguousarray(lr.pairs[0][2], F), np.ascontiguousarray(lr.pairs[0][3], F)
    cam, gb = cam_struct(TUM1), capi.GridBounds(*lr.bounds)
    badb = [capi.GridBounds(*b) for b in ((0, 0, 0, 480), (0, 480, 640, 0), (float("nan"), 0, 640, 480), (0, 0, float("inf"), 480))]
    sf, rm = lr.sf.copy(), lr.rmax.copy()
    base = dict(ctx=ctx.h, s1=C.byref(s1), s2=C.byref(s2), M21=M21.ctypes.data, M12=M12.ctypes.data, cam=C.byref(cam), b=C.byref(gb), th=4.0, sf=sf.ctypes.data,
                rm=rm.ctypes.data, nl=NL, high=1000, m12=out.ctypes.data + lay["match12"], nfo=out.ctypes.data + lay["n_found"])

    def call(**kw):
        a = dict(base); a.update(kw)
        return L.xfh_sim3_search(*[a[k] for k in base])

    nan, inf = float("nan"), float("inf")
    bad = [dict(nl=0), dict(nl=17), dict(th=nan), dict(th=inf), dict(ctx=None), dict(s1=None), dict(s2=None), dict(M21=None), dict(M12=None), dict(cam=None), dict(b=None),
           dict(sf=None), dict(rm=None), dict(m12=None), dict(nfo=None)] + [dict(b=C.byref(x)) for x in badb]
    held = []
    for which, side in (("s1", s1), ("s2", s2)):
        for n in (0, -1, capi.GRID_MAX_N + 1):
            held.append(with_field(side, "n", n)); bad.append({which: C.byref(held[-1])})
        for f in ("kps",) + SIDE_FIELDS[1:-1]:
            held.append(with_field(side, f, None)); bad.append({which: C.byref(held[-1])})
    ctx.synchronize()
    ctx.timing_enable(capi.K["GRID_BUILD"])
    for kw in bad:
        assert call(**kw) == 1, kw
    assert ctx.timing_read()[0] == 0 and np.array_equal(out, sent)
    nop = with_field(s2, "proj_out", None)
    assert call() == 0 and call(s2=C.byref(nop)) == 0                                  # the valid calls still work afterwards
    assert ctx.timing_read()[0] == 4 and not np.array_equal(out, sent)
    ctx.timing_enable(capi.K["NONE"])
