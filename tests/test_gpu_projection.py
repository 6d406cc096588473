"""xfh_search_projection_device (k_proj_candidates / k_proj_resolve / k_proj_count) against the sequential restatement
tests/ref_projection.py on the scene and with the guarded runs of tests/projection_rig.py, stage by stage: proj against the model's projection of the same points, then the culls, then the matches
of the model evaluated on the DEVICE's own proj and statuses -- so one failure names one stage.  Every comparison is equality of
bits and integers.

Scenes: frames extracted on the device (synth.image of a seed and shifted copies), finished with the TUM1 camera (undistorted
keypoints, uright from a seeded depth image, the grid of the finish); world points from the last frame's undistorted keypoints and a
seeded depth, a small seeded pose per problem.  The synthetic weights' descriptors are weakly discriminative (tests/test_projection_ref.py
prints the figures): under the reference's init_dist = 256 few queries find a match at all, so the scenes are searched with
init_dist = 1 << 30 and th_high = 1000, where most do and the claim order decides a large share of them, and with 256 as well."""
import ctypes as C

import numpy as np
import pytest

import ref_frame as RF
import ref_projection as RP
import ref_window as RW
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context

pytestmark = pytest.mark.gpu

from projection_rig import BIG, F, OUT_INT, TUM1, Rig, cam_struct


def same(res, m, tag):
    for k in OUT_INT + ("assigned", "status"):
        assert np.array_equal(res[k], m[k]), (tag, k, np.nonzero(res[k] != m[k])[0][:8])
    assert res["n_matches"] == m["n_matches"], tag


def check_points(rig, O, B, r, tag, **kw):
    """POINTS mode, stage by stage"""
    nf = rig.nf
    res, raw, pj, hdr = rig.run(B, capi.PROJ_POINTS, np.tile(rig.xyz, (B, 1)), np.tile(rig.flags, B), radius=r, **kw)
    for p in range(B):
        u, v, ur, st = RP.project(rig.poses[p], TUM1, rig.bounds, rig.xyz)
        act = (rig.flags & 1) != 0
        for j, a in enumerate((u, v, ur)):                                           # stage 1: proj
            assert RF.same_bits(pj[p][act, j], a[act]), (tag, "proj", p, j)
        assert np.all(pj[p][~act] == 0)
        st = np.where(act, st, RP.INACTIVE).astype(np.uint8)
        dst = res[p]["status"]
        assert np.array_equal(dst >= RP.VISIBLE, st == RP.VISIBLE) and np.array_equal(dst[st != RP.VISIBLE], st[st != RP.VISIBLE]), (tag, "cull", p)     # stage 2
        st_dev = np.where(dst >= RP.VISIBLE, RP.VISIBLE, dst).astype(np.uint8)
        m = rig.model(O, p, st_dev, pj[p][:, 0].copy(), pj[p][:, 1].copy(), F(r), pj[p][:, 2].copy(), **kw)             # stage 3, on the DEVICE's proj
        same(res[p], m, (tag, p))
        print(f"{tag} p={p} r={r}: visible {(st == RP.VISIBLE).sum()}, matched {m['n_matches']}, rejected {(m['status'] == RP.REJECTED).sum()}, "
              f"no candidates {(m['status'] == RP.NO_CANDIDATES).sum()}, rounds {hdr[p][0]}, searched again {hdr[p][1]}")
    return res, raw


@pytest.fixture(scope="module", params=[(900, 4096), (901, 1000)])
def rig(request, gpu_lib, weights_dense):
    r = Rig(gpu_lib, weights_dense[1], request.param[1], request.param[0])
    yield r
    r.close()


@pytest.mark.parametrize("r", [7.0, 15.0, 30.0])
def test_points_mode_matches_the_sequential_loop(rig, oracle_mod, r):
    res, raw = check_points(rig, oracle_mod, 1, r, "plain")
    assert res[0]["n_matches"] > rig.nf // 4 and (res[0]["status"] == RP.MATCHED).sum() == res[0]["n_matches"]
    # two runs of the same input give identical bytes in every output (the workspace of the second starts from other bytes)
    res2, raw2, _, _ = rig.run(1, capi.PROJ_POINTS, rig.xyz, rig.flags, radius=r, fill=0x3C)
    assert np.array_equal(raw, raw2)
    # the share of visible queries whose match the claim order decides on the DEVICE's extraction: printed, not asserted -- the 5 % bound
    # is held where the seeds were chosen, on the CPU (tests/test_projection_ref.py); every output above is already compared by equality
    u, v, ur, st = RP.project(rig.poses[0], TUM1, rig.bounds, rig.xyz)
    st = np.where(rig.flags & 1, st, RP.INACTIVE).astype(np.uint8)
    free = rig.model(oracle_mod, 0, st, u, v, F(r), ur, claims=np.zeros(rig.nf, bool))
    act = st == RP.VISIBLE
    share = float(np.mean(free["match_idx"][act] != res[0]["match_idx"][act]))
    print(f"r={r}: match_idx differs from the claim-free answer for {share:.3f} of the visible queries")
    check_points(rig, oracle_mod, 1, r, "ratio+skip+uright", ratio=0.9, skip=True, uright=True)
    check_points(rig, oracle_mod, 1, r, "init256+uright", init=256, uright=True)
    check_points(rig, oracle_mod, 1, r, "ratio+skip", ratio=0.9, skip=True, init=256)


def test_four_problems_with_their_own_poses(rig, oracle_mod):
    res, _ = check_points(rig, oracle_mod, 4, 15.0, "B=4", skip=True, uright=True)
    assert len({r["n_matches"] for r in res}) > 1
    one, _, _, _ = rig.run(1, capi.PROJ_POINTS, rig.xyz, rig.flags, radius=15.0, skip=True, uright=True)
    same(one[0], res[0], "B=1 against problem 0 of B=4")


@pytest.mark.parametrize("r", [7.0, 15.0, 30.0])
def test_given_mode(rig, oracle_mod, r):
    nf = rig.nf
    u, v, ur, _ = RP.project(rig.poses[0], TUM1, rig.bounds, rig.xyz)
    rq = (F(r) + (np.random.RandomState(5).rand(nf) < 0.3).astype(F) * F(2.5)).astype(F)          # a radius per query
    uvr = np.stack([u, v, rq], 1).astype(F)
    st = np.where(rig.flags & 1, RP.VISIBLE, RP.INACTIVE).astype(np.uint8)
    for tag, kw, uq in (("given", dict(), None), ("given+uright+ratio", dict(uright=True, ratio=0.9, skip=True), ur), ("given256", dict(init=256, skip=True), None)):
        res, _, pj, hdr = rig.run(1, capi.PROJ_GIVEN, uvr, rig.flags, ur_query=uq, **kw)
        act = st == RP.VISIBLE
        assert RF.same_bits(pj[0][act, 0], u[act]) and RF.same_bits(pj[0][act, 1], v[act]) and RF.same_bits(pj[0][act, 2], (ur if uq is not None else np.zeros(nf, F))[act])
        m = rig.model(oracle_mod, 0, st, u, v, rq, ur, **kw)
        same(res[0], m, tag)
        print(f"{tag} r={r}: matched {m['n_matches']}, rounds {hdr[0][0]}, searched again {hdr[0][1]}")
    # all claim bits clear, no skip mask: xfh_search_window_device on the same uvr
    flags = np.ones(nf, np.uint8)
    res, _, _, hdr = rig.run(1, capi.PROJ_GIVEN, uvr, flags, ur_query=ur, uright=True, init=256)
    assert hdr[0][0] <= 2
    ctx = rig.ctx
    du = capi.DeviceBuffer(uvr.nbytes).upload(uvr); dq = capi.DeviceBuffer(ur.nbytes).upload(ur); out = capi.DeviceBuffer(20 * nf)
    ctx.search_window_device(rig.rec.ptr + ctx.desc_off, du.ptr, nf, rig.fin[3].ptr + ctx.grid_bytes(nf), rig.rec.ptr + ctx.rec_bytes + ctx.desc_off, nf,
                             out.ptr, 256, d_uright=rig.fin[1].ptr + 4 * nf, d_ur_query=dq.ptr)
    ctx.synchronize()
    bi, bd, si, sd, nc = out.download(np.int32, 5 * nf).reshape(5, nf)
    assert np.array_equal(res[0]["best_dist"], bd) and np.array_equal(res[0]["second_dist"], sd) and np.array_equal(res[0]["n_candidates"], nc)
    assert np.array_equal(res[0]["match_idx"], bi)                                        # best_idx >= 0 means dist < 256 <= th_high: accepted
    assert res[0]["n_matches"] == (bi >= 0).sum()
    for x in (du, dq, out):
        x.free()


def test_deep_chain_every_query_takes_the_next_best(gpu_lib, oracle_mod):
    """2048 queries with ONE descriptor on one spot, 4096 keypoints inside the window, every query claims: query q gets the
    keypoint of rank q, the K-lists are exhausted from the fifth query on and the round loop runs its worst case"""
    nq, nt = 2048, 4096
    rng = np.random.RandomState(3)
    k = np.zeros(nt, capi.KP_DTYPE); k["size"] = 1; k["angle"] = -1
    k["x"] = rng.uniform(270, 330, nt).astype(F); k["y"] = rng.uniform(170, 230, nt).astype(F)
    tg = rng.randn(nt, 64); tg = (tg / np.linalg.norm(tg, axis=1, keepdims=True)).astype(F)
    q1 = rng.randn(64); q1 = (q1 / np.linalg.norm(q1)).astype(F)
    qd = np.tile(q1, (nq, 1))
    qd[1500:] = tg[7]                                                   # a second group with another order of preference
    uvr = np.tile(np.array([300, 200, 40], F), (nq, 1))
    flags = np.full(nq, 3, np.uint8)
    b = (0.0, 0.0, 640.0, 480.0)
    ctx = Context(nfeatures=64, max_height=32, max_width=32)
    res = ctx.search_projection(capi.PROJ_GIVEN, uvr, qd, flags, k, b, tg, init_dist=BIG, th_high=BIG)
    x, y = k["x"].copy(), k["y"].copy()
    m = RP.search(oracle_mod, np.full(nq, RP.VISIBLE, np.uint8), np.ones(nq, bool), uvr[:, 0], uvr[:, 1], uvr[:, 2], np.zeros(nq, F), qd,
                  RW.build(x, y, b), x, y, b, tg, init_dist=BIG, th_high=BIG)
    assert m["n_matches"] == nq and len(set(m["match_idx"].tolist())) == nq and np.array_equal(m["n_candidates"], nt - np.arange(nq))
    same(res, m, "deep chain")
    ctx.close()


def test_hostile_points_and_poses(rig, oracle_mod):
    """points and poses filled with NaN / Inf / 1e38: the call returns, statuses match the restatement, guard words are intact
    (Rig.run checks them)"""
    nf = rig.nf
    vals = np.array([np.nan, np.inf, -np.inf, 1e38, -1e38, 0.0, -0.0, 3.4e38], F)
    xyz = rig.xyz.copy()
    for j in range(nf // 3):
        xyz[3 * j, j % 3] = vals[(j // 3) % len(vals)]
    flags = rig.flags | 1
    keep = rig.poses.copy()
    try:
        for T in (keep[0], np.full(12, np.nan, F), np.full(12, np.inf, F), np.full(12, 1e38, F)):
            rig.poses = keep.copy(); rig.poses[0] = T
            res, _, pj, _ = rig.run(1, capi.PROJ_POINTS, xyz, flags, radius=15.0, uright=True)
            u, v, ur, st = RP.project(T, TUM1, rig.bounds, xyz)
            assert RF.same_bits(pj[0][:, 0], u) and RF.same_bits(pj[0][:, 1], v) and RF.same_bits(pj[0][:, 2], ur)
            m = rig.model(oracle_mod, 0, st, u, v, F(15.0), ur, uright=True)
            same(res[0], m, "hostile")
        # GIVEN mode: hostile (u, v, r) and right coordinates
        uvr = np.stack([u, v, np.full(nf, 15, F)], 1)
        uvr[::5, 2] = vals[np.arange(len(uvr[::5])) % len(vals)]
        urq = ur.copy(); urq[::7] = np.nan
        rig.poses = keep
        res, _, _, _ = rig.run(1, capi.PROJ_GIVEN, uvr, flags, ur_query=urq, uright=True)
        m = rig.model(oracle_mod, 0, np.full(nf, RP.VISIBLE, np.uint8), uvr[:, 0].copy(), uvr[:, 1].copy(), uvr[:, 2].copy(), urq, uright=True)
        same(res[0], m, "hostile given")
    finally:
        rig.poses = keep


def test_host_form_equals_the_device_form(rig):
    nf = rig.nf
    res, _, pj, _ = rig.run(1, capi.PROJ_POINTS, rig.xyz, rig.flags, radius=15.0, skip=True, uright=True, ratio=0.9)
    k = np.zeros(nf, capi.KP_DTYPE); k["x"] = rig.xy[1][:, 0]; k["y"] = rig.xy[1][:, 1]
    h = rig.ctx.search_projection(capi.PROJ_POINTS, rig.xyz, rig.recs[0][1], rig.flags, k, rig.bounds, rig.recs[1][1], radius=15.0, Tcw=rig.poses[0],
                                  cam=cam_struct(TUM1), skip=rig.skip[0], uright=rig.ur[1], init_dist=BIG, nn_ratio=0.9)
    same(h, res[0], "host form")
    assert RF.same_bits(h["proj"], pj[0])


def test_invalid_arguments_launch_nothing(rig):
    L, ctx, nf = rig.L, rig.ctx, rig.nf
    lay = Context.search_projection_layout(1, nf, nf)
    sent = np.full(lay["bytes"], 0xA5, np.uint8)
    out = capi.DeviceBuffer(lay["bytes"]).upload(sent)
    ws = capi.DeviceBuffer(Context.search_projection_workspace_bytes(nf, nf, 1))
    pts = capi.DeviceBuffer(nf * 12 + 16).upload(rig.xyz); fl = capi.DeviceBuffer(nf + 16).upload(rig.flags); T = capi.DeviceBuffer(64).upload(rig.poses[0])
    cam, gb = cam_struct(TUM1), capi.GridBounds(*rig.bounds)
    base = dict(ctx=ctx.h, mode=capi.PROJ_POINTS, B=1, nq=nf, pts=pts.ptr, urq=None, T=T.ptr, cam=C.byref(cam), b=C.byref(gb), radius=15.0, qd=rig.rec.ptr + ctx.desc_off,
                fl=fl.ptr, grids=rig.fin[3].ptr + ctx.grid_bytes(nf), tg=rig.rec.ptr + ctx.rec_bytes + ctx.desc_off, stride=ctx.rec_bytes, nt=nf, skip=None,
                ur=None, init=256, th=1000, ratio=0.0, ws=ws.ptr, st=out.ptr + lay["status"], mi=out.ptr + lay["match_idx"], bd=out.ptr + lay["best_dist"],
                sd=out.ptr + lay["second_dist"], nc=out.ptr + lay["n_candidates"], pj=None, asg=out.ptr + lay["assigned"], nm=out.ptr + lay["n_matches"])

    def call(**kw):
        a = dict(base); a.update(kw)
        return L.xfh_search_projection_device(*[a[k] for k in base])

    nan, inf = float("nan"), float("inf")
    bad = [dict(B=0), dict(B=-1), dict(nq=0), dict(nq=capi.GRID_MAX_N + 1), dict(nt=0), dict(nt=capi.GRID_MAX_N + 1), dict(mode=2), dict(mode=-1),
           dict(mode=capi.PROJ_GIVEN, urq=pts.ptr), dict(mode=capi.PROJ_GIVEN, ur=rig.fin[1].ptr),                  # only one of the uright pair
           dict(qd=base["qd"] + 4), dict(tg=base["tg"] + 8), dict(stride=ctx.rec_bytes + 4), dict(grids=base["grids"] + 8), dict(ws=ws.ptr + 4),
           dict(pts=pts.ptr + 2), dict(mi=base["mi"] + 2), dict(asg=base["asg"] + 1), dict(nm=base["nm"] + 2), dict(T=T.ptr + 2),
           dict(radius=nan), dict(radius=inf), dict(ratio=-0.5), dict(ratio=nan),
           dict(T=None), dict(cam=None), dict(b=None), dict(ctx=None), dict(pts=None), dict(qd=None), dict(fl=None), dict(ws=None), dict(st=None), dict(nm=None)]
    for kw in bad:
        assert call(**kw) == 1, kw
    ctx.synchronize()
    assert np.array_equal(out.download(np.uint8, lay["bytes"]), sent)
    assert call() == 0                                                                     # the valid call still works afterwards
    ctx.synchronize()
    assert not np.array_equal(out.download(np.uint8, lay["bytes"]), sent)
    for x in (out, ws, pts, fl, T):
        x.free()
