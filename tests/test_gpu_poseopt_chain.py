"""search -> optimise -> search on the device, on the scene of tests/projection_rig.py: xfh_search_projection_device writes `assigned`,
xfh_pose_optimize_device reads it with the frame's xy_un / uright and the world points and writes the pose and the outlier flags,
xfh_search_projection_device runs again with that pose as d_Tcw and the flags as d_skip (a flagged keypoint is not matched again; query flags are
indexed by map point, the outlier flags by keypoint, so d_skip is where they go without a host step).  Three calls queued on the ctx stream, ONE
synchronisation at the end.  Compared stage by stage with the restatements, each stage's model evaluated on what the device handed it."""
import ctypes as C

import numpy as np
import pytest

import guarded
import ref_poseopt as RPO
import ref_projection as RP
from projection_rig import BIG, F, GUARD, OUT_INT, TUM1, Rig, cam_struct
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context

pytestmark = pytest.mark.gpu
SEED, NF, RADIUS = 902, 1000, 5.0                                      # chosen on the device: the optimisation of this chain holds the rig's condition
CAM5 = tuple(float(TUM1[k]) for k in ("fx", "fy", "cx", "cy", "bf"))


@pytest.fixture(scope="module")
def rig(gpu_lib, weights_dense):
    r = Rig(gpu_lib, weights_dense[1], NF, SEED)
    yield r
    r.close()


def chain(rig, radius):
    """-> (search 1, pose optimisation, search 2) as dicts of host arrays"""
    nf, ctx, L = rig.nf, rig.ctx, rig.L
    lay, play = Context.search_projection_layout(1, nf, nf, GUARD), Context.pose_optimize_layout(1, nf, GUARD)
    outs, po = [guarded.outputs(lay) for _ in range(2)], guarded.outputs(play)
    ws = guarded.Guarded(Context.search_projection_workspace_bytes(nf, nf, 1), GUARD)
    pws = guarded.Guarded(int(L.xfh_pose_optimize_workspace_bytes(nf, 1)), GUARD)
    qd, dp, dfl, dT = rig.dev(rig.recs[0][1]), rig.dev(np.ascontiguousarray(rig.xyz, F)), rig.dev(np.ascontiguousarray(rig.flags, np.uint8)), rig.dev(rig.poses[0])
    cam = cam_struct(TUM1)
    grids, targets = rig.fin[3].ptr + ctx.grid_bytes(nf), rig.rec.ptr + ctx.rec_bytes + ctx.desc_off
    kw = dict(radius=radius, cam=cam, bounds=rig.bounds, init_dist=BIG, th_high=1000, nn_ratio=0.0, guard=GUARD)
    ctx.search_projection_device(capi.PROJ_POINTS, 1, nf, dp.ptr, qd.ptr, dfl.ptr, grids, targets, ctx.rec_bytes, nf, ws.ptr, outs[0].ptr, d_Tcw=dT.ptr, **kw)
    rc = L.xfh_pose_optimize_device(ctx.h, 1, nf, nf, dT.ptr, C.byref(cam), rig.fin[0].ptr + 8 * nf, rig.fin[1].ptr + 4 * nf, outs[0].ptr + lay["assigned"], dp.ptr, 1.0,
                                    pws.ptr, *[po.ptr + play[k] for k in play.names])
    assert rc == 0
    ctx.search_projection_device(capi.PROJ_POINTS, 1, nf, dp.ptr, qd.ptr, dfl.ptr, grids, targets, ctx.rec_bytes, nf, ws.ptr, outs[1].ptr, d_Tcw=po.ptr + play["Tcw_out"],
                                 d_skip=po.ptr + play["outlier"], **kw)
    ctx.synchronize()                                                     # the only one
    res = [guarded.problems(lay.parse(guarded.download(o, lay)), 1)[0] for o in outs]
    pose = guarded.problems(play.parse(guarded.download(po, play)), 1)[0]
    ws.download(); pws.download()
    for b in outs + [ws, po, pws] + rig.bufs:
        b.free()
    rig.bufs = []
    return res[0], pose, res[1]


def search_model(rig, O, Tcw, radius, skip=None):
    u, v, ur, st = RP.project(Tcw, TUM1, rig.bounds, rig.xyz)
    st = np.where(rig.flags & 1, st, RP.INACTIVE).astype(np.uint8)
    return RP.search(O, st, (rig.flags & 2) != 0, u, v, F(radius), ur, rig.recs[0][1], rig.grids[1], rig.xy[1][:, 0].copy(), rig.xy[1][:, 1].copy(), rig.bounds,
                     rig.recs[1][1], skip=skip, init_dist=BIG, th_high=1000, nn_ratio=0.0)


def same_search(res, m, tag):
    for k in OUT_INT + ("assigned",):
        assert np.array_equal(res[k], m[k]), (tag, k, np.nonzero(res[k] != m[k])[0][:8])
    assert res["n_matches"] == m["n_matches"] and np.array_equal(res["status"] >= RP.VISIBLE, m["status"] >= RP.VISIBLE), tag


def test_search_optimise_search_on_the_device(rig, oracle_mod):
    s1, po, s2 = chain(rig, RADIUS)
    same_search(s1, search_model(rig, oracle_mod, rig.poses[0], RADIUS), "first search")
    m = RPO.rule(rig.poses[0], CAM5, rig.xy[1], rig.ur[1], s1["assigned"], rig.xyz, 1.0)
    print(f"chain: matches {s1['n_matches']} -> edges {m['header'].tolist()}, reasons {m['reasons']}, margins { {k: f'{v:.1e}' for k, v in m['margins'].items()} } "
          f"-> matches {s2['n_matches']}; final chi2 {po['final_chi2']:.17g} (rule {m['final_chi2']:.17g})")
    assert min(m["margins"].values()) > 1e-9, m["margins"]              # the scene holds the rig's condition, so the decisions can be compared
    assert m["header"][0] >= 100 and 0 < m["header"][1] < m["header"][0]
    assert np.array_equal(po["header"], m["header"]) and np.array_equal(po["outlier"], m["outlier"])
    assert RPO.ulps(po["Tcw_out"], m["Tcw_out"]).max() <= 1 and RPO.ulps(po["chi2"], m["chi2"]).max() <= 1
    same_search(s2, search_model(rig, oracle_mod, po["Tcw_out"], RADIUS, skip=po["outlier"]), "second search")
    k = np.nonzero(po["outlier"])[0]
    assert np.all(s2["assigned"][k] == -1) and s2["n_matches"] > 0        # a flagged keypoint takes no map point in the second search
