"""OptimizeSim3 inside the loop-detection chain of LoopClosing::DetectCommonRegionsFromBoW (src/LoopClosing.cc:746-777), every step on ONE set of
device buffers with nothing read back between the calls:
  xfh_sim3_solve_device -> coarse xfh_map_projection_search_device (th 8, 1.5 TH_LOW) fed the solver's d_Tcw / d_Ow
  -> xfh_sim3_optimize_device fed the solver's d_floats + 12 (stride XFH_SIM3_SOLVE_FLOATS, optimised in place), the coarse search's d_assigned and
     its FLAG_ACTIVE bytes -> fine xfh_map_projection_search_device (th 5, TH_LOW) fed the optimiser's d_Tcw / d_Ow,
against the same chain made of the Python rules (ref_sim3solve.rule, ref_loop.map_project + map_search, ref_optsim3.rule).  The integer outputs of
both searches must be equal; the optimiser's outputs agree under the comparison rules of tests/test_gpu_optsim3.py.

The scene.  The current keyframe is frame 0 of tests/loop_rig.py at pose 0, its map points the rig's query block; the candidate keyframe (which is
also pMostBoWMatchesKF) sits at pose 0 as well, so the true S12 is the identity, and the solver's scene is made with a small similarity (0.3 degrees,
1 cm, scale 1.02) that the optimiser has to take back.  Side 1 of the optimiser: keypoint i owns the point its ray was made from.  Side 2: every
query is seen in KF2 where it projects.  The condition, checked here on the CPU with the Python rules alone: the fine search's integer outputs do
not change when the pose it is fed moves by SIM3OPT_TOL in any direction tried (all entries up, all down, random signs)."""
import numpy as np
import pytest

import guarded
import optsim3_rig as OG
import ref_fuse as RU
import ref_loop as RL
import ref_optsim3 as RO
import ref_sim3solve as R
import sim3solve_rig as G
from loop_rig import MAP_INT, LoopRig
from projection_rig import GUARD, TUM1, cam_struct
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64
CAM4 = tuple(float(TUM1[k]) for k in ("fx", "fy", "cx", "cy"))
TH2 = 10.0


@pytest.fixture(scope="module")
def lr(gpu_lib, weights_dense, oracle_mod):
    r = LoopRig(gpu_lib, weights_dense[1], 1000, 901, oracle_mod)
    yield r
    r.close()


def search_rule(lr, blk, Tcw, Ow, th, accept):
    """the Python rules of one map projection search of frame 0 -> its integer outputs"""
    u, v, r, level, st = RL.map_project(Tcw, Ow, TUM1, lr.bounds, th, 1.2, 8, RL.FORM_SIM3, blk["xyz"], blk["normals"], blk["dist"])
    act = (np.asarray(blk["flags"]) & 1) != 0
    st, level = np.where(act, st, RL.INACTIVE).astype(np.uint8), np.where(act, level, -1).astype(np.int32)
    m = lr.model_map(0, st, level, u, v, r, blk, accept)
    m["level"] = level
    return m


def moved(a, blocks, steps, sign):
    """a with every entry of each block moved by `steps` float32 steps at the block's largest magnitude, in the direction sign gives per entry"""
    a = np.asarray(a, F).copy()
    for blk in blocks:
        a[blk] = (a[blk].astype(D) + sign[blk] * steps * float(np.spacing(F(np.abs(a[blk]).max())))).astype(F)
    return a


def optimiser_problem(lr, sc, blk, assigned, S12):
    nf = lr.nf
    T0 = np.asarray(lr.poses[0], D).reshape(3, 4)
    xyz0 = RU.scene(lr.seed, lr.rig.xy[0], TUM1, lr.poses[0], lr.rmax)[0]                     # the point each keypoint's ray was made from
    P1c = xyz0.astype(D) @ T0[:, :3].T + T0[:, 3]
    T1 = np.asarray(sc["T1w"], D).reshape(3, 4)
    points1 = ((P1c - T1[:, 3]) @ T1[:, :3]).astype(F)
    P2c = np.asarray(blk["xyz"], D) @ T0[:, :3].T + T0[:, 3]
    with np.errstate(all="ignore"):
        xy2 = np.stack([CAM4[0] * P2c[:, 0] / P2c[:, 2] + CAM4[2], CAM4[1] * P2c[:, 1] / P2c[:, 2] + CAM4[3]], 1)
    return dict(T1w=np.asarray(sc["T1w"], F).reshape(12), xy_un1=lr.rig.xy[0].astype(F), point1=np.arange(nf, dtype=np.int32), points1=points1,
                assigned=np.asarray(assigned, np.int32), points2=np.asarray(blk["xyz"], F), flags2=np.asarray(blk["flags"], np.uint8),
                index2=np.arange(nf, dtype=np.int32), xy_un2=np.nan_to_num(xy2, posinf=0, neginf=0).astype(F), T2w=np.asarray(lr.poses[0], F).reshape(12),
                S12=np.asarray(S12, F), Tmw=np.asarray(lr.poses[0], F).reshape(12), cam1=CAM4, cam2=CAM4, th2=TH2, fix_scale=0, all_points=1, inv_sigma2_1=1.0,
                inv_sigma2_2=1.0)


def test_solve_search_optimise_search_on_one_set_of_device_buffers(lr):
    sc = G.scene(50, inlier_frac=0.9, deg=0.3, tmax=0.01, scale=1.02, T2w=lr.poses[0])
    rule_s = G.rule_of(sc)
    assert rule_s["header"][1] == R.CONVERGED
    nf, ctx, r = lr.nf, lr.ctx, lr.rig
    blk = lr.block(0)
    acc_c, acc_f = float(F(RL.TH_LOW) * F(1.5)), float(F(RL.TH_LOW) * F(1.0))
    # ---- the chain of the Python rules
    coarse = search_rule(lr, blk, rule_s["Tcw"], rule_s["Ow"], 8.0, acc_c)
    p = optimiser_problem(lr, sc, blk, coarse["assigned"], rule_s["floats"][12:25])
    rule_o = RO.rule(p)
    assert rule_o["header"][0] > 100 and rule_o["header"][6] >= 10 and rule_o["header"][7] == 2, rule_o["header"]
    fine = search_rule(lr, blk, rule_o["Tcw"], rule_o["Ow"], 5.0, acc_f)
    assert fine["n_matches"] > 100
    # ---- the condition: the fine search does not see a pose that moved by SIM3OPT_TOL
    rng = np.random.RandomState(3)
    for sign_T, sign_O in ((np.ones(12), np.ones(3)), (-np.ones(12), -np.ones(3)), (rng.choice([-1.0, 1.0], 12), rng.choice([-1.0, 1.0], 3))):
        alt = search_rule(lr, blk, moved(rule_o["Tcw"], RO.TCW_BLOCKS, OG.SIM3OPT_TOL.tcw, sign_T), moved(rule_o["Ow"], (slice(0, 3),), OG.SIM3OPT_TOL.ow, sign_O),
                          5.0, acc_f)
        for k in MAP_INT + ("assigned", "status"):
            assert np.array_equal(alt[k], fine[k]), ("the fine search is sensitive to SIM3OPT_TOL in this scene", k)
    # ---- the chain on the device
    d = [lr.dev(np.ascontiguousarray(blk[k], t)) for k, t in (("xyz", F), ("normals", F), ("dist", F), ("qdesc", F), ("flags", np.uint8), ("taken", np.uint8))]
    ins = [lr.dev(np.ascontiguousarray(a)) for a in (sc["points"], sc["point1"], sc["matched"], sc["T1w"], sc["T2w"], sc["table"], sc["draws"][0])]
    n1s, M = len(sc["point1"]), len(sc["points"])
    lay_s = Context.sim3_solve_layout(1, n1s, GUARD)
    out_s = guarded.outputs(lay_s, keep=lr.bufs)
    ws_s = lr.dev(np.zeros(capi.lib().xfh_sim3_solve_workspace_bytes(n1s, M, 1), np.uint8))
    lay = Context.map_projection_search_layout(1, nf, nf, GUARD)
    out_c, out_f = guarded.outputs(lay, keep=lr.bufs), guarded.outputs(lay, keep=lr.bufs)
    ws = lr.dev(np.zeros(Context.map_projection_search_workspace_bytes(nf, nf, 1), np.uint8))
    side1 = [lr.dev(p[k]) for k in ("T1w",)] + [None] + [lr.dev(p[k]) for k in ("point1", "points1")]
    i2, xy2 = lr.dev(p["index2"]), lr.dev(p["xy_un2"])
    off = Context.sim3_optimize_layout(1, nf, GUARD)                        # (its S12_out stays unwritten: the optimiser rewrites the solver's record in place)
    out_o = guarded.outputs(off, keep=lr.bufs)
    ws_o = lr.dev(np.zeros(ctx.sim3_optimize_workspace_bytes(nf, 1), np.uint8))
    cam, S12_ptr = cam_struct(TUM1), out_s.ptr + lay_s["floats"] + 48
    search = lambda Tp, Op, th, accept, o: ctx.map_projection_search_device(
        RL.FORM_SIM3, 1, nf, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, Tp, Op, cam, lr.bounds, th, lr.sf, lr.rmax, r.fin[3].ptr, r.rec.ptr + ctx.desc_off,
        ctx.rec_bytes, 0, nf, ws.ptr, o.ptr, d_taken=d[5].ptr, accept_max=accept, guard=GUARD)
    try:
        ctx.sim3_solve_device(1, n1s, M, ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, 0, ins[4].ptr, G.camera(sc["cam1"]), G.camera(sc["cam2"]), ins[5].ptr,
                              len(sc["draws"][0]), ins[6].ptr, 0, G.RAND_MAX, ws_s.ptr, out_s.ptr, min_inliers=sc["min_inliers"], guard=GUARD)
        search(out_s.ptr + lay_s["Tcw"], out_s.ptr + lay_s["Ow"], 8.0, acc_c, out_c)
        ctx.sim3_optimize_device(1, nf, nf, nf, nf, False, [side1[0].ptr, r.fin[0].ptr, side1[2].ptr, side1[3].ptr],
                                 [out_c.ptr + lay["assigned"], d[0].ptr, d[4].ptr, i2.ptr, xy2.ptr, ins[4].ptr], S12_ptr, capi.SIM3_SOLVE_FLOATS, ins[4].ptr, cam, cam,
                                 ws_o.ptr, out_o.ptr + off["assigned_out"], out_o.ptr + off["status"], out_o.ptr + off["chi2"], out_o.ptr + off["state"], S12_ptr,
                                 capi.SIM3_SOLVE_FLOATS, out_o.ptr + off["Tcw"], out_o.ptr + off["Ow"], out_o.ptr + off["header"], out_o.ptr + off["final_chi2"],
                                 th2=TH2, fix_scale=False, all_points=True)
        search(out_o.ptr + off["Tcw"], out_o.ptr + off["Ow"], 5.0, acc_f, out_f)
        ctx.synchronize()                                                   # the only wait of the chain
        raw_c, raw_f = guarded.download(out_c, lay), guarded.download(out_f, lay)
        got_o = guarded.problems(off.parse(guarded.download(out_o, off, skip=("S12_out",))), 1)[0]
        got_s = lay_s.parse(guarded.download(out_s, lay_s))
    finally:
        lr.free()
    got_o["S12_out"] = got_s["floats"][0, 12:25].copy()
    # the solver's record: everything but the 13 floats the optimiser rewrote in place is the solver's
    keep = np.r_[0:12, 25:capi.SIM3_SOLVE_FLOATS]
    assert np.array_equal(got_s["floats"][0, keep].view(np.int32), np.asarray(rule_s["floats"], F)[keep].view(np.int32))
    assert np.array_equal(got_s["header"][0], rule_s["header"]) and np.array_equal(got_s["Tcw"][0].view(np.int32), np.asarray(rule_s["Tcw"], F).view(np.int32))

    def ints(raw, model, tag):
        for k in MAP_INT + ("assigned",):
            a = raw[lay[k]:lay[k] + 4 * nf].view(np.int32)
            assert np.array_equal(a, model[k]), (tag, k, int((a != model[k]).sum()))
        assert np.array_equal(raw[lay["status"]:lay["status"] + nf], model["status"]), tag
        assert int(raw[lay["n_matches"]:lay["n_matches"] + 4].view(np.int32)[0]) == model["n_matches"], tag
    ints(raw_c, coarse, "coarse")
    print("optimiser in the chain:", dict(zip(RO.H_KEYS, got_o["header"][:12].tolist())), "distances", RO.distances(got_o, rule_o, TH2))
    bad = RO.outputs_agree(got_o, rule_o, OG.SIM3OPT_TOL)
    assert bad == [], bad
    ints(raw_f, fine, "fine")
    print("chain: coarse matches", coarse["n_matches"], "-> OptimizeSim3 returns", int(got_o["header"][6]), "of", int(got_o["header"][0]), "-> fine matches", fine["n_matches"])
