"""The Sim3 solver inside the place-recognition chain of LoopClosing::DetectCommonRegionsFromBoW, every step on ONE set of device buffers with
nothing read back between the calls:
  xfh_bow_search_device (shared = 1, the current keyframe against J = 3 covisibles, the scene of tests/bow_rig.py) -> xfh_sim3_merge_matches_device
  -> xfh_sim3_solve_device gated by the merge's count on the device, against the same steps through the restatements (ref_bow, ref_sim3solve);
  xfh_sim3_solve_device -> xfh_map_projection_search_device fed the solver's d_Tcw / d_Ow directly (the scene of tests/loop_rig.py), against the
  same search fed the rule's pose from the host: identical bytes."""
import numpy as np
import pytest

import bow_rig as BR
import guarded
import ref_loop as RL
import ref_sim3solve as R
import sim3solve_rig as G
from loop_rig import LoopRig
from projection_rig import GUARD, TUM1, cam_struct
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context

pytestmark = pytest.mark.gpu
F = np.float32


def geometry(rng, M, point1, matched, outlier_frac=0.2):
    """a point table in which the correspondences of (point1, matched) obey one similarity between the camera frames, some of them not"""
    T1w, T2w = G.pose(rng), G.pose(rng)
    Rm, t, s = G.rot(rng.randn(3), 6.0), rng.uniform(-0.2, 0.2, 3), 1.1
    points = rng.uniform(-40, 40, (M, 3))
    inv = lambda T, X: (X - T[:, 3]) @ T[:, :3]
    for i1 in np.nonzero((point1 >= 0) & (matched >= 0))[0]:
        X1 = np.array([rng.uniform(-2.5, 2.5), rng.uniform(-1.6, 1.6), rng.uniform(3, 9)])
        points[point1[i1]] = inv(T1w, X1)
        if rng.rand() >= outlier_frac:
            points[matched[i1]] = inv(T2w, (X1 - t) @ Rm / s + 2e-3 * rng.randn(3))
    return points.astype(F), T1w.ravel().astype(F), T2w.ravel().astype(F)


def test_bow_search_then_merge_then_solve_on_one_set_of_device_buffers(gpu_lib, oracle_mod):
    s = BR.Scene()
    J, n1, n2, M = 3, BR.N1, BR.N2, 1200
    want_bow = [s.want(oracle_mod, 0, j, keyframe=True) for j in range(J)]
    rng = np.random.RandomState(77)
    point2 = (400 + rng.randint(0, 700, (J, n2))).astype(np.int32)                          # a small pool: covisibles share map points
    for j in range(J):
        point2[j][s.s2[j]["has"] == 0] = -1
    point1 = rng.permutation(n1).astype(np.int32)
    point1[rng.rand(n1) < 0.1] = -1
    match12 = np.stack([w["match12"] for w in want_bow])
    matched, kf, num = R.merge(match12, point2, M)                                           # the restatements, step by step
    points, T1w, T2w = geometry(rng, M, point1, matched)
    table = R.iterations_table(G.PROB, 15, G.MAX_ITS, n1)
    draws = rng.randint(0, G.RAND_MAX + 1, (G.MAX_ITS, 3)).astype(np.int32)
    rule = R.rule(points, point1, matched, T1w, T2w, G.CAM, G.CAM2, table, draws, G.RAND_MAX, min_matches=20, num_matches=num)
    assert num >= 20 and rule["header"][1] == R.CONVERGED and len(set(kf.tolist())) >= 3 and rule["header"][0] > 30
    ctx = Context(nfeatures=1, max_height=32, max_width=32)
    bufs = []

    def dev(a):
        b = capi.DeviceBuffer(max(np.ascontiguousarray(a).nbytes, 16)).upload(a)
        bufs.append(b)
        return b
    try:
        s1, s2 = BR.BowRig.side([s.s1], "active"), BR.BowRig.side(s.s2, "has")
        lay_b = Context.bow_search_layout(J, n1, n2, GUARD)
        out_b = guarded.outputs(lay_b, keep=bufs)
        ws_b = dev(np.zeros(Context.bow_search_workspace_bytes(n1, n2, J), np.uint8))
        d1 = [dev(s1[k]).ptr for k in ("blob", "flag", "desc")]; d2 = [dev(s2[k]).ptr for k in ("blob", "flag", "desc")]
        lay_s = Context.sim3_solve_layout(1, n1, GUARD)
        out_s = guarded.outputs(lay_s, keep=bufs)
        ws_s = dev(np.zeros(gpu_lib.xfh_sim3_solve_workspace_bytes(n1, M, 1), np.uint8))
        lay_mid = Context.sim3_merge_layout(n1, GUARD)                                       # d_matched [n1], d_matched_kf [n1], the count
        mid = guarded.outputs(lay_mid, keep=bufs)
        d_matched, d_kf, d_num = (mid.ptr + lay_mid[k] for k in lay_mid.names)
        ins = [dev(a) for a in (points, point1, point2, T1w, T2w, table, draws)]
        ctx.bow_search_device(J, n1, n2, 1, *d1, s1["stride"], *d2, s2["stride"], ws_b.ptr, out_b.ptr, strict_low=True, guard=GUARD)
        ctx.sim3_merge_matches_device(J, n1, n2, M, out_b.ptr + lay_b["match12"], ins[2].ptr, ws_s.ptr, d_matched, d_kf, d_num)
        ctx.sim3_solve_device(1, n1, M, ins[0].ptr, ins[1].ptr, d_matched, ins[3].ptr, 0, ins[4].ptr, G.camera(G.CAM), G.camera(G.CAM2), ins[5].ptr, G.MAX_ITS, ins[6].ptr, 0,
                              G.RAND_MAX, ws_s.ptr, out_s.ptr, min_inliers=15, min_matches=20, d_num_matches=d_num, guard=GUARD)
        ctx.synchronize()                                                   # the only wait of the chain
        got_m12 = lay_b.parse(guarded.download(out_b, lay_b))["match12"]
        got_mid = lay_mid.parse(guarded.download(mid, lay_mid))
        got = lay_s.parse(guarded.download(out_s, lay_s))
    finally:
        for b in bufs:
            b.free()
        ctx.close()
    assert np.array_equal(got_m12, match12)
    assert np.array_equal(got_mid["matched"], matched) and np.array_equal(got_mid["matched_kf"], kf) and got_mid["num_matches"][0] == num
    G.assert_equals_rule(got, rule, 0)
    print("chain: BoW matches per covisible", [int((m >= 0).sum()) for m in match12], "numBoWMatches", num, dict(zip(R.HEADER, got["header"][0].tolist())))


@pytest.fixture(scope="module")
def lr(gpu_lib, weights_dense, oracle_mod):
    r = LoopRig(gpu_lib, weights_dense[1], 1000, 901, oracle_mod)
    yield r
    r.close()


def test_solve_then_map_projection_search_fed_the_device_pose(lr):
    """the candidate's pose is the loop scene's pose 0 and the similarity is small, so that the composed Scw looks at the scene's map points"""
    sc = G.scene(50, inlier_frac=0.9, deg=0.3, tmax=0.01, scale=1.02, T2w=lr.poses[0])
    rule = G.rule_of(sc)
    assert rule["header"][1] == R.CONVERGED
    nf, ctx, r = lr.nf, lr.ctx, lr.rig
    n1, M, th, form, accept = len(sc["point1"]), len(sc["points"]), 8.0, RL.FORM_SIM3, float(F(RL.TH_LOW) * F(1.5))
    want, raw_host, _ = lr.run_map(1, th, form, accept, poses=rule["Tcw"][None], Ow=rule["Ow"][None])       # the rule's pose from the host
    blk = lr.block(0)
    d = [lr.dev(np.ascontiguousarray(blk[k], t)) for k, t in (("xyz", F), ("normals", F), ("dist", F), ("qdesc", F), ("flags", np.uint8), ("taken", np.uint8))]
    ins = [lr.dev(np.ascontiguousarray(a)) for a in (sc["points"], sc["point1"], sc["matched"], sc["T1w"], sc["T2w"], sc["table"], sc["draws"][0])]
    lay_s = Context.sim3_solve_layout(1, n1, GUARD)
    out_s = guarded.outputs(lay_s, keep=lr.bufs)
    ws_s = lr.dev(np.zeros(capi.lib().xfh_sim3_solve_workspace_bytes(n1, M, 1), np.uint8))
    lay = Context.map_projection_search_layout(1, nf, nf, GUARD)
    out = guarded.outputs(lay, keep=lr.bufs)
    ws = lr.dev(np.zeros(Context.map_projection_search_workspace_bytes(nf, nf, 1), np.uint8))
    try:
        ctx.sim3_solve_device(1, n1, M, ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, 0, ins[4].ptr, G.camera(sc["cam1"]), G.camera(sc["cam2"]), ins[5].ptr,
                              len(sc["draws"][0]), ins[6].ptr, 0, G.RAND_MAX, ws_s.ptr, out_s.ptr, min_inliers=sc["min_inliers"], guard=GUARD)
        ctx.map_projection_search_device(form, 1, nf, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, out_s.ptr + lay_s["Tcw"], out_s.ptr + lay_s["Ow"], cam_struct(TUM1),
                                         lr.bounds, th, lr.sf, lr.rmax, r.fin[3].ptr, r.rec.ptr + ctx.desc_off, ctx.rec_bytes, 0, nf, ws.ptr, out.ptr, d_taken=d[5].ptr,
                                         accept_max=accept, guard=GUARD)
        ctx.synchronize()                                                   # nothing was read back between the two calls
        raw = guarded.download(out, lay)
        got = lay_s.parse(guarded.download(out_s, lay_s))
    finally:
        lr.free()
    G.assert_equals_rule(got, rule, 0)
    assert np.array_equal(raw, raw_host)
    print("solve -> projection search: matches", want[0]["n_matches"], "statuses", np.bincount(want[0]["status"], minlength=8).tolist())
    assert want[0]["n_matches"] > 0
