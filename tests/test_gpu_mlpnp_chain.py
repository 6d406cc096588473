"""The MLPnP solver inside the relocalisation chain of Tracking::Relocalization (src/Tracking.cc:3678-3773), every step on ONE set of device buffers
and one stream with no host step between the calls:
  xfh_bow_search_device (shared = 2, three candidate keyframes against the current frame, the scene of tests/bow_rig.py) -> xfh_mlpnp_solve_device fed
  the search's d_assigned2 and d_n_matches directly -> xfh_pose_optimize_device fed the solver's d_Tcw and d_assigned_out directly,
against the same three calls run separately through host copies (identical bytes) and against the restatements chained (ref_bow, ref_mlpnp,
ref_poseopt).  One candidate refines, one finds nothing (NONE) and one is below the BoW match count (TOO_FEW): the last two reach the optimiser with
every match -1 and are refused there (it returns 0 without touching the pose)."""
import numpy as np
import pytest

import bow_rig as BR
import guarded
import mlpnp_rig as G
import poseopt_rig as PR
import ref_mlpnp as R
import ref_poseopt as RPO
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context

pytestmark = pytest.mark.gpu
F = np.float32
GUARD = 256
CAM5 = tuple(G.CAM) + (F(0.0),)                                              # the optimiser's rule takes (fx, fy, cx, cy, bf); every edge is mono


def geometry(rng, xy, assigned2, nq, outlier_frac):
    """a point block in which the matches of assigned2 (frame keypoint -> point) obey one camera pose, some of them not"""
    Rm, t = G.rot(rng.randn(3), 25.0), rng.uniform(-1, 1, 3)
    pts = rng.uniform(-30, 30, (nq, 3))
    for k in np.nonzero(assigned2 >= 0)[0]:
        if rng.rand() < outlier_frac:
            continue
        px = xy[k] + 0.4 * rng.randn(2)
        Xc = rng.uniform(3, 9) * np.array([(px[0] - float(G.CAM[2])) / float(G.CAM[0]), (px[1] - float(G.CAM[3])) / float(G.CAM[1]), 1.0])
        pts[assigned2[k]] = (Xc - t) @ Rm
    return pts.astype(F)


def test_bow_search_then_mlpnp_then_pose_optimisation_on_one_stream(gpu_lib, oracle_mod):
    s = BR.Scene()
    B, n1, n2 = 3, BR.N1, BR.N2                                             # n1: keypoints (= map points) of a candidate, n2: keypoints of the frame
    want_bow = [s.want(oracle_mod, p, 0, keyframe=False, nn_ratio=0.75) for p in range(B)]
    nm = [int(w["n_matches"]) for w in want_bow]
    assert nm[2] < nm[1] and nm[2] < nm[0] and nm[2] >= 15
    min_matches = nm[2] + 1                                                 # candidate 2 is below the count
    rng = np.random.RandomState(91)
    xy = np.stack([rng.uniform(20, 732, n2), rng.uniform(20, 460, n2)], 1).astype(F)
    points = np.stack([geometry(rng, xy, want_bow[b]["assigned2"], n1, (0.2, 1.0, 0.2)[b]) for b in range(B)])
    tables = R.iterations_table(n2)
    max_iters = 40
    draws = rng.randint(0, G.RAND_MAX + 1, (max_iters, 6)).astype(np.int32)
    rules = [R.rule(xy, want_bow[b]["assigned2"], points[b], G.CAM, tables, draws, G.RAND_MAX, max_err=G.MAX_ERR, n_matches=nm[b], min_matches=min_matches) for b in range(B)]
    assert [r["header"][1] for r in rules] == [R.REFINED, R.NONE, R.TOO_FEW] and rules[0]["header"][0] > 100
    ctx = Context(nfeatures=1, max_height=32, max_width=32)
    cam = G.camera()
    bufs = []

    def dev(a):
        b = capi.DeviceBuffer(max(np.ascontiguousarray(a).nbytes, 16)).upload(a)
        bufs.append(b)
        return b
    try:
        s1, s2 = BR.BowRig.side(s.blocks, "active"), BR.BowRig.side([s.s2[0]], None)
        lay_b = Context.bow_search_layout(B, n1, n2, GUARD)
        ws_b = dev(np.zeros(Context.bow_search_workspace_bytes(n1, n2, B), np.uint8))
        d1 = [dev(s1[k]).ptr for k in ("blob", "flag", "desc")]; d2 = [dev(s2["blob"]).ptr, None, dev(s2["desc"]).ptr]
        lay_m, lay_p = Context.mlpnp_layout(B, n2, GUARD), Context.pose_optimize_layout(B, n2, GUARD)
        ws_m = dev(np.zeros(gpu_lib.xfh_mlpnp_workspace_bytes(n2, n1, B, max_iters), np.uint8))
        ins = [dev(a) for a in (xy, points, tables[0], tables[1], draws, np.tile(xy, (B, 1, 1)))]      # the optimiser takes d_xy_un [B][nt][2]: the frame's keypoints per candidate
        ws_p = dev(np.zeros(Context.pose_optimize_workspace_bytes(n2, B), np.uint8))

        def chain(host_copies):
            """the three calls; host_copies: every intermediate goes through the host and comes back in a fresh buffer"""
            out_b, out_m, out_p = (guarded.outputs(lay, keep=bufs) for lay in (lay_b, lay_m, lay_p))
            ctx.bow_search_device(B, n1, n2, 2, *d1, s1["stride"], *d2, s2["stride"], ws_b.ptr, out_b.ptr, nn_ratio=0.75, guard=GUARD)
            d_assigned, d_nm = out_b.ptr + lay_b["assigned2"], out_b.ptr + lay_b["n_matches"]
            if host_copies:
                ctx.synchronize()
                a = lay_b.parse(out_b.download(np.uint8, lay_b["bytes"]))
                d_assigned, d_nm = dev(a["assigned2"]).ptr, dev(a["n_matches"]).ptr
            ctx.mlpnp_solve_device(B, n2, n1, ins[0].ptr, d_assigned, ins[1].ptr, None, cam, G.MAX_ERR, ins[2].ptr, ins[3].ptr, 5, None, max_iters, ins[4].ptr, 0,
                                   G.RAND_MAX, ws_m.ptr, out_m.ptr, min_matches=min_matches, d_n_matches=d_nm, guard=GUARD)
            d_T, d_a = out_m.ptr + lay_m["Tcw"], out_m.ptr + lay_m["assigned_out"]
            if host_copies:
                ctx.synchronize()
                a = lay_m.parse(out_m.download(np.uint8, lay_m["bytes"]))
                d_T, d_a = dev(a["Tcw"]).ptr, dev(a["assigned_out"]).ptr
            ctx.pose_optimize_device(B, n2, n1, d_T, cam, ins[5].ptr, None, d_a, ins[1].ptr, ws_p.ptr, *[out_p.ptr + lay_p[k] for k in lay_p.names], inv_sigma2=1.0)
            ctx.synchronize()                                               # the only wait of the device chain
            return guarded.download(out_b, lay_b), guarded.download(out_m, lay_m), guarded.download(out_p, lay_p)
        raw_b, raw_m, raw_p = chain(False)
        sep_b, sep_m, sep_p = chain(True)
    finally:
        for b in bufs:
            b.free()
        ctx.close()
    assert np.array_equal(raw_b, sep_b) and np.array_equal(raw_m, sep_m) and np.array_equal(raw_p, sep_p)
    got_b = lay_b.parse(raw_b)
    for b in range(B):
        assert np.array_equal(got_b["assigned2"][b], want_bow[b]["assigned2"]) and got_b["n_matches"][b] == nm[b]
    got = lay_m.parse(raw_m)
    for b in range(B):
        G.assert_equals_rule(got, rules[b], b, prior_byte=guarded.FILL)
    got_p = lay_p.parse(raw_p)
    Tout, hdr = got_p["Tcw_out"], got_p["header"]
    m = RPO.rule(got["Tcw"][0], CAM5, xy, None, got["assigned_out"][0], points[0], 1.0)     # the optimiser's rule on the solver's outputs (within a step of its rule's)
    assert RPO.outputs_agree(guarded.problems(got_p, B)[0], m, PR.MONO_TOL) == [] and hdr[0, 2] > 50
    for b in (1, 2):                                                        # no pose, every match -1: refused (fewer than three edges)
        assert np.all(got["assigned_out"][b] == -1) and hdr[b, 0] == 0 and hdr[b, 2] == 0, (b, hdr[b])
        m = RPO.rule(got["Tcw"][b], CAM5, xy, None, got["assigned_out"][b], points[b], 1.0)
        assert np.array_equal(hdr[b][:4], m["header"][:4]) and Tout[b].tobytes() == np.asarray(m["Tcw_out"], F).tobytes()
    print("chain: BoW matches", nm, "MLPnP", [dict(zip(R.HEADER, got["header"][b].tolist())) for b in range(B)], "PoseOptimization returns", hdr[:, 2].tolist())
