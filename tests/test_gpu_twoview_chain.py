"""Monocular initialisation on the device with no host step between the calls, ONE synchronisation at the end of each chain:
  search -> reconstruct: xfh_init_search_device writes matches12, xfh_two_view_device reads it with the two frames' undistorted keypoints where
      xfh_frame_finish left them (the scene of tests/init_rig.py: an image and its shifted, slightly warped copy);
  reconstruct -> optimise: xfh_two_view_device writes T21 and p3d, xfh_pose_optimize_device takes them as the initial pose of the current frame and
      as the world points (indexed by idx1, which is what matches21 holds), on the general scene of tests/twoview_rig.py, which succeeds.
Each stage is compared with its restatement evaluated on what the device handed it."""
import ctypes as C

import numpy as np
import pytest

import guarded
import ref_twoview as R
import twoview_rig as G
from init_rig import InitRig
from projection_rig import TUM1, cam_struct
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context

pytestmark = pytest.mark.gpu
F = np.float32
NF, SEED, WINDOW, ITERS = 1000, 1200, 100.0, 32


def test_init_search_then_two_view_on_the_device(gpu_lib, weights_dense, oracle_mod):
    rig = InitRig(gpu_lib, weights_dense[1], NF, SEED, oracle_mod)
    ctx, L, nf = rig.ctx, rig.L, rig.nf
    bufs = []
    try:
        cam = cam_struct(TUM1)
        lay, tlay = Context.init_search_layout(1, nf, nf, 256), Context.two_view_layout(1, nf, 256)
        dev = lambda a: bufs.append(capi.DeviceBuffer(max(np.ascontiguousarray(a).nbytes, 16)).upload(a)) or bufs[-1]
        q, pm = rig.block(0)
        dq, dpm = dev(np.ascontiguousarray(q, F)), dev(np.ascontiguousarray(pm, F))
        draws = G.draws_of(77, ITERS)
        dd = dev(draws)
        out, ws = guarded.outputs(lay, keep=bufs), dev(np.zeros(Context.init_search_workspace_bytes(nf, nf, 1), np.uint8))
        tout, tws = guarded.outputs(tlay, keep=bufs), dev(np.zeros(L.xfh_two_view_workspace_bytes(nf, nf, ITERS, 1), np.uint8))
        ctx.init_search_device(1, nf, dq.ptr, dpm.ptr, rig.dgrid, rig.dtg.ptr, 0, nf, ws.ptr, out.ptr, window=WINDOW, guard=256)
        ctx.two_view_device(1, nf, nf, cam, rig.fin[0].ptr, rig.dxy, out.ptr + lay["matches12"], dd.ptr, 0, ITERS, G.RAND_MAX, tws.ptr, tout.ptr, guard=256)
        ctx.synchronize()                                                   # the only one
        m12 = lay.parse(guarded.download(out, lay, skip=("prev_out",)))["matches12"][0]         # (no d_target_xy: prev_out is not written)
        got = tlay.parse(guarded.download(tout, tlay))
        want = R.rule(rig.xy[0], rig.xy[1], m12, [F(TUM1[k]) for k in ("fx", "fy", "cx", "cy")], draws, G.RAND_MAX)
        print("chain: matches", int((m12 >= 0).sum()), "->", R.STATUS_NAMES[want["header"][1]], dict(zip(R.HEADER, want["header"].tolist())))
        assert (m12 >= 0).sum() >= 100 and want["header"][0] == (m12 >= 0).sum()
        G.assert_equals_rule(got, want, 0)
    finally:
        for b in bufs:
            b.free()
        rig.close()


def test_two_view_then_pose_optimize_on_the_device(gpu_lib):
    s = G.rig()["general"]
    n1, n2, iters = len(s["xy1"]), len(s["xy2"]), len(s["draws"])
    m21 = np.full(n2, -1, np.int32)
    m21[s["m12"][s["m12"] >= 0]] = np.nonzero(s["m12"] >= 0)[0]              # known before the chain starts, like SearchForInitialization's vnMatches21
    ctx = Context(nfeatures=1, max_height=32, max_width=32)
    L = gpu_lib
    bufs = []
    try:
        dev = lambda a: bufs.append(capi.DeviceBuffer(max(np.ascontiguousarray(a).nbytes, 16)).upload(a)) or bufs[-1]
        tlay = Context.two_view_layout(1, n1, 256)
        dx1, dx2, dm, dd, dm21 = dev(s["xy1"]), dev(s["xy2"]), dev(s["m12"]), dev(s["draws"]), dev(m21)
        tout, tws = guarded.outputs(tlay, keep=bufs), dev(np.zeros(L.xfh_two_view_workspace_bytes(n1, n2, iters, 1), np.uint8))
        play = Context.pose_optimize_layout(1, n2, 256)
        po, pws = guarded.outputs(play, keep=bufs), dev(np.zeros(int(L.xfh_pose_optimize_workspace_bytes(n2, 1)), np.uint8))
        cam = G.camera()
        ctx.two_view_device(1, n1, n2, cam, dx1.ptr, dx2.ptr, dm.ptr, dd.ptr, 0, iters, G.RAND_MAX, tws.ptr, tout.ptr, guard=256)
        rc = L.xfh_pose_optimize_device(ctx.h, 1, n2, n1, tout.ptr + tlay["floats"] + 4 * R.F_T21, C.byref(cam), dx2.ptr, None, dm21.ptr, tout.ptr + tlay["p3d"], 1.0,
                                        pws.ptr, *[po.ptr + play[k] for k in play.names])
        assert rc == 0
        ctx.synchronize()                                                   # the only one
        got = tlay.parse(guarded.download(tout, tlay))
        pose = guarded.problems(play.parse(guarded.download(po, play)), 1)[0]
        want = G.rule_of(s)
        G.assert_equals_rule(got, want, 0)
        assert got["header"][0, 1] == R.OK_F
        T0, T1 = got["floats"][0, R.F_T21:R.F_T21 + 12].reshape(3, 4), pose["Tcw_out"].reshape(3, 4)
        hdr, outlier = pose["header"], pose["outlier"]
        tri2 = s["m12"][np.nonzero(got["tri"][0])[0]]                        # the current frame's keypoints whose points were triangulated
        print("pose optimisation on T21 and p3d:", dict(zip(Context.POSE_HEADER, hdr.tolist())), "triangulated", len(tri2), "of them outliers", int(outlier[tri2].sum()))
        # every triangulated point reprojects within 2 px into both frames under T21 (CheckRT), so the optimisation starts at a pose that fits them:
        # it keeps nearly all of them (chi2 < 5.991 is the tighter gate: 2.45 px) and moves the pose by little
        assert hdr[0] == (m21 >= 0).sum() and hdr[2] >= 0.9 * len(tri2) and outlier[tri2].sum() <= 0.1 * len(tri2)
        ang = np.degrees(np.arccos(np.clip((np.trace(T1[:, :3].astype(np.float64) @ T0[:, :3].astype(np.float64).T) - 1) / 2, -1, 1)))
        assert ang < 0.5 and np.linalg.norm(T1[:, 3] - T0[:, 3]) < 0.1, (ang, T0, T1)
    finally:
        for b in bufs:
            b.free()
        ctx.close()
