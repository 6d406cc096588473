"""LocalBundleAdjustment -> PoseOptimization on ONE point table in device memory: xfh_local_ba_device with write_back refines the table in place, then
xfh_pose_optimize_device tracks a frame against that very table (nq = its rows, assigned[k] = a row), with nothing copied between the two calls.
Against the chain of the two Python rules (tests/ref_local_ba.py, tests/ref_poseopt.py): the optimiser's flags and header[0:4] equal, its pose and chi2
within the pose optimiser's trajectory-free tolerance (poseopt_rig.MONO_TOL; final_chi2 is printed: with stereo edges it carries the float invz).  The condition is checked here on the CPU, with the Python rules alone: the optimiser's decisions do
not change when the refined points move by LBA_TOL in any direction tried (all up, all down, random signs)."""
import ctypes as C

import numpy as np
import pytest

import guarded
import local_ba_rig as G
import poseopt_rig as PG
import ref_poseopt as RP
from xfeatslam_amd import capi, local_ba

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64


def frame_of(p, k0):
    """the observations of keyframe k0 as a frame to track: xy_un, uright, assigned = the ROW of the point in the table"""
    e = np.nonzero(p["edge_kf"] == k0)[0]
    pt = np.repeat(np.arange(len(p["point_row"])), np.diff(p["edge_begin"]))[e]
    return p["edge_obs"][e, :2].copy(), p["edge_obs"][e, 2].copy(), p["point_row"][pt].astype(np.int32)


@pytest.mark.parametrize("name,k0", [("eleven_mixed", 3), ("outliers", 2)])
def test_local_ba_then_pose_optimization(name, k0):
    p = G.scene(name)
    lba = G.rule_of(name)
    xy, ur, assigned = frame_of(p, k0)
    assert len(assigned) >= 10
    Tcw0 = np.asarray(p["pose_table"], F)[p["kf_row"][k0]]                  # the frame starts from the keyframe's pose BEFORE the adjustment
    table = np.asarray(p["point_table"], F).copy()
    seen = np.diff(p["edge_begin"]) > 0
    table[p["point_row"][seen]] = lba["points_out"][seen]
    want = RP.rule(Tcw0, G.CAM, xy, ur, assigned, table, 1.0)
    # ---- the condition: the optimiser does not see points that moved by LBA_TOL
    rng = np.random.RandomState(4)
    step = np.spacing(F(max(float(np.max(np.abs(lba["points_out"]))), 1.0))) * G.LBA_TOL.points
    for sign in (np.ones(table.shape), -np.ones(table.shape), rng.choice([-1.0, 1.0], table.shape)):
        alt = RP.rule(Tcw0, G.CAM, xy, ur, assigned, (table.astype(D) + sign * step).astype(F), 1.0)
        assert np.array_equal(alt["outlier"], want["outlier"]) and np.array_equal(alt["header"][:4], want["header"][:4]), "the optimiser is sensitive to LBA_TOL in this scene"
    # ---- the chain on the device
    rig = G.LbaRig(capi.lib())
    try:
        L, ctx = rig.L, rig.ctx
        nK, nP, nE = G.dims(p)
        arrays = [np.ascontiguousarray(np.asarray(p[k], dt)) for k, dt in G.INPUTS]
        tables = [guarded.Guarded(a.nbytes, G.GUARD, inner=a, what=k) for a, k in zip(arrays[:2], ("the pose table", "the point table"))]
        dev = [capi.DeviceBuffer(a.nbytes).upload(a) for a in arrays[2:]]
        lay = local_ba.local_ba_layout(nK, nP, nE, G.GUARD)
        out = guarded.outputs(lay)
        ws = guarded.Guarded(local_ba.workspace_bytes(nK, nP, nE, G.n_free_of(p)), G.GUARD, inner=0x3C)
        cam = G.cam_struct()
        local_ba.local_ba_device(ctx, nK, G.n_free_of(p), nP, nE, tables[0].ptr, len(arrays[0]), tables[1].ptr, len(arrays[1]), *[d.ptr for d in dev], cam, ws.ptr, out.ptr, lay,
                                 write_back=True)
        nt, nq = len(assigned), len(table)
        play = ctx.pose_optimize_layout(1, nt, G.GUARD)
        pout = guarded.outputs(play)
        pin = [capi.DeviceBuffer(a.nbytes).upload(a) for a in (Tcw0.copy(), np.ascontiguousarray(xy, F), np.ascontiguousarray(ur, F), assigned)]
        pws = guarded.Guarded(max(ctx.pose_optimize_workspace_bytes(nt, 1), 16), G.GUARD, inner=0x3C)
        ctx.pose_optimize_device(1, nt, nq, pin[0].ptr, cam, pin[1].ptr, pin[2].ptr, pin[3].ptr, tables[1].ptr, pws.ptr, *[pout.ptr + play[k] for k in play.names])
        ctx.synchronize()
        got_lba = lay.parse(guarded.download(out, lay))
        got_lba["final_chi2"] = float(got_lba["final_chi2"][0])
        got = guarded.problems(play.parse(guarded.download(pout, play)), 1)[0]
        ws.download(), pws.download(), tables[0].download()
        dev_table = tables[1].download().view(F).reshape(-1, 3)
        for d in dev + pin + [out, pout, ws.buf, pws.buf, tables[0].buf, tables[1].buf]:
            d.free()
    finally:
        rig.close()
    assert G.outputs_agree(got_lba, lba) == []
    moved = np.abs(dev_table.astype(D) - table.astype(D)).max() / step * G.LBA_TOL.points
    assert moved <= G.LBA_TOL.points, moved
    # the optimiser against its rule ON THE TABLE THE DEVICE LEFT (the two tables may differ by LBA_TOL), and that rule's decisions against the chain's
    want_dev = want if np.array_equal(dev_table.view(np.uint32), table.view(np.uint32)) else RP.rule(Tcw0, G.CAM, xy, ur, assigned, dev_table, 1.0)
    assert np.array_equal(want_dev["outlier"], want["outlier"]) and np.array_equal(want_dev["header"][:4], want["header"][:4])
    assert np.array_equal(got["outlier"], want_dev["outlier"]) and np.array_equal(got["header"][:4], want_dev["header"][:4]), (got["header"], want_dev["header"])
    ut, uc = RP.ulps(got["Tcw_out"], want_dev["Tcw_out"]), RP.ulps(got["chi2"], want_dev["chi2"])
    print(f"{name}: PoseOptimization float steps off: pose {int(ut.max())}, chi2 {int(uc.max())}; final chi2 {got['final_chi2']:.17g} (rule {want_dev['final_chi2']:.17g})")
    assert ut.max() <= PG.MONO_TOL.pose and uc.max() <= PG.MONO_TOL.chi2 and RP.header_in_bounds(got["header"])
    print(f"{name}: LBA erased {got_lba['header'][9]} of {nE} edges -> PoseOptimization keeps {int(got['header'][2])} of {int(got['header'][0])} edges")
