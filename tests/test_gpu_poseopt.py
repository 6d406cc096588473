"""xfh_pose_optimize_device (k_pose_optimize) against the kernel's rule of tests/ref_poseopt.py on the scenes of tests/poseopt_rig.py, whose condition
tests/test_poseopt_ref.py holds: flags and the eight header ints are EQUAL, the pose and the chi2 of the classifications within one float32 step (a
double-precision discrepancy far below half a float step can flip a rounding and no more); final_chi2 and the largest discrepancy are printed there,
not asserted.  That is SCENES and EDGE_SCENES (nt at the sizes where the kernel instance changes and at the maximum, edges on the first and last
keypoint and around every stride).  MONO_SCENES -- all-mono, ten or more edges, converging: what a monocular tracker has -- cannot hold that
condition; there the flags and header[0:4] are equal and pose, chi2 and final_chi2 lie within R.MONO_TOL, the spread of the float64 forms among
themselves (ref_poseopt.outputs_agree; the counts of iterations and trials are printed and only bounded).  Runs repeat byte for byte, a batch equals
its problems run alone -- also where the per-edge state is in the workspace, whatever the workspace held -- a null uright equals an all-negative one in
every instance, the host-pointer form and an in-place pose equal the device form, hostile input returns and leaves the guard bytes around the outputs
and the workspace alone.  What the rig cannot be given is a scene in which the stale-error rule shows (tests/test_poseopt_ref.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import poseopt_rig as R
import ref_poseopt as RP
from xfeatslam_amd import capi

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64


@pytest.fixture(scope="module")
def rig(gpu_lib):
    r = R.PoseRig(gpu_lib)
    yield r
    r.close()


def compare(res, m, tag):
    assert np.array_equal(res["header"], m["header"]), (tag, res["header"], m["header"])
    assert np.array_equal(res["outlier"], m["outlier"]), (tag, np.nonzero(res["outlier"] != m["outlier"])[0][:8])
    ut, uc = RP.ulps(res["Tcw_out"], m["Tcw_out"]), RP.ulps(res["chi2"], m["chi2"])
    rel = abs(res["final_chi2"] - m["final_chi2"]) / max(abs(m["final_chi2"]), 1e-300)
    print(f"{tag}: header {res['header'].tolist()}, final chi2 {res['final_chi2']:.17g} (rule {m['final_chi2']:.17g}, relative difference {rel:.1e}), "
          f"float steps off: pose {int(ut.max())}, chi2 {int(uc.max())}")
    assert ut.max() <= 1 and uc.max() <= 1, (tag, int(ut.max()), int(uc.max()))


@functools.lru_cache(maxsize=None)
def rule_of(name):
    """the rule's result for a scene of the rig, computed once for all tests (read, never changed)"""
    return R.model(R.scene(name))


def padded(m, nt):
    """the rule's result for the scene padded to nt keypoints (R.batch): keypoint k is lane k % 256's whatever nt is, and the padding adds nothing"""
    o, c = np.zeros(nt, np.uint8), np.zeros(nt, F)
    o[:len(m["outlier"])], c[:len(m["chi2"])] = m["outlier"], m["chi2"]
    return dict(m, outlier=o, chi2=c)


def agree(res, m, tag):
    """the trajectory-free comparison (all-mono scenes): prints both headers and the distances, -> ref_poseopt.outputs_agree's list"""
    ut, uc = RP.ulps(res["Tcw_out"], m["Tcw_out"]), RP.ulps(res["chi2"], m["chi2"])
    print(f"{tag}: header device {res['header'].tolist()}, rule {m['header'].tolist()}; float steps off: pose {int(ut.max())}, chi2 {int(uc.max())}; "
          f"final chi2 {res['final_chi2']:.17g} (rule {m['final_chi2']:.17g}, relative difference {RP.final_rel(res, m):.1e})")
    return RP.outputs_agree(res, m, R.MONO_TOL)


def same_bytes(a, b):
    return [k for k in ("Tcw_out", "outlier", "chi2", "header") if a[k].tobytes() != b[k].tobytes()] + (["final_chi2"] if a["final_chi2"] != b["final_chi2"] else [])


@pytest.mark.parametrize("name", list(R.SCENES))
def test_scene_against_the_rule(rig, name):
    s = R.scene(name)
    res, _ = rig.run([s])
    m = rule_of(name)
    compare(res[0], m, name)
    if m["header"][0] < 3:                                                # refused: the input pose, bit for bit, and no flag
        assert res[0]["Tcw_out"].tobytes() == s["Tcw"].tobytes() and not res[0]["outlier"].any() and not res[0]["chi2"].any() and res[0]["header"][2] == 0


@pytest.mark.parametrize("name", list(R.EDGE_SCENES))
def test_edge_sizes_against_the_rule(rig, name):
    """nt = 1024, 1025, 4096, 4097 and 16384 with edges at the first and last keypoint, around the strides of 256 and around the sizes at which the
    instance changes; conditioned scenes, so the comparison is the exact one"""
    res, _ = rig.run([R.scene(name)])
    compare(res[0], rule_of(name), name)


@pytest.mark.parametrize("name", list(R.MONO_SCENES))
def test_mono_scenes_agree_with_the_rule(rig, name):
    """all-mono scenes of ten or more edges: flags and header[0:4] equal, pose, chi2 and final_chi2 within R.MONO_TOL (the spread of the float64 forms
    among themselves); the number of trials is not compared"""
    res, _ = rig.run([R.scene(name)])
    assert agree(res[0], rule_of(name), name) == []


def test_runs_repeat_and_in_place_pose(rig):
    for name in ("n257", "e4097", "m700_null_out"):
        s = R.scene(name)
        a, raw_a = rig.run([s], fill=0x00)
        b, raw_b = rig.run([s], fill=0xFF)
        assert raw_a.tobytes() == raw_b.tobytes(), name
        c, _ = rig.run([s], in_place=True)                                # d_Tcw_out == d_Tcw
        assert same_bytes(a[0], c[0]) == [], name


def test_batch_of_three_equals_three_calls(rig):
    sc = R.batch(R.BATCH3)
    res, _ = rig.run(sc)
    for p, s in enumerate(sc):
        one, _ = rig.run([s])
        for k in ("Tcw_out", "outlier", "chi2", "header"):
            assert res[p][k].tobytes() == one[0][k].tobytes(), (p, k)
        assert res[p]["final_chi2"] == one[0]["final_chi2"]
        compare(res[p], R.model(s), f"B=3 problem {p}")
    assert [int(r["header"][0]) for r in res] == [64, 2, 257]
    assert res[1]["Tcw_out"].tobytes() == sc[1]["Tcw"].tobytes() and not res[1]["outlier"].any() and res[1]["header"].tolist() == [2, 0, 0, 0, 0, 0, 0, 0]


def test_null_uright_is_all_mono(rig):
    """a null uright and an all-negative array give the same bytes, in each of the three instances (nt <= 1024, <= 4096, above)"""
    for name in ("n9_mono", "m200_null_out", "m300_null", "m700_null_out", "m400_null_max"):
        s = R.scene(name)
        assert s["uright"] is None
        a, raw_a = rig.run([s])
        t = dict(s, uright=np.full(s["nt"], -1.0, F))
        b, raw_b = rig.run([t])
        assert same_bytes(a[0], b[0]) == [] and raw_a.tobytes() == raw_b.tobytes(), name


def test_workspace_instance_in_a_batch(rig):
    """B = 3 at nt = 5000, where the per-edge state lives in the caller's workspace, one stride per problem: a conditioned mixed scene, an all-mono
    one and a refused one.  Each problem equals its run alone byte for byte and the rule; what the workspace held before does not matter;
    PoseRig.run checks the bytes around the workspace.  Problem p leaves in the p-th stride of the workspace exactly what it leaves there alone:
    workgroups on different XCDs do not see each other's stores while the kernel runs, so problems that shared workspace could still give the
    right outputs; the bytes left behind show where each one wrote.  Then B = 2 with a null uright at nt = 4096, where the workspace is not
    touched (include/xfeat_hip.h)."""
    sc = R.batch(R.WS_BATCH3)
    assert sc[0]["nt"] == 5000 and len(sc) == 3
    res, raw0 = rig.run(sc, ws_fill=0x00)
    left = rig.workspace
    stride = int(rig.L.xfh_pose_optimize_workspace_bytes(5000, 1))
    assert len(left) == 3 * stride
    res_ff, raw1 = rig.run(sc, ws_fill=0xFF)
    assert raw0.tobytes() == raw1.tobytes()
    for p, (s, name) in enumerate(zip(sc, R.WS_BATCH3)):
        one, _ = rig.run([s], ws_fill=0x00)
        assert same_bytes(res[p], one[0]) == [], (p, same_bytes(res[p], one[0]))
        assert rig.workspace.tobytes() == left[p * stride:(p + 1) * stride].tobytes(), f"problem {p} ({name}) left other bytes in its stride of the workspace than alone"
    assert left[:stride].any() and left[stride:2 * stride].any()          # (the state words of the edges: the instance does use it)
    assert R.WS_BATCH3 == ("big", "m700_null_out", "n2")
    compare(res[0], padded(rule_of("big"), 5000), "B=3, nt=5000, problem 0 (big)")
    assert agree(res[1], padded(rule_of("m700_null_out"), 5000), "B=3, nt=5000, problem 1 (m700_null_out)") == []
    assert res[2]["header"].tolist() == [2, 0, 0, 0, 0, 0, 0, 0] and res[2]["Tcw_out"].tobytes() == sc[2]["Tcw"].tobytes() and not res[2]["outlier"].any() and not res[2]["chi2"].any()
    sc = R.batch(R.NULL_BATCH2, null_uright=True)
    assert sc[0]["nt"] == 4096 and all(s["uright"] is None for s in sc)
    res, _ = rig.run(sc, ws_fill=0x3C)
    assert np.all(rig.workspace == 0x3C)
    for p, (s, name) in enumerate(zip(sc, R.NULL_BATCH2)):
        one, _ = rig.run([s])
        assert same_bytes(res[p], one[0]) == [], (p, same_bytes(res[p], one[0]))
        assert agree(res[p], padded(rule_of(name), 4096), f"B=2, nt=4096, null uright, problem {p} ({name})") == []


def test_host_pointer_form_equals_the_device_form(rig):
    L = rig.L
    for name in ("n65_mixed", "n9_mono", "n2", "e4097", "m700_null_out"):  # the last two: nt > 4096, the workspace is the call's own
        s = R.scene(name)
        dev, _ = rig.run([s])
        nt = s["nt"]
        To, ol, ch, hd, fc = np.zeros(12, F), np.zeros(nt, np.uint8), np.zeros(nt, F), np.zeros(8, np.int32), np.zeros(1, D)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = L.xfh_pose_optimize(rig.ctx.h, nt, s["nq"], p(s["Tcw"]), C.byref(rig.cam), p(s["xy_un"]), p(s["uright"]) if s["uright"] is not None else None,
                                 p(s["assigned"]), p(s["points"]), R.INV_SIGMA2, p(To), p(ol), p(ch), p(hd), p(fc))
        assert rc == 0
        for k, v in (("Tcw_out", To), ("outlier", ol), ("chi2", ch), ("header", hd)):
            assert dev[0][k].tobytes() == v.tobytes(), (name, k)
        assert dev[0]["final_chi2"] == fc[0]


def test_hostile_values_return_and_stay_inside_the_outputs(rig):
    """NaN / Inf in the points, the pose and the observations, a point in the camera plane: the call returns (every loop is bounded), the header
    stays within its bounds and nothing outside the five output arrays is written (PoseRig.run checks the bytes around them)"""
    base = R.scene("n257")
    nan, inf = F(np.nan), F(np.inf)
    cases = []
    s = dict(base, points=base["points"].copy()); s["points"][::7] = nan; s["points"][3::11, 2] = inf; cases.append(("points", s))
    s = dict(base, Tcw=base["Tcw"].copy()); s["Tcw"][5] = nan; cases.append(("pose nan", s))
    s = dict(base, Tcw=base["Tcw"].copy()); s["Tcw"][3] = inf; cases.append(("pose inf", s))
    s = dict(base, Tcw=np.zeros(12, F)); cases.append(("pose zero", s))
    s = dict(base, xy_un=base["xy_un"].copy(), uright=base["uright"].copy()); s["xy_un"][::5] = nan; s["uright"][::3] = nan; s["xy_un"][1::9] = -inf; cases.append(("observations", s))
    for tag, s in cases:
        res, _ = rig.run([s, base])
        h = res[0]["header"]
        print(tag, h.tolist(), res[0]["final_chi2"])
        assert h[0] == 257 and 0 <= h[1] <= 257 and h[2] == h[0] - h[1] and 1 <= h[3] <= 4 and 0 <= h[4] <= 40 and h[4] <= h[5] <= 400 and 0 <= h[6] <= h[5] and 0 <= h[7] <= h[5]
        assert set(np.unique(res[0]["outlier"])) <= {0, 1}
        one, _ = rig.run([base])                                          # the neighbour in the batch is untouched by it
        assert all(res[1][k].tobytes() == one[0][k].tobytes() for k in ("Tcw_out", "outlier", "chi2", "header"))


def test_refusals_launch_nothing(rig):
    L, ctx = rig.L, rig.ctx.h
    b = capi.DeviceBuffer(4096)
    p = b.ptr
    cam = C.byref(rig.cam)
    ok = lambda **kw: L.xfh_pose_optimize_device(ctx, kw.get("B", 1), kw.get("nt", 8), kw.get("nq", 8), kw.get("T", p), cam, p, None, p, p, kw.get("w", 1.0),
                                                 kw.get("ws", p), p, p, p, p, kw.get("fc", p))
    for kw in (dict(B=0), dict(nt=0), dict(nq=capi.GRID_MAX_N + 1), dict(T=None), dict(T=p + 2), dict(ws=p + 8), dict(fc=p + 4), dict(w=0.0), dict(w=float("nan"))):
        assert ok(**kw) == 1, kw
    rig.ctx.synchronize()
    b.free()
