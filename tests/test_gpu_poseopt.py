"""xfh_pose_optimize_device (k_pose_optimize) against the kernel's rule of tests/ref_poseopt.py on the scenes of tests/poseopt_rig.py, whose condition
tests/test_poseopt_ref.py holds: flags and the eight header ints are EQUAL, the pose and the chi2 of the classifications within one float32 step (a
double-precision discrepancy far below half a float step can flip a rounding and no more).  Runs repeat byte for byte, a batch equals its
problems run alone, the host-pointer form equals the device form, hostile input returns and leaves the guard bytes alone.  final_chi2 and the
largest discrepancy are printed, not asserted."""
import ctypes as C

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


@pytest.mark.parametrize("name", list(R.SCENES))
def test_scene_against_the_rule(rig, name):
    s = R.scene(name)
    res, _ = rig.run([s])
    m = R.model(s)
    compare(res[0], m, name)
    if m["header"][0] < 3:                                                # refused: the input pose, bit for bit, and no flag
        assert res[0]["Tcw_out"].tobytes() == s["Tcw"].tobytes() and not res[0]["outlier"].any() and not res[0]["chi2"].any() and res[0]["header"][2] == 0


def test_runs_repeat_and_in_place_pose(rig):
    s = R.scene("n257")
    a, raw_a = rig.run([s], fill=0x00)
    b, raw_b = rig.run([s], fill=0xFF)
    assert raw_a.tobytes() == raw_b.tobytes()
    c, _ = rig.run([s], in_place=True)                                    # d_Tcw_out == d_Tcw
    assert all(np.array_equal(a[0][k], c[0][k]) for k in ("Tcw_out", "outlier", "chi2", "header")) and a[0]["final_chi2"] == c[0]["final_chi2"]


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
    s = R.scene("n9_mono")
    a, _ = rig.run([s])
    t = dict(s, uright=np.full(s["nt"], -1.0, F))
    b, _ = rig.run([t])
    assert all(a[0][k].tobytes() == b[0][k].tobytes() for k in ("Tcw_out", "outlier", "chi2", "header"))


def test_host_pointer_form_equals_the_device_form(rig):
    L = rig.L
    for name in ("n65_mixed", "n9_mono", "n2"):
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
