"""xfh_sim3_optimize_device on the GPU against the Python rule (tests/ref_optsim3.py) on the rig's scenes (tests/optsim3_rig.py).

The comparison rules.  EQUAL: the pair status, d_assigned_out and header[0:8] (the counts, n_more, the return value, the classifications run).
Within SIM3OPT_TOL -- the spread of the float64 forms among themselves, measured on the CPU with nothing from the device in it: S12_out, the state,
Tcw, Ow, chi2 and final_chi2.  Iterations, trials, rejections and factorisation failures are printed and held against their static bounds only:
the Jacobian is a central difference over 2e-9, so once a problem has converged rho is rounding noise over 1e-3 and the number of trials is
chance.  Nothing here asserts that the device took the rule's trajectory."""
import ctypes as C

import numpy as np
import pytest

import optsim3_rig as G
import ref_optsim3 as R
from xfeatslam_amd import capi

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64
INVALID = 1


@pytest.fixture(scope="module")
def rig():
    r = G.Sim3OptRig(capi.lib())
    yield r
    r.close()


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = R.rule(G.scene(name))
        return cache[name]
    return get


def check(got, ref, tag):
    h = np.asarray(got["header"])
    print(f"{tag}: device {dict(zip(R.H_KEYS, h[:12].tolist()))}  rule trajectory {np.asarray(ref['header'])[8:12].tolist()}  distances {R.distances(got, ref, G.TH2)}")
    bad = R.outputs_agree(got, ref, G.SIM3OPT_TOL)
    assert bad == [], (tag, bad)


@pytest.mark.parametrize("name", list(G.SCENES))
def test_scene_against_the_rule(rig, models, name):
    (got,), _ = rig.run([G.scene(name)])
    check(got, models(name), name)


def test_runs_repeat_byte_for_byte(rig):
    for names in (("out100",), ("e1025",), G.BATCH3):
        ps = G.batch([G.scene(n) for n in names])
        a, b = rig.run(ps)[1], rig.run(ps, fill=0x5A, ws_fill=0xC3)[1]
        assert a.tobytes() == b.tobytes(), names


@pytest.mark.parametrize("names", [G.BATCH3, G.WS_BATCH3])
def test_batch_equals_the_problems_alone(rig, names):
    """B = 3 with different pair counts, the middle one returning early, whatever the workspace held: each problem's bytes are those of a call of its own"""
    ps = G.batch([G.scene(n) for n in names])
    together, _ = rig.run(ps, ws_fill=0xFF)
    assert [int(r["header"][7]) for r in together] == [2, 1, 2]
    for b, p in enumerate(ps):
        (alone,), _ = rig.run([p], ws_fill=0x00)
        for k in alone:
            assert np.array_equal(together[b][k], alone[k], equal_nan=True), (names, b, k)
        check(together[b], R.rule(p), f"{names[b]} in a batch")


def test_side1_shared_equals_copies(rig):
    ps = G.batch([G.scene(n) for n in G.BATCH3])
    shared = [dict(p, **{k: ps[0][k] for k, _ in G.SIDE1}) for p in ps]
    a, _ = rig.run(shared, side1_shared=True)
    b, _ = rig.run(shared, side1_shared=False)
    for x, y in zip(a, b):
        for k in x:
            assert np.array_equal(x[k], y[k], equal_nan=True), k


@pytest.mark.parametrize("name", ["out100", "e1025"])
def test_in_place_equals_out_of_place(rig, name):
    """d_assigned_out = d_assigned and d_S12_out = d_S12, the latter in the solver's layout (13 floats in a record of 32, the rest untouched)"""
    p = [G.scene(name)]
    (out,), _ = rig.run(p)
    (inp,), _ = rig.run(p, in_place=True, s12_stride=32)
    for k in out:
        assert np.array_equal(out[k], inp[k], equal_nan=True), k


def test_host_pointer_form_equals_the_device_form(rig):
    L = rig.L
    for name in ("out100", "keep9"):
        p = G.scene(name)
        (dev,), _ = rig.run([p])
        n1 = len(p["assigned"])
        arrays = [np.ascontiguousarray(np.asarray(p[k], dt)) for k, dt in G.SIDE1 + G.SIDE2]
        outs = dict(assigned_out=np.zeros(n1, np.int32), status=np.zeros(n1, np.uint8), chi2=np.zeros((n1, 2), F), state=np.zeros(8, D), S12_out=np.zeros(13, F),
                    Tcw=np.zeros(12, F), Ow=np.zeros(3, F), header=np.zeros(16, np.int32), final_chi2=np.zeros(1, D))
        c1, c2 = G.cam_struct(), G.cam_struct()
        rc = L.xfh_sim3_optimize(rig.ctx.h, n1, len(p["points1"]), len(p["points2"]), len(p["xy_un2"]), *[a.ctypes.data for a in arrays],
                                 np.asarray(p["S12"], F).ctypes.data, np.asarray(p["Tmw"], F).ctypes.data, C.byref(c1), C.byref(c2), p["th2"], p["fix_scale"],
                                 p["all_points"], p["inv_sigma2_1"], p["inv_sigma2_2"], *[o.ctypes.data for o in outs.values()])
        assert rc == 0
        for k, v in outs.items():
            assert np.array_equal(np.asarray(dev[k]).reshape(-1), v.reshape(-1), equal_nan=True), (name, k)


def test_context_method_equals_the_device_form(rig):
    """Context.sim3_optimize of xfeatslam_amd/extractor.py (the host-pointer form behind the Python mirror), with and without the composed pose"""
    p = G.scene("all_points")
    (dev,), _ = rig.run([p])
    cam = G.cam_struct()
    args = [p[k] for k, _ in G.SIDE1 + G.SIDE2] + [p["S12"], cam, cam]
    r = rig.ctx.sim3_optimize(*args, Tmw=p["Tmw"], th2=p["th2"], fix_scale=p["fix_scale"], all_points=p["all_points"])
    assert r["ret"] == int(dev["header"][6]) and list(r["header"].values()) == dev["header"][:12].tolist()
    for k, d in (("assigned", "assigned_out"), ("status", "status"), ("chi2", "chi2"), ("state", "state"), ("S12", "S12_out"), ("Tcw", "Tcw"), ("Ow", "Ow")):
        assert np.array_equal(np.asarray(r[k]).reshape(-1), np.asarray(dev[d]).reshape(-1)), k
    r2 = rig.ctx.sim3_optimize(*args, th2=p["th2"], fix_scale=p["fix_scale"], all_points=p["all_points"])
    assert r2["Tcw"] is None and np.array_equal(r2["S12"], r["S12"]) and np.array_equal(r2["assigned"], r["assigned"])
    assert rig.ctx.sim3_optimize_workspace_bytes(4096, 3) == rig.L.xfh_sim3_optimize_workspace_bytes(4096, 3) > 0


def hostile(seed, n1, level):
    """every array holds anything: ints far outside their range, NaN, Inf, huge and tiny floats"""
    rng = np.random.RandomState(seed)
    p = G.make(seed=seed, n_pairs=60, n1=n1, outliers=10, not_in_kf2=6, all_points=1)

    def ints(a, n):
        a = np.asarray(a).copy()
        k = rng.rand(a.size) < 0.4
        a[k] = rng.choice([np.iinfo(np.int32).min, np.iinfo(np.int32).max, -1, n, n + 1, 0, n - 1], int(k.sum()))
        return a

    def floats(a, share):
        a = np.asarray(a, F).copy()
        k = rng.rand(*a.shape) < share
        a[k] = rng.choice(np.array([np.nan, np.inf, -np.inf, 0.0, 3e38, -1e-38, 1e6, -7.0], F), int(k.sum()))
        return a
    p["assigned"], p["point1"], p["index2"] = ints(p["assigned"], len(p["points2"])), ints(p["point1"], len(p["points1"])), ints(p["index2"], len(p["xy_un2"]))
    p["flags2"] = rng.randint(0, 256, len(p["flags2"])).astype(np.uint8)
    if level:
        share = 0.05 if level == 1 else 1.0
        for k in ("T1w", "xy_un1", "points1", "points2", "xy_un2", "T2w", "S12", "Tmw"):
            p[k] = floats(p[k], share)
    return p


@pytest.mark.parametrize("n1", [300, 1500])
def test_hostile_input_returns_and_leaves_the_guards_alone(rig, n1):
    """the call terminates (the rig synchronises) and no byte outside the named outputs and the workspace changes (the rig asserts it).  With the
    index arrays spoiled and the geometry intact, which keypoints have a pair is still an exact function of the input: the status NO_EDGE and the
    three counts equal the rule's.  The numbers are not compared here: a spoiled index pairs a keypoint with an unrelated point, and on such scenes
    the float64 forms themselves lie thousands of float steps apart in chi2 (the rig's condition does not hold)."""
    for level in (0, 1, 2):
        ps = G.batch([hostile(100 * n1 + 10 * level + b, n1, level) for b in range(3)])
        res, _ = rig.run(ps)
        for r in res:
            assert R.header_in_bounds(r["header"]) and np.all(r["status"] <= R.INLIER), r["header"]
        if level == 0:
            for r, p in zip(res, ps):
                st = R.pairs_of(p)[0]
                assert np.array_equal(r["status"] == R.NO_EDGE, (st & R.EDGE) == 0)
                assert r["header"][:3].tolist() == [int((st != 0).sum()), int(((st & R.IN_KF2) != 0).sum()), int(((st != 0) & ((st & R.IN_KF2) == 0)).sum())]
                assert r["header"][0] > 0


def test_refusals(rig):
    L, p = rig.L, G.scene("clean30")
    n1, M1, nq, n2 = len(p["assigned"]), len(p["points1"]), len(p["points2"]), len(p["xy_un2"])
    buf = capi.DeviceBuffer(1 << 16)
    ptr, c1, c2 = buf.ptr, G.cam_struct(), G.cam_struct()
    good = dict(ctx=rig.ctx.h, B=1, n1=n1, M1=M1, nq=nq, n2=n2, shared=0, T1w=ptr, xy1=ptr, point1=ptr, points1=ptr, assigned=ptr, points2=ptr, flags2=ptr, index2=ptr,
                xy2=ptr, T2w=ptr, S12=ptr, S12_stride=13, Tmw=ptr, cam1=C.byref(c1), cam2=C.byref(c2), th2=10.0, fix_scale=0, all_points=0, w1=1.0, w2=1.0, ws=ptr,
                assigned_out=ptr, status=ptr, chi2=ptr, state=ptr, S12_out=ptr, S12_out_stride=13, Tcw=ptr, Ow=ptr, header=ptr, final_chi2=ptr)

    def refused(**kw):
        assert L.xfh_sim3_optimize_device(*dict(good, **kw).values()) == INVALID, kw
    refused(ctx=None)
    for k in ("n1", "M1", "nq", "n2"):
        for v in (0, capi.GRID_MAX_N + 1):
            refused(**{k: v})
    for v in (0, 65536):
        refused(B=v)
    for k, v in good.items():
        if v == ptr and k != "Tmw":
            refused(**{k: None})
            if k not in ("flags2", "status"):
                refused(**{k: ptr + (8 if k == "ws" else 4 if k in ("state", "final_chi2") else 2)})
    for k in ("cam1", "cam2"):
        refused(**{k: None})
    for k in ("th2", "w1", "w2"):
        for v in (0.0, -2.0, float("nan"), float("inf")):
            refused(**{k: v})
    for k in ("shared", "fix_scale", "all_points"):
        for v in (-1, 2):
            refused(**{k: v})
    refused(S12_stride=12)
    refused(S12_out_stride=12)
    rig.ctx.synchronize()
    buf.free()
