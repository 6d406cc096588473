"""xfh_two_view_device (k_twoview_prepare / _fit / _score / _select / _check_rt / _final) against the rule form of tests/ref_twoview.py on the
scenes and with the guarded runs of tests/twoview_rig.py: the header as integers, every float by its bits.  The device's fp64 and fp32 add, mul,
div and sqrt are IEEE and the library is built without contraction, so no tolerance is needed anywhere.  Shapes: n1 = 301, n2 = 515, B = 3,
iters = 200; n1 = n2 = 65, B = 2, iters = 24 (one past a wave); n1 = n2 = 8, B = 1, iters = 3; seven matches; iters = 1; n1 = n2 = 4096.  The call
supports the whole range 1 .. XFH_GRID_MAX_N: its scoring reads the coordinates through the caches instead of staging them in LDS, so there is no
smaller limit to refuse."""
import ctypes as C

import numpy as np
import pytest

import ref_twoview as R
import twoview_rig as G
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def rig(gpu_lib):
    r = G.TwoViewRig(gpu_lib)
    yield r
    r.close()


@pytest.fixture(scope="module")
def scenes():
    """the rig's scenes and the rule's answer for each: computed once, never changed"""
    s = G.rig()
    return s, {k: G.rule_of(v) for k, v in s.items()}


def one(s):
    return tuple(a[None] for a in (s["xy1"], s["xy2"], s["m12"])) + (s["draws"],)


def test_three_problems_200_iterations(rig, scenes):
    """n1 = 301, n2 = 515, B = 3, iters = 200, per-problem draws; two runs give identical bytes; B problems equal B separate calls"""
    s, want = scenes
    names = ("general", "ambiguous", "collinear")
    xy1, xy2, m12, draws = G.stack([s[n] for n in names])
    got, raw = rig.run(xy1, xy2, m12, draws)
    for b, n in enumerate(names):
        G.assert_equals_rule(got, want[n], b)
        print(n, dict(zip(R.HEADER, got["header"][b].tolist())))
    assert np.array_equal(rig.run(xy1, xy2, m12, draws)[1], raw)
    lay3, lay1 = Context.two_view_layout(3, 301, G.GUARD), Context.two_view_layout(1, 301, G.GUARD)
    for b in range(3):
        _, raw1 = rig.run(xy1[b:b + 1], xy2[b:b + 1], m12[b:b + 1], draws[b])
        for k in Context.TWO_VIEW_OUT:
            per = lay1[k + "_bytes"]
            assert np.array_equal(raw1[lay1[k]:lay1[k] + per], raw[lay3[k] + b * per:lay3[k] + (b + 1) * per]), (b, k)


def test_shared_draws_equal_per_problem_copies(rig, scenes):
    s, want = scenes
    names = ("general", "collinear", "equal")
    xy1, xy2, m12, _ = G.stack([s[n] for n in names])
    d = s["general"]["draws"]
    got, raw = rig.run(xy1, xy2, m12, d)                                                     # stride 0
    got2, raw2 = rig.run(xy1, xy2, m12, np.stack([d, d, d]))
    assert np.array_equal(raw, raw2)
    G.assert_equals_rule(got, want["general"], 0)
    G.assert_equals_rule(got, R.rule(s["equal"]["xy1"], s["equal"]["xy2"], s["equal"]["m12"], G.CAM, d, G.RAND_MAX), 2)


def test_every_status_of_the_rig_is_reached_on_the_device(rig, scenes):
    s, want = scenes
    seen = set()
    for n, sc in s.items():
        got, _ = rig.run(*one(sc), sigma=sc["sigma"], cam=sc.get("cam"))
        G.assert_equals_rule(got, want[n], 0, prior_byte=0xA5)
        assert R.STATUS_NAMES[got["header"][0, 1]] == G.EXPECT[n], n
        seen.add(int(got["header"][0, 1]))
    assert seen == set(range(8))


def test_one_past_a_wave_and_the_smallest_shapes(rig):
    """n1 = n2 = 65, B = 2, iters = 24; n1 = n2 = 8, iters = 3; n1 = 7 (TOO_FEW: the header and nothing else); iters = 1"""
    a, b = G.scene(21, 65, 65, 65, noise=0.2, outliers=0.1, iters=24), G.scene(22, 65, 65, 60, kind="plane", noise=0.2, outliers=0.0, iters=24)
    xy1, xy2, m12, draws = G.stack([a, b])
    got, _ = rig.run(xy1, xy2, m12, draws)
    for k, sc in enumerate((a, b)):
        G.assert_equals_rule(got, G.rule_of(dict(sc, sigma=1.0)), k)
    c = dict(G.scene(23, 8, 8, 8, noise=0.0, outliers=0.0, iters=3), sigma=1.0)
    got, _ = rig.run(*one(c))
    G.assert_equals_rule(got, G.rule_of(c), 0)
    assert got["header"][0, 0] == 8
    d = dict(G.scene(24, 7, 9, 7, iters=3), sigma=1.0)
    got, _ = rig.run(*one(d))
    G.assert_equals_rule(got, G.rule_of(d), 0, prior_byte=0xA5)
    assert got["header"][0, :2].tolist() == [7, R.TOO_FEW]
    e = dict(G.scene(25, 301, 515, 220, iters=1), sigma=1.0)
    got, _ = rig.run(*one(e))
    G.assert_equals_rule(got, G.rule_of(e), 0)


def test_4096_keypoints(rig):
    s = dict(G.scene(31, 4096, 4096, 3900, noise=0.3, outliers=0.05, iters=32), sigma=1.0)
    got, _ = rig.run(*one(s))
    want = G.rule_of(s)
    G.assert_equals_rule(got, want, 0)
    assert want["header"][1] == R.OK_F and want["header"][0] == 3900


def test_hostile_matches_and_draws(rig, scenes):
    s, _ = scenes
    sc = dict(s["general"])
    m = sc["m12"].copy(); m[3], m[4], m[5], m[6] = 515, -7, 2 ** 31 - 1, m[7]                # outside 0 .. n2 - 1: no match; a duplicate idx2
    d = sc["draws"].copy(); d[2] = -5; d[3, ::2] = 2 ** 31 - 1
    sc.update(m12=m, draws=d)
    got, _ = rig.run(*one(sc))
    G.assert_equals_rule(got, G.rule_of(sc), 0)


def test_host_pointer_form(gpu_lib, scenes):
    s, want = scenes
    ctx = Context(nfeatures=1, max_height=32, max_width=32)
    try:
        for n in ("general", "plane", "n7", "nonfinite"):
            sc = s[n]
            got = ctx.two_view(G.camera(sc.get("cam")), sc["xy1"], sc["xy2"], sc["m12"], sc["draws"], G.RAND_MAX, sigma=sc["sigma"])
            G.assert_equals_rule(got, want[n], 0)
    finally:
        ctx.close()


def test_every_refusal_returns_before_anything_is_queued(rig):
    L, ctx = rig.L, rig.ctx
    buf = capi.DeviceBuffer(1 << 16)
    cam = G.camera()
    p = buf.ptr

    def call(B=1, n1=8, n2=8, iters=2, sigma=1.0, stride=0, rand_max=7, mpc=0.9998, mt=50, cam_=cam, ptrs=None, h=None):
        ptrs = dict(dict(xy1=p, xy2=p, m=p, draws=p, ws=p, hd=p, fl=p, ih=p, if_=p, tr=p, p3=p, mo=p), **(ptrs or {}))
        return L.xfh_two_view_device(ctx.h if h is None else h, B, n1, n2, ptrs["xy1"], ptrs["xy2"], ptrs["m"], None if cam_ is None else C.byref(cam_), sigma, iters,
                                     ptrs["draws"], stride, rand_max, mpc, mt, ptrs["ws"], ptrs["hd"], ptrs["fl"], ptrs["ih"], ptrs["if_"], ptrs["tr"], ptrs["p3"], ptrs["mo"])
    try:
        bad = [call(B=0), call(B=65536), call(n1=0), call(n1=capi.GRID_MAX_N + 1), call(n2=0), call(n2=capi.GRID_MAX_N + 1), call(iters=0),
               call(iters=capi.TWO_VIEW_MAX_ITERS + 1), call(sigma=0.0), call(sigma=float("nan")), call(sigma=float("inf")), call(rand_max=0),
               call(mpc=float("nan")), call(mt=-1), call(cam_=None), call(B=2, stride=15)]
        bad += [call(ptrs={k: None}) for k in ("xy1", "xy2", "m", "draws", "ws", "hd", "fl", "ih", "if_", "tr", "p3", "mo")]
        bad += [call(ptrs={k: p + 2}) for k in ("xy1", "xy2", "m", "draws", "hd", "fl", "p3", "mo")] + [call(ptrs=dict(ws=p + 8))]
        assert all(rc == 1 for rc in bad), bad
        assert L.xfh_two_view_workspace_bytes(capi.GRID_MAX_N + 1, 8, 2, 1) == 0 and L.xfh_two_view_workspace_bytes(capi.GRID_MAX_N, capi.GRID_MAX_N, 200, 1) > 0
        ctx.synchronize()                                                   # nothing was queued: the stream is idle and no error is pending
    finally:
        buf.free()
