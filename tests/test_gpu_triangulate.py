"""xfh_triangulate_device (k_triangulate_pairs / _winner / _finish) against the rule form of tests/ref_triangulate.py on the scenes and with the
guarded runs of tests/triangulate_rig.py: statuses, kinds, headers, winners and the compact indices as integers, every float by its bits.  The
device's fp64 add, mul, div and sqrt and its fp32 div and sqrt are IEEE and the library is built without contraction, so no tolerance is needed
anywhere.  Shapes: n1 = 301, n2 = 515, B = 3; n1 = n2 = 65, B = 2; n1 = n2 = 1, B = 1.  The conditions the scenes are chosen for are asserted on
the CPU (tests/test_triangulate_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import ref_triangulate as RG
import triangulate_rig as R
import triangulation_rig as TR
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context, ORBmatcher

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def rig(gpu_lib):
    r = R.TriangRig(gpu_lib)
    yield r
    r.close()


@pytest.fixture(scope="module")
def main(oracle_mod):
    """the scene, the snapshot match12 of the restated search, and the rule with and without the claim: computed once, never changed"""
    s = R.main_scene()
    m = RG.snapshot_matches(s.dists(oracle_mod), s.k1, s.k2, s.F12, s.ep)
    P = R.main_params()
    return s, m, P, RG.rule_from_matches(P, s.k1, s.k2, m), RG.rule_from_matches(P, s.k1, s.k2, m, claim=False)


def test_three_neighbours_with_the_claim(rig, main):
    s, m, P, want, _ = main
    got, raw = rig.run(R.cam_struct(), [s.k1], s.k2, m, P, claim=True)
    R.assert_equals_rule(got, want)
    print("headers", got["header"].tolist(), "n_new", got["n_new"])
    assert np.array_equal(rig.run(R.cam_struct(), [s.k1], s.k2, m, P, claim=True)[1], raw)               # two runs: identical bytes


def test_shared_side_equals_separate_calls(rig, main):
    s, m, P, _, want = main
    got, raw = rig.run(R.cam_struct(), [s.k1], s.k2, m, P, claim=False)
    R.assert_equals_rule(got, want, claim=False)
    n1 = len(s.k1["xy"])
    lay3, lay1 = Context.triangulate_layout(3, n1, R.GUARD), Context.triangulate_layout(1, n1, R.GUARD)
    for b in range(3):
        one, raw1 = rig.run(R.cam_struct(), [s.k1], [s.k2[b]], m[b:b + 1], P, claim=False)
        for k, per in (("status", n1), ("kind", n1), ("xyz", 12 * n1), ("header", 32)):
            assert np.array_equal(raw1[lay1[k]:lay1[k] + per], raw[lay3[k] + b * per:lay3[k] + (b + 1) * per]), (b, k)


def test_own_side1_blocks(rig, main):
    s, m, P, _, _ = main
    roll = lambda k, p: dict(k, **{f: np.roll(k[f], p * TR.ROLL, 0) for f in ("xy", "ur", "depth")})
    side1 = [roll(s.k1, b) for b in range(3)]
    mr = np.stack([np.roll(m[b], b * TR.ROLL) for b in range(3)])
    got, _ = rig.run(R.cam_struct(), side1, s.k2, mr, P, claim=False)
    R.assert_equals_rule(got, RG.rule_from_matches(P, s.k1, s.k2, mr, claim=False, side1=side1), claim=False)
    mono1, mono2 = dict(s.k1, ur=None), [dict(k, ur=None) for k in s.k2]                                 # both uright NULL
    got, _ = rig.run(R.cam_struct(), [mono1], mono2, m, P, claim=True)
    R.assert_equals_rule(got, RG.rule_from_matches(P, mono1, mono2, m))


def test_planted_pairs_and_a_partial_wave(rig):
    o, m = R.planted()
    P = R.planted_params()
    for claim in (False, True):
        got, _ = rig.run(R.cam_struct(), [o.k1], o.k2, m, P, claim=claim)
        R.assert_equals_rule(got, RG.rule_from_matches(P, o.k1, o.k2, m, claim=claim), claim=claim)
    hostile = m.copy(); hostile[0, 9], hostile[0, 10], hostile[1, 11] = 65, -7, 2 ** 31 - 1                 # outside 0 .. n2 - 1: no match
    got, _ = rig.run(R.cam_struct(), [o.k1], o.k2, hostile, P, claim=True)
    R.assert_equals_rule(got, RG.rule_from_matches(P, o.k1, o.k2, hostile))
    assert got["status"][0, 9] == RG.NO_MATCH and got["status"][0, 10] == RG.NO_MATCH and got["status"][1, 11] == RG.NO_MATCH


def test_single_pairs_with_written_out_answers(rig):
    """n1 = n2 = 1, B = 1: every hand-made pair through the kernels"""
    for name, o1, o2, kw, want in R.handmade():
        P = RG.params(R.HCAM, **dict(dict(ratio_factor=R.RATIO_FACTOR, scale_last=R.SCALE_LAST), **kw))
        kf = lambda o: dict(xy=np.array([[o["x"], o["y"]]], F), xy_raw=np.array([[o["xr"], o["yr"]]], F), ur=np.array([o["ur"]], F), depth=np.array([o["depth"]], F),
                            Tcw=o["T"], Ow=o["Ow"])
        k1, k2 = kf(o1), kf(o2)
        m = np.zeros((1, 1), np.int32)
        got, _ = rig.run(R.cam_struct(R.HCAM), [k1], [k2], m, P, claim=True)
        R.assert_equals_rule(got, RG.rule_from_matches(P, k1, [k2], m))
        assert got["status"][0, 0] == want["status"] and got["kind"][0, 0] == want["kind"], name
        assert got["n_new"] == int(want["status"] == RG.ACCEPTED)


def test_host_form_and_matcher(gpu_lib, main):
    s, m, P, want, _ = main
    ctx = Context(nfeatures=1, max_height=32, max_width=32)
    try:
        got = ctx.triangulate(R.cam_struct(), s.k1, s.k2, m, sigma2=P["sigma2"], ratio_factor=P["ratio_factor"], scale_last=P["scale_last"], far_th=P["far_th"])
        R.assert_equals_rule(got, want)
        lst, _ = ORBmatcher(0.6, False, ctx=ctx).triangulate(R.cam_struct(), s.k1, s.k2, m, scale_factor=R.SCALE_FACTOR, scale_factor_last=R.SCALE_LAST, far_th=R.FAR_TH)
        assert [(i, b, j) for i, b, j, *_ in lst] == [(int(want["new_idx1"][q]), int(want["new_b"][q]), int(want["new_idx2"][q])) for q in range(want["n_new"])]
        assert all(st == bool(want["kind"][b, i]) for i, b, _, _, _, _, st in lst)
    finally:
        ctx.close()


def test_every_refusal_returns_before_anything_is_queued(rig):
    L, ctx = rig.L, rig.ctx
    n1, n2, B = 8, 8, 2
    lay = Context.triangulate_layout(B, n1, 0)
    out = capi.DeviceBuffer(lay["bytes"]).upload(np.full(lay["bytes"], 0xA5, np.uint8))
    inp = capi.DeviceBuffer(4096).upload(np.zeros(4096, np.uint8))
    cam = R.cam_struct()
    d = inp.ptr

    def call(B=B, n1=n1, n2=n2, shared=1, flags=capi.TRIANG_CLAIM, sigma2=1.0, rf=1.8, sl=1.0, far=0.0, cam=cam, **ptr):
        a = dict(xy1=d, raw1=None, ur1=d, z1=d, T1=d, O1=d, xy2=d, raw2=None, ur2=d, z2=d, T2=d, O2=d, m=d, status=out.ptr + lay["status"], kind=out.ptr + lay["kind"],
                 xyz=out.ptr + lay["xyz"], header=out.ptr + lay["header"])
        a.update({k: out.ptr + lay[k] for k in Context.TRIANG_CLAIM_OUT})
        a.update(ptr)
        return L.xfh_triangulate_device(ctx.h, B, n1, n2, shared, flags, C.byref(cam) if cam is not None else None, sigma2, rf, sl, far, *a.values())

    bad = [call(B=0), call(B=65536), call(n1=0), call(n1=capi.GRID_MAX_N + 1), call(n2=0), call(n2=capi.GRID_MAX_N + 1), call(shared=2), call(flags=4), call(flags=8 | 2),
           call(shared=0), call(cam=None), call(sigma2=float("nan")), call(rf=float("inf")), call(sl=float("nan")), call(far=float("-inf")),
           call(z1=None), call(z2=None), call(xy1=d + 2), call(m=d + 1), call(xyz=out.ptr + lay["xyz"] + 2), call(n_new=out.ptr + lay["n_new"] + 1)]
    bad += [call(**{k: None}) for k in ("xy1", "T1", "O1", "xy2", "T2", "O2", "m", "status", "kind", "xyz", "header") + Context.TRIANG_CLAIM_OUT]
    assert all(rc == 1 for rc in bad), bad
    ctx.synchronize()
    assert np.all(out.download(np.uint8, lay["bytes"]) == 0xA5)
    assert call(shared=0, flags=0, **{k: None for k in Context.TRIANG_CLAIM_OUT}) == 0 and call(ur1=None, z1=None) == 0     # what IS allowed
    ctx.synchronize()
    out.free(); inp.free()


def test_chain_search_then_triangulate(rig, main, oracle_mod):
    """xfh_triangulation_search_device writes d_match12; xfh_triangulate_device reads that same buffer, no host step between: the result is the
    rule form run on the restated search"""
    s, m, P, want, _ = main
    ctx = rig.ctx
    B, n1, n2 = 3, len(s.k1["xy"]), len(s.k2[0]["xy"])
    s1, s2 = TR.TriRig.side([s.k1]), TR.TriRig.side(s.k2)
    lay = Context.triangulation_search_layout(B, n1, 0)
    sout = capi.DeviceBuffer(lay["bytes"])
    d1 = [rig.dev(s1[k]) for k in ("blob", "xy", "ur", "has", "desc")]; d2 = [rig.dev(s2[k]) for k in ("blob", "xy", "ur", "has", "desc")]
    dF, de = rig.dev(np.stack(s.F12).astype(F)), rig.dev(np.stack(s.ep).astype(F))
    ctx.triangulation_search_device(B, n1, n2, True, *d1, s1["stride"], *d2, s2["stride"], dF, de, sout.ptr)
    keep, rig.bufs = rig.bufs, []                                          # (rig.run frees its own uploads)
    got, _ = rig.run(R.cam_struct(), [s.k1], s.k2, None, P, claim=True, d_match12=sout.ptr + lay["match12"])
    assert np.array_equal(sout.download(np.int32, B * n1, lay["match12"]).reshape(B, n1), m)
    R.assert_equals_rule(got, want)
    rig.bufs = keep; rig.free(); sout.free()
