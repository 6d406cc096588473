"""CPU tests of the two-view reconstruction (xfh_two_view*): the library's host code -- the very lines the kernels compile, twoview_math.h --
against the rule form of tests/ref_twoview.py BY BITS on the scenes of tests/twoview_rig.py; the set generator against the reference's
shrinking-vector loop; hand-made cases with written-out answers; the scenes' geometry against the motion they were made with; every refusal
that needs no device; and the stand-alone sanitizer program.  No GPU is used."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_twoview as R
import twoview_rig as G
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
bits = lambda a: np.ascontiguousarray(a).view(np.uint8).ravel()


@pytest.fixture(scope="module")
def scenes():
    s = G.rig()
    return s, {k: G.rule_of(v) for k, v in s.items()}


def host(s, **kw):
    return Context.two_view_host(G.camera(s.get("cam")), s["xy1"], s["xy2"], s["m12"], s["draws"], G.RAND_MAX, sigma=s["sigma"], **kw)


def test_host_form_equals_the_rule_by_bits_and_every_status_is_reached(scenes):
    s, want = scenes
    seen = set()
    for n, sc in s.items():
        G.assert_equals_rule(host(sc), want[n], 0)
        assert R.STATUS_NAMES[want[n]["header"][1]] == G.EXPECT[n], (n, dict(zip(R.HEADER, want[n]["header"].tolist())))
        seen.add(int(want[n]["header"][1]))
    assert seen == set(range(8))


def test_conditions_of_the_scenes(scenes):
    """what each scene is in the rig for"""
    s, want = scenes
    h = lambda n: dict(zip(R.HEADER, want[n]["header"].tolist()))
    assert h("general")["model"] == R.MODEL_F and h("plane")["model"] == R.MODEL_H and h("plane")["n_hyp"] == 8
    assert h("n7")["N"] == 7 and h("n8")["N"] == 8
    g = h("ambiguous")                                                      # two hypotheses above 0.7 maxGood
    ng = [g[f"ngood{k}"] for k in range(4)]
    assert sum(v > 0.7 * max(ng) for v in ng) == 2 and max(ng) >= max(int(0.9 * g["inliers_f"]), 50)
    g = h("few")                                                            # fewer than 51 counted pairs: the index is size - 1, the largest cosine
    assert 0 < g["ngood3"] < 51
    r = want["few"]
    idx = np.nonzero(r["inl_f"])[0]
    v, c, _ = R.check_rt(G.CAM, r["motions"][3], 1.0, s["few"]["xy1"][idx, 0], s["few"]["xy1"][idx, 1], s["few"]["xy2"][s["few"]["m12"][idx], 0],
                         s["few"]["xy2"][s["few"]["m12"][idx], 1])
    assert r["floats"][R.F_COS + 3] == c[v != 0].max()
    r = want["collinear"]                                                   # iteration 0 fits eight collinear points: it neither wins nor poisons the argmax
    sets0 = r["sets"][0]
    assert len(set(s["collinear"]["xy1"][r["cm"][0][sets0], 1].tolist())) == 1
    assert r["header"][3] != 0 and r["header"][4] != 0 and np.isfinite(r["floats"][:3]).all()
    r = want["equal"]                                                       # iterations 198 and 199 draw the same set: the earlier one wins
    assert r["score"][1][198].tobytes() == r["score"][1][199].tobytes() and r["score"][1][198] == r["score"][1].max() and r["header"][4] == 198
    r = want["still"]
    assert np.allclose(r["floats"][R.F_H21:R.F_H21 + 9] / r["floats"][R.F_H21 + 8], np.eye(3).ravel(), atol=5e-3) and r["header"][17] == 0      # the translation entries are pixels
    r = want["rotation_h"]                                                  # H without a baseline: four hypotheses triangulate the same
    assert sorted(r["header"][5:13].tolist())[-4:] == [99, 99, 99, 99]
    r, i = want["epipole"], s["epipole"]["epipole_idx1"]                    # a match at the two epipoles: an inlier of F on the baseline, never triangulated
    assert r["inl_f"][i] == 1 and r["tri"][i] == 0 and r["matches_out"][i] == -1 and r["header"][1] == R.OK_F
    r = want["outliers"]
    assert r["floats"][0] == 0 and r["floats"][1] == 0 and r["header"][3] == -1 and r["header"][4] == -1
    r, sc = want["nonfinite"], s["nonfinite"]                               # every inlier of the chosen model triangulates to a non-finite point and is skipped
    idx = np.nonzero(r["inl_f"])[0]
    assert r["header"][2] == R.MODEL_F and len(idx) >= 150 and r["header"][17] == 4 and np.isfinite(r["floats"][:21]).all()
    for Rt in r["motions"]:
        v, c, p = R.check_rt(sc["cam"], Rt, 1.0, sc["xy1"][idx, 0], sc["xy1"][idx, 1], sc["xy2"][sc["m12"][idx], 0], sc["xy2"][sc["m12"][idx], 1])
        assert not np.isfinite(p).all(1).any() and not v.any() and not c.any()
    assert r["header"][5:13].tolist() == [0] * 8 and r["floats"][R.F_COS:R.F_COS + 8].tolist() == [1.0] * 8 and r["header"][1] == R.F_NO_WINNER
    assert not r["tri"].any() and not r["p3d"].any() and np.array_equal(r["matches_out"], sc["m12"])


def test_successful_scenes_recover_the_motion_they_were_made_with(scenes):
    """T21 against the scene's R, t / |t| (the scale is free) and the points against their reprojection.  Bounds from the noise: 0.3 px at f = 458
    is 0.04 degrees per ray; a pose from ~200 such rays over a 3-degree motion is far inside 0.5 degrees of rotation, and the direction of a
    translation whose flow is a few tens of pixels inside 5 degrees."""
    s, want = scenes
    for n in ("general", "plane", "collinear", "equal", "epipole"):
        r, sc = want[n], s[n]
        T = r["floats"][R.F_T21:R.F_T21 + 12].reshape(3, 4).astype(np.float64)
        Rm, t = T[:, :3], T[:, 3]
        assert abs(np.linalg.det(Rm) - 1) < 1e-4 and abs(np.linalg.norm(t) - 1) < 1e-5
        ang = np.degrees(np.arccos(np.clip((np.trace(Rm @ sc["R"].T) - 1) / 2, -1, 1)))
        dirn = np.degrees(np.arccos(np.clip(t @ sc["t"] / np.linalg.norm(sc["t"]), -1, 1)))
        assert ang < 0.5 and dirn < 5.0, (n, ang, dirn)
        tri = np.nonzero(r["tri"])[0]
        assert len(tri) == r["header"][16] >= 50 and np.all(r["matches_out"][tri] == sc["m12"][tri])
        lost = (sc["m12"] >= 0) & (r["tri"] == 0)
        assert np.all(r["matches_out"][lost] == -1) and np.all(r["matches_out"][sc["m12"] < 0] == sc["m12"][sc["m12"] < 0])
        P = r["p3d"][tri].astype(np.float64)
        e1 = G.project(P, np.eye(3), np.zeros(3)) - sc["xy1"][tri]
        e2 = G.project(P, Rm, t) - sc["xy2"][sc["m12"][tri]]
        assert (e1 ** 2).sum(1).max() <= 4.0 + 1e-3 and (e2 ** 2).sum(1).max() <= 4.0 + 1e-3 and P[:, 2].min() > 0
    for n in ("rotation", "small_baseline", "ambiguous", "outliers", "still", "rotation_h", "nonfinite"):     # a failed call changes no match and triangulates nothing
        assert np.array_equal(want[n]["matches_out"], s[n]["m12"]) and not want[n]["tri"].any() and not want[n]["floats"][R.F_T21:R.F_T21 + 12].any()


def test_set_generator_equals_the_shrinking_vector_loop():
    rng = np.random.RandomState(5)
    for rand_max in (32767, 2147483647, 1):
        for N in (8, 9, 65, 1000):
            for k in range(60):
                d = rng.randint(0, rand_max + 1, 8, dtype=np.int64).astype(np.int32)
                if k == 0:
                    d[:] = 0
                elif k == 1:
                    d[:] = rand_max
                elif k == 2:
                    d[::2], d[1::2] = 0, rand_max
                got = Context.two_view_set(d, rand_max, N).tolist()
                assert got == R.set_of_iteration(d, rand_max, N), (rand_max, N, d.tolist())
                assert len(set(got)) == 8 and min(got) >= 0 and max(got) < N
    assert Context.two_view_set([0] * 8, 32767, 10).tolist() == [0, 9, 8, 7, 6, 5, 4, 3]              # position 0 is refilled from the back each time
    assert Context.two_view_set([32767] * 8, 32767, 10).tolist() == [9, 8, 7, 6, 5, 4, 3, 2]          # always the last position
    assert Context.two_view_set([16384] * 8, 32767, 8).tolist() == [4, 3, 6, 2, 7, 1, 5, 0]           # int(0.5 * d) of the shrinking vector, by hand
    assert Context.two_view_set([40000, -3] + [0] * 6, 32767, 9).tolist()[:2] == [8, 0]               # outside 0 .. rand_max: clamped into the vector


def test_host_pieces_equal_the_rule_on_every_iteration(scenes):
    """every rig scene with eight matches or more, every iteration: the set, both fits, and the score terms of both models for three matches that
    move with the iteration (the same lines run for every match; all of them are run for the two winning iterations); CheckRT for every inlier of
    the chosen model under every motion hypothesis, the cosine included where the verdict is 0"""
    s, want = scenes
    eq = lambda a, b: bits(np.asarray(a, F)).tobytes() == bits(np.asarray(b, F)).tobytes()
    ran = 0
    for n, sc in s.items():
        r = want[n]
        if r["header"][0] < 8:
            continue
        ran += 1
        cam = sc.get("cam", G.CAM)
        cm1, cm2 = r["cm"]
        N, iters = len(cm1), len(sc["draws"])
        p1 = R.normalized(r["nrm"][0], sc["xy1"][cm1[r["sets"]]])
        p2 = R.normalized(r["nrm"][1], sc["xy2"][cm2[r["sets"]]])
        Hn, Fn = R.fit_h(p1, p2), R.fit_f(p1, p2)
        u1, v1, u2, v2 = sc["xy1"][cm1, 0], sc["xy1"][cm1, 1], sc["xy2"][cm2, 0], sc["xy2"][cm2, 1]
        terms = [R.score_terms(m + 1, r["hyp"][m], sc["sigma"], u1, v1, u2, v2) for m in range(2)]
        for it in range(iters):
            assert Context.two_view_set(sc["draws"][it], G.RAND_MAX, N).tolist() == r["sets"][it].tolist(), (n, it)
            assert eq(Context.two_view_fit(R.MODEL_H, p1[it], p2[it]), Hn[it]) and eq(Context.two_view_fit(R.MODEL_F, p1[it], p2[it]), Fn[it]), (n, it)
            for m in range(2):
                chi, inl, term = terms[m]
                ks = range(N) if it == r["header"][3 + m] else sorted({(7 * it) % N, (13 * it + 5) % N, N - 1 - it % N})
                for k in ks:
                    c, i, t = Context.two_view_score(m + 1, r["hyp"][m][it], sc["sigma"], sc["xy1"][cm1[k]], sc["xy2"][cm2[k]])
                    assert eq(c, chi[it, k]) and i == int(inl[it, k]) and eq(t, term[it, k]), (n, m, it, k)
        idx = np.nonzero(r["inl_h"] if r["header"][2] == R.MODEL_H else r["inl_f"])[0] if r["header"][2] else []
        for h, Rt in enumerate(r["motions"]):
            v, c, p = R.check_rt(cam, Rt, sc["sigma"], sc["xy1"][idx, 0], sc["xy1"][idx, 1], sc["xy2"][sc["m12"][idx], 0], sc["xy2"][sc["m12"][idx], 1])
            for k, i in enumerate(idx):
                gv, gc, gp = Context.two_view_check_rt(G.camera(cam), Rt, sc["sigma"], sc["xy1"][i], sc["xy2"][sc["m12"][i]])
                assert gv == v[k] and eq(gp, p[k]) and eq(gc, c[k]), (n, h, i)
    assert ran == len(s) - 1                                                # all but n7


def test_hand_made_cases_with_written_out_answers():
    eye18 = np.concatenate([np.eye(3).ravel(), np.eye(3).ravel()]).astype(F)
    th = F(5.991)
    chi, inl, term = Context.two_view_score(R.MODEL_H, eye18, 1.0, [10, 20], [11, 20])               # identity H, one pixel apart: chi = 1 both ways
    assert chi.tolist() == [1.0, 1.0] and inl == 1 and term == (th - F(1)) + (th - F(1))
    chi, inl, term = Context.two_view_score(R.MODEL_H, eye18, 1.0, [10, 20], [13, 20])               # three pixels: 9 > 5.991
    assert chi.tolist() == [9.0, 9.0] and inl == 0 and term == 0
    chi, inl, term = Context.two_view_score(R.MODEL_H, eye18, 2.0, [10, 20], [13, 20])               # sigma 2: 9 / 4
    assert chi.tolist() == [2.25, 2.25] and inl == 1 and term == (th - F(2.25)) + (th - F(2.25))
    Fx = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], F)                                                   # translation along x: l2 = (0, -1, v1), distance |v2 - v1|
    chi, inl, term = Context.two_view_score(R.MODEL_F, Fx, 1.0, [10, 20], [50, 21])
    assert chi.tolist() == [1.0, 1.0] and inl == 1 and term == (th - F(1)) + (th - F(1))
    chi, inl, term = Context.two_view_score(R.MODEL_F, Fx, 1.0, [10, 20], [50, 22])                  # 4 > 3.841: an outlier under F although 4 < 5.991
    assert chi.tolist() == [4.0, 4.0] and inl == 0 and term == 0
    chi, inl, term = Context.two_view_score(R.MODEL_F, Fx, 1.0, [10, 20], [float("nan"), 21])        # a NaN passes `chi > th` as in the reference and poisons the sum
    assert inl == 1 and np.isnan(term)
    fx, fy, cx, cy = [float(c) for c in G.CAM]
    T = np.array([[1, 0, 0, -1], [0, 1, 0, 0], [0, 0, 1, 0]], F)                                      # camera 2 one unit to the right; the point (0, 0, 4)
    v, c, p = Context.two_view_check_rt(G.camera(), T, 1.0, [cx, cy], [cx - fx / 4, cy])
    assert v == 2 and np.allclose(p, [0, 0, 4], atol=1e-4) and abs(c - 4 / np.sqrt(17)) < 1e-6
    v, c, p = Context.two_view_check_rt(G.camera(), T, 1.0, [cx, cy], [cx + fx / 4, cy])              # the rays meet behind both cameras
    assert v == 0 and p[2] < 0
    v, c, p = Context.two_view_check_rt(G.camera(), T, 1.0, [cx, cy], [cx - fx / 4, cy + 2])          # 2 px off the epipolar line: the point splits it, 1 px in each image
    assert v == 2
    v, c, p = Context.two_view_check_rt(G.camera(), T, 1.0, [cx, cy], [cx - fx / 4, cy + 6])          # 6 px off: about 3 px in each image, 9 > 4 sigma^2
    assert v == 0
    v, c, p = Context.two_view_check_rt(G.camera(), T, 1.0, [cx, cy], [cx - fx / 4000, cy])           # depth 4000: counted, but the parallax is too small to be good
    assert v == 1 and c > 0.99998
    v, c, p = Context.two_view_check_rt(G.camera(), T, 1.0, [float("nan"), cy], [cx, cy])              # a NaN row: nothing rotates, x3Dh = (1, 0, 0, 0), the point (1 / 0, 0 / 0, 0 / 0) is skipped
    assert v == 0 and p[0] == np.inf and np.isnan(p[1]) and np.isnan(p[2])
    assert Context.two_view_cos(1.0) == float(np.cos(np.pi / 180.0))


def test_decisions_at_their_thresholds():
    cos1 = R.DEFAULT_COS
    d = lambda model, ng, cs, n, deg=False: R.decide(model, deg, ng + [0] * (8 - len(ng)), [F(c) for c in cs] + [F(1)] * (8 - len(cs)), n, cos1, 50)
    assert d(R.MODEL_F, [100, 70, 0, 0], [0.99] * 4, 100) == (R.OK_F, 0)                              # 70 > 0.7 * 100 is false
    assert d(R.MODEL_F, [100, 71, 0, 0], [0.99] * 4, 100) == (R.F_NO_WINNER, -1)
    assert d(R.MODEL_F, [89, 0, 0, 0], [0.99] * 4, 100) == (R.F_NO_WINNER, -1) and d(R.MODEL_F, [90, 0, 0, 0], [0.99] * 4, 100) == (R.OK_F, 0)
    assert d(R.MODEL_F, [49, 0, 0, 0], [0.99] * 4, 20) == (R.F_NO_WINNER, -1) and d(R.MODEL_F, [0, 0, 50, 0], [1, 1, 0.99, 1], 20) == (R.OK_F, 2)
    assert d(R.MODEL_F, [60, 0, 60, 0], [0.99999, 1, 0.99, 1], 60)[0] == R.F_NO_WINNER                 # two equal: nsimilar = 2
    assert d(R.MODEL_F, [60, 0, 0, 0], [0.99999, 1, 1, 1], 60) == (R.LOW_PARALLAX, -1)
    assert d(R.MODEL_H, [100, 74] + [0] * 6, [0.99] * 8, 100) == (R.OK_H, 0) and d(R.MODEL_H, [100, 75] + [0] * 6, [0.99] * 8, 100)[0] == R.H_GATES
    assert d(R.MODEL_H, [50] + [0] * 7, [0.99] * 8, 50)[0] == R.H_GATES and d(R.MODEL_H, [51] + [0] * 7, [0.99] * 8, 51) == (R.OK_H, 0)
    assert d(R.MODEL_H, [90] + [0] * 7, [0.99] * 8, 100)[0] == R.H_GATES and d(R.MODEL_H, [0, 0, 91] + [0] * 5, [1, 1, 0.99] + [1] * 5, 100) == (R.OK_H, 2)
    assert d(R.MODEL_H, [91] + [0] * 7, [0.99999] + [1] * 7, 100)[0] == R.LOW_PARALLAX and d(R.MODEL_H, [0] * 8, [1] * 8, 100)[0] == R.H_GATES
    assert d(R.MODEL_H, [91] + [0] * 7, [0.99] * 8, 100, deg=True)[0] == R.H_DEGENERATE
    assert d(R.MODEL_H, [60, 70, 0, 0, 0, 0, 0, 0], [0.99] * 8, 60)[0] == R.H_GATES                   # the second best of an earlier hypothesis counts


def test_batches_strides_and_untouched_outputs_on_the_host(scenes):
    s, want = scenes
    names = ("general", "collinear", "equal")
    xy1, xy2, m12, draws = G.stack([s[n] for n in names])
    cam = G.camera()
    got = Context.two_view_host(cam, xy1, xy2, m12, draws, G.RAND_MAX)
    for b, n in enumerate(names):
        G.assert_equals_rule(got, want[n], b)
    d = s["general"]["draws"]
    shared, copies = Context.two_view_host(cam, xy1, xy2, m12, d, G.RAND_MAX), Context.two_view_host(cam, xy1, xy2, m12, np.stack([d, d, d]), G.RAND_MAX)
    assert all(bits(shared[k]).tobytes() == bits(copies[k]).tobytes() for k in R.OUTPUTS)
    sc = s["n7"]                                                            # TOO_FEW: the header and nothing else
    prior = dict(floats=np.full(48, 7.5, F), inl_h=np.full(65, 9, np.uint8), inl_f=np.full(65, 9, np.uint8), tri=np.full(65, 9, np.uint8),
                 p3d=np.full((65, 3), -2.0, F), matches_out=np.full(65, 77, np.int32))
    got = host(sc, prior=prior)
    assert got["header"][0].tolist() == [7, 0, 0, -1, -1] + [0] * 8 + [-1] + [0] * 10
    assert all(bits(got[k]).tobytes() == bits(prior[k]).tobytes() for k in prior)
    nan = dict(s["general"], xy1=s["general"]["xy1"].copy())                # a NaN in an UNMATCHED keypoint: Normalize spreads it, no score is > 0
    nan["xy1"][int(np.nonzero(nan["m12"] < 0)[0][0]), 0] = np.nan
    got = host(nan)
    G.assert_equals_rule(got, G.rule_of(nan), 0)
    assert got["header"][0, 1] == R.BOTH_ZERO
    hostile = dict(s["general"])
    m = hostile["m12"].copy(); m[3], m[4], m[5], m[6] = 515, -7, 2 ** 31 - 1, m[7]
    dd = hostile["draws"].copy(); dd[2] = -5; dd[3, ::2] = 2 ** 31 - 1
    hostile.update(m12=m, draws=dd)
    G.assert_equals_rule(host(hostile), G.rule_of(hostile), 0)


def test_refusals_without_a_device_and_kernel_names():
    L = capi.lib()
    cam = G.camera()
    a = np.zeros(4096, np.float64)
    p = a.ctypes.data

    def hostcall(B=1, n1=8, n2=8, iters=2, sigma=1.0, stride=0, rand_max=7, mpc=0.9998, mt=50, cam_=cam, bad=None, off=0):
        ptrs = [p] * 12
        if bad is not None:
            ptrs[bad] = None if off == 0 else p + off
        return L.xfh_two_view_host(B, n1, n2, ptrs[0], ptrs[1], ptrs[2], None if cam_ is None else C.byref(cam_), sigma, iters, ptrs[3], stride, rand_max, mpc, mt,
                                   *ptrs[4:])
    bad = [hostcall(B=0), hostcall(n1=0), hostcall(n1=capi.GRID_MAX_N + 1), hostcall(n2=0), hostcall(iters=0), hostcall(iters=capi.TWO_VIEW_MAX_ITERS + 1),
           hostcall(sigma=0.0), hostcall(sigma=-1.0), hostcall(sigma=float("nan")), hostcall(rand_max=0), hostcall(mpc=float("inf")), hostcall(mt=-1),
           hostcall(cam_=None), hostcall(B=2, stride=8)]
    bad += [hostcall(bad=k) for k in range(12)] + [hostcall(bad=k, off=2) for k in (0, 1, 2, 3, 5, 6, 10, 11)] + [hostcall(bad=4, off=8)]
    assert all(rc == 1 for rc in bad), bad
    assert hostcall() == 0
    assert L.xfh_two_view_device(None, 1, 8, 8, p, p, p, C.byref(cam), 1.0, 2, p, 0, 7, 0.9998, 50, *([p] * 8)) == 1
    assert L.xfh_two_view(None, 8, 8, p, p, p, C.byref(cam), 1.0, 2, p, 7, 0.9998, 50, *([p] * 7)) == 1
    assert L.xfh_two_view_set(None, 7, 8, p) == 1 and L.xfh_two_view_set(p, 0, 8, p) == 1 and L.xfh_two_view_set(p, 7, 7, p) == 1
    assert L.xfh_two_view_fit(0, p, p, p) == 1 and L.xfh_two_view_fit(3, p, p, p) == 1 and L.xfh_two_view_fit(1, None, p, p) == 1
    assert L.xfh_two_view_score(0, p, 1.0, p, p, p, p, p) == 1 and L.xfh_two_view_score(1, p, 0.0, p, p, p, p, p) == 1 and L.xfh_two_view_score(1, p, 1.0, p, None, p, p, p) == 1
    assert L.xfh_two_view_check_rt(None, p, 1.0, p, p, p, p, p) == 1 and L.xfh_two_view_check_rt(C.byref(cam), p, float("nan"), p, p, p, p, p) == 1
    assert L.xfh_two_view_workspace_bytes(0, 8, 2, 1) == 0 and L.xfh_two_view_workspace_bytes(8, 8, 2, 1) % 16 == 0
    names = [L.xfh_kernel_name(capi.K[k]) for k in ("TWOVIEW_PREPARE", "TWOVIEW_FIT", "TWOVIEW_SCORE", "TWOVIEW_SELECT", "TWOVIEW_CHECK_RT", "TWOVIEW_FINAL")]
    assert names == [b"k_twoview_prepare", b"k_twoview_fit", b"k_twoview_score", b"k_twoview_select", b"k_twoview_check_rt", b"k_twoview_final"]
    assert capi.K["TWOVIEW_PREPARE"] == 39 and L.xfh_kernel_name(38) == b"k_triangulate_finish"      # existing ids keep their values


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("twoview") / "asan_twoview_test")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "xfeatslam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "asan_twoview_test.cpp"), "-o", exe])
    return exe


def test_rule_under_sanitizers_on_hostile_inputs(asan_exe):
    """a stand-alone program built from this repository's header alone with AddressSanitizer + UBSan: nothing of the library is linked, nothing
    runs on a GPU, nothing is loaded into Python"""
    r = subprocess.run([asan_exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "asan_twoview_test ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


def test_rule_under_sanitizers_equals_the_python_rule(asan_exe, tmp_path, scenes):
    s, want = scenes
    for n, sc in s.items():
        n1, n2, iters = len(sc["xy1"]), len(sc["xy2"]), len(sc["draws"])
        with open(tmp_path / "in.bin", "wb") as f:
            f.write(struct.pack("<5i5fd", n1, n2, iters, G.RAND_MAX, 50, *[float(c) for c in sc.get("cam", G.CAM)], float(sc["sigma"]), R.DEFAULT_COS))
            for a, dt in ((sc["xy1"], F), (sc["xy2"], F), (sc["m12"], np.int32), (sc["draws"], np.int32)):
                f.write(np.ascontiguousarray(a, dt).tobytes())
        r = subprocess.run([asan_exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert r.returncode == 0, (n, r.stdout[-1000:], r.stderr[-3000:])
        w = want[n]
        blob = b"".join(np.ascontiguousarray(np.asarray(w[k], G.OUT_DTYPES[k])).tobytes() for k in R.OUTPUTS)
        assert open(tmp_path / "out.bin", "rb").read() == blob, n
