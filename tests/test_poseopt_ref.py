"""The two restatements of PoseOptimization (tests/ref_poseopt.py: the literal transcription and the kernel's rule) against each other on the rig
and on random small scenes, the host lines of the library (xfh_pose_edge, _oplus, _solve, _from_tcw, _to_tcw) against both and against a central
difference, hand-made cases whose answers are written out, every class of refusal, the condition of the rig's scenes, and the C lines -- the
state machine and the fold of k_pose_optimize run by one host thread, under AddressSanitizer + UBSan -- against the rule bit by bit.  No GPU.

Two kinds of scene, two comparisons.  SCENES and EDGE_SCENES hold the 1e-9 condition (test_rig_condition: every decision of the Levenberg loop stays
that far from its decision point), so two correct evaluations walk the same trajectory and everything is compared, the header's counts included.
Stereo edges keep such scenes conditioned: cam_project's float invz makes the cost a staircase whose steps (1e-5) dwarf rounding noise.  All-mono
scenes of ten or more edges that converge never hold that condition (the unrobustified round converges quadratically into rounding noise, where rho is
noise / 1e-3 and its sign is chance), but their OUTPUTS are determined all the same: MONO_SCENES hold a condition on the classifications and the pivots
only (test_mono_scene_condition) and are compared through ref_poseopt.outputs_agree, which leaves the trajectory out, within R.MONO_TOL -- the spread
of the float64 forms among themselves, a libm that is off by an ulp included (test_mono_spread_of_the_reference).

What the rig could NOT be given: a scene in which the stale-error rule changes a flag or a float chi2.  A round's last trial is rejected only when ten
trials in a row fail or rho == 0, and both happen only at convergence, where the rejected estimate differs from the restored one by less than the
outputs resolve (test_rig_condition prints the count; the rule itself is exercised: rounds of the rig end on ten rejected trials)."""
import ctypes as C
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import poseopt_rig as R
import ref_poseopt as RP
from xfeatslam_amd import capi

F, D = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-9
DP = C.POINTER(C.c_double)


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    import __graft_entry__ as g
    if not os.path.exists(capi.LIB_PATH):
        g.build()


@pytest.fixture(scope="module")
def models():
    """both forms of every rig scene that is compared exactly, computed once"""
    return {n: (R.model(R.scene(n), RP.literal), R.model(R.scene(n), RP.rule)) for n in list(R.SCENES) + list(R.EDGE_SCENES)}


@pytest.fixture(scope="module")
def mono_models():
    """both forms of the all-mono scenes, computed once"""
    return {n: (R.model(R.scene(n), RP.literal), R.model(R.scene(n), RP.rule)) for n in R.MONO_SCENES}


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def lib_edge(pose, X, xy, ur, w, robust, cam=None):
    L = capi.lib()
    p = np.array(pose, D); Xf = np.array(X, F); xf = np.array(xy, F)
    e, c, J, r1 = np.zeros(3, D), np.zeros(1, D), np.zeros(18, D), np.zeros(1, D)
    cs = R.cam_struct()
    if cam is not None:
        cs.fx, cs.fy, cs.cx, cs.cy, cs.bf = cam
    assert L.xfh_pose_edge(_ptr(p), C.byref(cs), _ptr(Xf), _ptr(xf), float(ur), float(w), int(robust), _ptr(e), _ptr(c), _ptr(J), _ptr(r1)) == 0
    return e, float(c[0]), J, float(r1[0])


def lib_oplus(pose, u):
    p, uu, o = np.array(pose, D), np.array(u, D), np.zeros(7, D)
    assert capi.lib().xfh_pose_oplus(_ptr(p), _ptr(uu), _ptr(o)) == 0
    return o


def test_the_two_forms_agree_on_the_rig(models):
    for n, (a, b) in models.items():
        assert RP.same_decisions(a, b) == [], (n, RP.same_decisions(a, b))
        assert RP.ulps(a["Tcw_out"], b["Tcw_out"]).max() <= 1 and RP.ulps(a["chi2"], b["chi2"]).max() <= 1, n
        assert abs(a["final_chi2"] - b["final_chi2"]) <= 1e-9 * max(1.0, abs(a["final_chi2"])), n


def test_the_two_forms_agree_on_200_random_small_scenes():
    """scenes drawn from one seeded stream; those whose literal form holds the condition are compared until 200 have been (the others are counted)"""
    kept = dropped = 0
    seed = 1000
    while kept < 200:
        rng = np.random.RandomState(seed)
        kind = ["mono", "stereo", "mixed", "mono_ur"][seed % 4]
        n = int(rng.randint(3, 10)) if kind.startswith("mono") else int(rng.randint(3, 40))
        s = R.make(seed, n, int(rng.randint(n + 3, 3 * n + 10)), kind=kind, outliers=float(rng.choice([0.0, 0.2])), noise=float(rng.choice([0.7, 3.0])),
                   start=(float(rng.choice([0.02, 0.2])), float(rng.choice([0.05, 0.5]))), beyond=int(rng.randint(0, 3)))
        seed += 1
        a = R.model(s, RP.literal)
        if min(a["margins"].values()) <= MARGIN:
            dropped += 1
            continue
        b = R.model(s, RP.rule)
        assert RP.same_decisions(a, b) == [], (seed - 1, RP.same_decisions(a, b))
        assert RP.ulps(a["Tcw_out"], b["Tcw_out"]).max() <= 1 and RP.ulps(a["chi2"], b["chi2"]).max() <= 1
        kept += 1
    print(f"{kept} scenes compared, {dropped} dropped for a decision within {MARGIN} of its point")
    assert dropped < 400


def test_pose_lines_against_the_restatement():
    L = capi.lib()
    rng = np.random.RandomState(5)
    for it in range(200):
        u0 = np.r_[rng.uniform(-3, 3, 3), rng.uniform(-2, 2, 3)]
        p = RP.oplus(u0, [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
        T = RP.to_tcw(p)
        back, p2 = np.zeros(12, F), np.zeros(7, D)
        assert L.xfh_pose_to_tcw(_ptr(np.array(p, D)), _ptr(back)) == 0 and back.tobytes() == T.tobytes()
        assert L.xfh_pose_from_tcw(_ptr(T), _ptr(p2)) == 0 and p2.tolist() == RP.from_tcw(T)
        u = np.r_[rng.randn(3), rng.randn(3)] * (1e-7 if it % 5 == 0 else 0.3)          # both branches of exp
        assert lib_oplus(p, u).tolist() == RP.oplus(u, p), it
    # the solve against the restatement, and against numpy
    for it in range(100):
        A = rng.randn(8, 6); Hm = A.T @ A
        H21 = np.array([Hm[i, j] for i in range(6) for j in range(i, 6)], D); b = rng.randn(6); x = np.zeros(6, D)
        lam = float(rng.choice([0.0, 1e-3, 10.0]))
        ok = L.xfh_pose_solve(_ptr(H21), lam, _ptr(b), _ptr(x))
        ok2, x2, piv = RP.ldlt_solve(H21, lam, b, [0.0] * 6)
        assert ok == 1 and ok2 and x.tolist() == x2 and np.allclose(x, np.linalg.solve(Hm + lam * np.eye(6), b), rtol=1e-8, atol=1e-10)


def test_pose_edge_against_both_forms_and_a_central_difference():
    """error, chi2, Jacobian and rho[1] equal the restatement's bit for bit; the Jacobian agrees with (e(+h) - e(-h)) / 2h along every twist axis.
    Bound: e = obs - fx x / z (and u - bf / z).  Along a unit twist the camera-frame point moves with speed <= s = max(|pc|, 1), and every
    derivative of x / z in that motion brings one more factor s / z and its order, so the k-th derivative is bounded by M_k = k! fx (s / z)^(k + 1)
    (bf / z: the same with bf / s for fx; both added).  The central difference is off by at most h^2 M_3 / 6 from truncation, by 2 eps E / 2h from
    rounding of errors of size E = |obs| + |projection|, and for a stereo edge by Q / h, Q = 2^-24 (|u - cx| + bf / z + |v - cy|) 2, the step of the
    float invz in cam_project.  h = 1e-5 (mono) balances the first two near 1e-7; h = 1e-3 (stereo) balances truncation and the float step."""
    cam = RP.cam_of(R.CAM)
    fx, fy, cx, cy, bf = cam
    rng = np.random.RandomState(9)
    eps = float(np.finfo(D).eps)
    worst = 0.0
    for it in range(300):
        p = RP.oplus(np.r_[rng.uniform(-0.5, 0.5, 3), rng.uniform(-1, 1, 3)], [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
        stereo = it % 2 == 1
        Xc = np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(1.0, 8.0)])
        inv = RP.normalize([-p[0], -p[1], -p[2], p[3]])
        X = np.array(RP.rotate(inv, list(Xc - np.array(p[4:7]))), D).astype(F)
        xy = np.array([rng.uniform(0, 640), rng.uniform(0, 480)], F)
        ur = F(rng.uniform(0, 600)) if stereo else F(-1.0)
        w = float(F(rng.choice([1.0, 0.694, 1.44])))
        for robust in (0, 1):
            e, c, J, r1 = lib_edge(p, X, xy, ur, w, robust)
            Xd, od, sa = X.astype(D).reshape(1, 3), np.array([[xy[0], xy[1], ur]], D), np.array([stereo])
            pc, e2, c2 = RP.edge_error(p, cam, Xd, od, sa, w)
            J2 = RP.edge_jacobian(cam, pc, sa)
            want_r1 = float(RP.huber(c2, sa)[1][0]) if robust else 1.0
            assert [float(v[0]) for v in e2] == e.tolist() and float(c2[0]) == c and [float(v[0]) for v in J2] == J.tolist() and want_r1 == r1, it
        pcv = np.array([float(v[0]) for v in pc])
        z, s = pcv[2], max(float(np.linalg.norm(pcv)), 1.0)
        h = 1e-3 if stereo else 1e-5
        M3 = 6.0 * (max(fx, fy) + (bf / s if stereo else 0.0)) * (s / z) ** 4
        E = 2.0 * (640.0 + 600.0 + max(fx, fy) * s / z)
        Q = 2.0 ** -24 * 2.0 * (abs(fx * pcv[0] / z) + abs(fy * pcv[1] / z) + bf / z) if stereo else 0.0
        bound = h * h * M3 / 6.0 + eps * E / h + Q / h
        for d in range(6):
            u = np.zeros(6); u[d] = h
            ep = lib_edge(lib_oplus(p, u), X, xy, ur, w, 0)[0]
            em = lib_edge(lib_oplus(p, -u), X, xy, ur, w, 0)[0]
            fd = (ep - em) / (2.0 * h)
            err = np.abs(fd - J.reshape(3, 6)[:, d]).max()
            worst = max(worst, err / bound)
            assert err <= bound, (it, d, err, bound)
    print(f"central difference: worst error / bound {worst:.3f}")
    assert 1e-4 < worst                                                   # the bound is not vacuous


# ---- hand-made cases: identity pose, fx = fy = 512, points whose projection is exact in binary ---------------------------------------------------
EXACT_CAM = (512.0, 512.0, 320.0, 240.0, 32.0)


def exact_scene(shift=None):
    pts = np.array([[x, y, z] for z in (2.0, 4.0) for x in (-0.5, 0.25, 0.75) for y in (-0.25, 0.5)], F)      # 12 points
    xy = np.stack([512.0 * pts[:, 0] / pts[:, 2] + 320.0, 512.0 * pts[:, 1] / pts[:, 2] + 240.0], 1).astype(F)
    if shift is not None:
        xy[shift] += F(50.0)
    T = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F)
    return dict(Tcw=T, xy_un=xy, uright=None, assigned=np.arange(12, dtype=np.int32), points=pts, nt=12, nq=12)


@pytest.mark.parametrize("form", [RP.literal, RP.rule])
def test_hand_made_cases(form):
    s = exact_scene()
    r = form(s["Tcw"], EXACT_CAM, s["xy_un"], None, s["assigned"], s["points"], 1.0)
    # zero noise at the true pose: b = 0, x = 0, the trial changes nothing, rho == 0 ends every round after one rejected trial
    assert r["header"].tolist() == [12, 0, 12, 4, 4, 4, 4, 0] and r["reasons"] == ["rho0"] * 4
    assert not r["outlier"].any() and not r["chi2"].any() and r["Tcw_out"].tobytes() == s["Tcw"].tobytes() and r["final_chi2"] == 0.0
    # one observation moved by 50 pixels in x and y: flagged, alone, in every round; the pose moves by less than the other edges' threshold
    s = exact_scene(shift=7)
    r = form(s["Tcw"], EXACT_CAM, s["xy_un"], None, s["assigned"], s["points"], 1.0)
    assert r["outlier"].tolist() == [0] * 7 + [1] + [0] * 4 and r["header"][:4].tolist() == [12, 1, 11, 4]
    assert all(h.tolist() == r["outlier"].tolist() for h in r["history"])
    assert r["chi2"][7] > 1000.0 and r["chi2"][np.arange(12) != 7].max() < 5.991
    assert np.abs(r["Tcw_out"] - s["Tcw"]).max() < 1e-3                   # after the last round (no outlier, no kernel) the pose is back at the truth
    # fewer than 3 edges: refused, the pose untouched; fewer than 10: one round
    s = exact_scene()
    a = s["assigned"].copy(); a[2:] = -1
    r = form(s["Tcw"], EXACT_CAM, s["xy_un"], None, a, s["points"], 1.0)
    assert r["header"].tolist() == [2, 0, 0, 0, 0, 0, 0, 0] and r["Tcw_out"].tobytes() == s["Tcw"].tobytes() and not r["outlier"].any()
    a = s["assigned"].copy(); a[9:] = 12                                  # an entry >= nq is no edge
    r = form(s["Tcw"], EXACT_CAM, s["xy_un"], None, a, s["points"], 1.0)
    assert r["header"].tolist() == [9, 0, 9, 1, 1, 1, 1, 0]


def test_every_class_of_refusal():
    """before any launch, so before the ctx is touched: a ctx that cannot be dereferenced shows that each check is there"""
    L = capi.lib()
    ctx, p, cam = C.c_void_p(4096), C.c_void_p(1 << 20), C.byref(R.cam_struct())
    odd, odd8 = C.c_void_p((1 << 20) + 2), C.c_void_p((1 << 20) + 4)

    def dev(B=1, nt=8, nq=8, T=p, cm=cam, xy=p, ur=None, a=p, pts=p, w=1.0, ws=p, To=p, o=p, c=p, h=p, fc=p, cx=ctx):
        return L.xfh_pose_optimize_device(cx, B, nt, nq, T, cm, xy, ur, a, pts, w, ws, To, o, c, h, fc)

    def host(nt=8, nq=8, T=p, cm=cam, xy=p, a=p, pts=p, w=1.0, To=p, o=p, c=p, h=p, fc=p, cx=ctx):
        return L.xfh_pose_optimize(cx, nt, nq, T, cm, xy, None, a, pts, w, To, o, c, h, fc)

    big = capi.GRID_MAX_N + 1
    for kw in (dict(cx=None), dict(B=0), dict(B=-1), dict(B=65536), dict(nt=0), dict(nt=big), dict(nq=0), dict(nq=big),
               dict(T=None), dict(cm=None), dict(xy=None), dict(a=None), dict(pts=None), dict(ws=None), dict(To=None), dict(o=None), dict(c=None), dict(h=None), dict(fc=None),
               dict(T=odd), dict(xy=odd), dict(ur=odd), dict(a=odd), dict(pts=odd), dict(To=odd), dict(c=odd), dict(h=odd), dict(ws=odd8), dict(fc=odd8),
               dict(w=0.0), dict(w=-1.0), dict(w=float("nan")), dict(w=float("inf"))):
        assert dev(**kw) == 1, kw
    for kw in (dict(cx=None), dict(nt=0), dict(nt=big), dict(nq=0), dict(nq=big), dict(T=None), dict(cm=None), dict(xy=None), dict(a=None), dict(pts=None),
               dict(To=None), dict(o=None), dict(c=None), dict(h=None), dict(fc=None), dict(w=0.0), dict(w=float("nan")), dict(w=float("inf"))):
        assert host(**kw) == 1, kw
    assert L.xfh_pose_edge(None, cam, p, p, -1.0, 1.0, 1, None, None, None, None) == 1 and L.xfh_pose_from_tcw(None, p) == 1
    assert L.xfh_pose_optimize_workspace_bytes(100, 2) == 2 * L.xfh_pose_optimize_workspace_bytes(100, 1) > 0
    assert all(L.xfh_pose_optimize_workspace_bytes(*a) == 0 for a in ((0, 1), (big, 1), (8, 0), (8, 65536)))
    assert L.xfh_kernel_name(capi.K["POSE_OPTIMIZE"]) == b"k_pose_optimize" and capi.K["POSE_OPTIMIZE"] == 35
    assert L.xfh_kernel_name(34) == b"k_bowdb_select" and L.xfh_kernel_name(30) == b"?"                 # existing ids keep their values


def test_rig_condition(models):
    """every scene the GPU tests compare: each classification's chi2 against its cut, each rho against 0, each (iniChi - currentChi) * 1e3 against
    iniChi and each LDL^T pivot against 0 stay farther than 1e-9 (relative) from the decision point, on the literal form; and the scenes show what
    they are in the rig for"""
    stale_visible = 0
    for n, (a, _) in models.items():
        print(n, a["header"].tolist(), a["reasons"], {k: f"{v:.1e}" for k, v in a["margins"].items()})
        assert min(a["margins"].values()) > MARGIN, (n, a["margins"])
        s = R.scene(n)
        fresh = RP.literal(s["Tcw"], R.CAM, s["xy_un"], s["uright"], s["assigned"], s["points"], s["w"], stale=False)
        stale_visible += int((fresh["outlier"] != a["outlier"]).sum() + (fresh["chi2"].view(np.int32) != a["chi2"].view(np.int32)).sum())
    print(f"outputs that the stale-error rule changes, over the rig: {stale_visible}")
    lit = {n: m[0] for n, m in models.items()}
    assert sorted(int(m["header"][0]) for m in lit.values())[:6] == [2, 3, 9, 9, 10, 12] and {63, 64, 65, 257, 1000} <= {int(m["header"][0]) for m in lit.values()}
    assert lit["n2"]["header"].tolist() == [2, 0, 0, 0, 0, 0, 0, 0] and lit["n9_mono"]["header"][3] == 1 and lit["n10"]["header"][3] == 4
    h = lit["n63_mono_far"]["history"]                                    # flagged after round 1, an inlier again at the end
    assert int((h[0].astype(bool) & ~h[3].astype(bool)).sum()) >= 1 and lit["n63_mono_far"]["reasons"] == ["iterations"] * 4
    lost = lit["n63_mono_lost"]                                           # trials rejected far from rho = 0, then rounds with no level-0 edge
    assert lost["header"][6] >= 3 and lost["margins"]["rho"] > 1e-2 and lost["reasons"][1:] == ["noactive"] * 3 and lost["header"][1] == 63
    assert lit["n64_stereo"]["reasons"][0] == "qmax" and "three" in lit["n64_stereo"]["reasons"]        # a round whose last (tenth) trial is rejected
    assert any(e[0] == "trial" and not e[4] for e in lit["far_stereo"]["events"])
    s = R.scene("n65_mixed")
    assert int((s["assigned"] >= s["nq"]).sum()) == 6 and lit["n65_mixed"]["header"][0] == 65
    assert lit["identical"]["header"][7] == 0 and lit["identical"]["margins"]["pivot"] < 1e-3         # rank-deficient, yet no pivot fails: lambda > 0
    assert all(m["header"][7] == 0 for m in lit.values())
    # the scenes at the sizes where the kernel instance changes: conditioned in the rule's form too, the pinned keypoints carry edges, and the
    # last keypoint, the last partial stride of 256 and both sides of 1024 / 4096 are among them
    assert sorted(kw["nt"] for kw in R.EDGE_SCENES.values()) == [1024, 1025, 4096, 4097, capi.GRID_MAX_N]
    for n, kw in R.EDGE_SCENES.items():
        s, nt = R.scene(n), kw["nt"]
        assert min(models[n][1]["margins"].values()) > MARGIN, (n, models[n][1]["margins"])
        assert kw["kind"] in ("stereo", "mixed") and 200 <= kw["n_edges"] <= 400 and int(lit[n]["header"][0]) == kw["n_edges"]
        want = {0, 255, 256, nt - 257, nt - 256, nt - 1} | {k for k in (1023, 1024, 4095, 4096) if k < nt}
        assert kw["pin"] == want and all(0 <= s["assigned"][k] < s["nq"] for k in want), n
        assert (s["uright"] >= 0).any()


def test_mono_scene_condition(mono_models):
    """the all-mono scenes the GPU tests compare through outputs_agree: ten or more edges, no stereo edge, and in BOTH forms every classification
    stays farther than 1e-4 (relative) from its cut and every pivot farther than 1e-9 from 0, no solve fails; and each is a scene the 1e-9 condition
    of test_rig_condition excludes (a rho within 1e-9 of 0 in at least one form), which is why it is here.  1e-4 is a condition, not a measurement:
    rounding noise on a chi2 is near 1e-13 relative, so no evaluation in doubles, whatever its order or libm, moves a classification."""
    kinds = set()
    for n, (a, b) in mono_models.items():
        s, kw = R.scene(n), R.MONO_SCENES[n]
        print(n, a["header"].tolist(), b["header"].tolist(), a["reasons"], {k: f"{v:.1e}" for k, v in a["margins"].items()}, {k: f"{v:.1e}" for k, v in b["margins"].items()})
        assert a["header"][0] == kw["n_edges"] >= 10 and (s["uright"] is None or not (s["uright"] >= 0).any())
        for m in (a, b):
            assert m["margins"]["classify"] > 1e-4 and m["margins"]["pivot"] > MARGIN and m["header"][7] == 0 and m["header"][3] == 4, (n, m["margins"])
        assert min(a["margins"]["rho"], b["margins"]["rho"]) <= MARGIN, n
        assert all(0 <= s["assigned"][k] < s["nq"] for k in kw.get("pin", ())), n
        kinds.add((s["uright"] is None, kw.get("outliers", 0.0) > 0, 0 if kw["nt"] <= 1024 else 1 if kw["nt"] <= 4096 else 2))
    assert {(True, i) for i in range(3)} <= {(k[0], k[2]) for k in kinds}                              # every instance meets a null uright
    assert {k[0] for k in kinds} == {True, False} and {k[1] for k in kinds} == {True, False}
    assert any(int(b["header"][1]) > 0 for _, b in mono_models.values())


def _spread(results):
    """largest disagreement among results of one scene: (pose steps, chi2 steps, final_chi2 relative, the chi2 that is that many steps off); flags
    and header[0:4] must be equal"""
    pose = chi = 0
    fin = at = 0.0
    for i, a in enumerate(results):
        assert np.array_equal(a["outlier"], results[0]["outlier"]) and np.array_equal(a["header"][:4], results[0]["header"][:4]), (i, a["header"], results[0]["header"])
        assert RP.header_in_bounds(a["header"])
        for b in results[:i]:
            pose = max(pose, int(RP.ulps(a["Tcw_out"], b["Tcw_out"]).max()))
            uc = RP.ulps(a["chi2"], b["chi2"])
            if uc.max() > chi:
                chi, at = int(uc.max()), float(a["chi2"][uc.argmax()])
            fin = max(fin, RP.final_rel(a, b))
    return pose, chi, fin, at


JITTER_SEEDS = (11, 12, 13)


def test_mono_spread_of_the_reference(mono_models):
    """where R.MONO_TOL comes from: how far the float64 forms lie apart on all-mono scenes -- the literal form, the rule, and the rule with three
    libm jitters (every sqrt / sin / cos moved by up to one double ulp) -- over MONO_SCENES and 200 all-mono scenes of 10 .. 1000 edges drawn from
    one seeded stream that hold the condition of test_mono_scene_condition (the others are counted; at most half may be dropped).  Flags and
    header[0:4] are equal throughout.  The tolerance is twice the largest value seen, at least one float32 step (1e-13 for final_chi2): twice for the
    finite sample; what the device may vary (its libm, the rule's fold) is part of what these forms vary (libm and the whole summation order).
    The constants are held to that here, so they cannot go stale; nothing from the device enters them."""
    forms = [functools.partial(RP.rule, libm_jitter=j) for j in JITTER_SEEDS]
    worst = [0, 0, 0.0]
    for n, (a, b) in mono_models.items():
        sp = _spread([a, b] + [R.model(R.scene(n), f) for f in forms])
        print(f"{n}: pose {sp[0]}, chi2 {sp[1]} float steps (at a chi2 of {sp[3]:.3g}), final_chi2 {sp[2]:.1e}; trials literal {a['header'][5]}, rule {b['header'][5]}")
        worst = [max(w, v) for w, v in zip(worst, sp)]
    kept = dropped = excluded = 0
    seed = 5000
    stream, at = [0, 0, 0.0], (0.0, 0)
    while kept < 200:
        rng = np.random.RandomState(seed)
        n = int(round(10 ** rng.uniform(1.0, 3.0)))
        s = R.make(seed, n, n + int(rng.randint(3, 3 * n + 10)), kind=["mono", "mono_ur"][seed % 2], outliers=float(rng.choice([0.0, 0.2])),
                   noise=float(rng.choice([0.5, 1.0])), beyond=int(rng.randint(0, 3)))
        seed += 1
        a, b = R.model(s, RP.literal), R.model(s, RP.rule)
        if not all(m["margins"]["classify"] > 1e-4 and m["margins"]["pivot"] > MARGIN and m["header"][7] == 0 for m in (a, b)):
            dropped += 1
            assert dropped <= 200, "more than half of the stream does not hold the condition"
            continue
        excluded += min(a["margins"]["rho"], b["margins"]["rho"]) <= MARGIN
        try:
            sp = _spread([a, b] + [R.model(s, f) for f in forms])
        except AssertionError as e:
            raise AssertionError(f"stream scene of seed {seed - 1} ({n} edges): {e}")
        at = (sp[3], n) if sp[1] > stream[1] else at
        stream = [max(w, v) for w, v in zip(stream, sp)]
        kept += 1
    print(f"stream: {kept} scenes compared, {dropped} dropped, {excluded} of the compared ones excluded by the 1e-9 condition; "
          f"pose {stream[0]}, chi2 {stream[1]} float steps (at a chi2 of {at[0]:.3g}, a scene of {at[1]} edges), final_chi2 {stream[2]:.1e}")
    worst = [max(w, v) for w, v in zip(worst, stream)]
    need = RP.Tol(pose=max(1, 2 * worst[0]), chi2=max(1, 2 * worst[1]), final=max(1e-13, 2.0 * worst[2]))
    print(f"largest seen: pose {worst[0]}, chi2 {worst[1]} float steps, final_chi2 {worst[2]:.2e} -> {need}; MONO_TOL {R.MONO_TOL}")
    assert need.pose <= R.MONO_TOL.pose and need.chi2 <= R.MONO_TOL.chi2 and need.final <= R.MONO_TOL.final
    assert excluded >= 100                                                # the stream is of the kind the tolerance is for


def test_outputs_agree_has_teeth(mono_models):
    """one pose entry one step too far, one flag, one chi2 of the input pose, n_bad, the number of rounds, a header count out of bounds: each is
    reported, and alone; an unchanged result and the two forms of every mono scene are not"""
    name, tol = "m100_neg_out", R.MONO_TOL
    s, m = R.scene(name), mono_models[name][1]
    copy = lambda: dict(m, Tcw_out=m["Tcw_out"].copy(), outlier=m["outlier"].copy(), chi2=m["chi2"].copy(), header=m["header"].copy())
    assert RP.outputs_agree(copy(), m, tol) == []
    assert all(RP.outputs_agree(a, b, tol) == [] for a, b in mono_models.values())
    idx, X, obs, st = RP.edges_of(s["xy_un"], s["uright"], s["assigned"], s["points"])
    at_input = RP.edge_error(RP.from_tcw(s["Tcw"]), RP.cam_of(R.CAM), X, obs, st, float(F(R.INV_SIGMA2)))[2].astype(F)
    e = int(np.argmin(RP.ulps(at_input, m["chi2"][idx])))                # the edge whose chi2 the optimisation changed least: still far more than tol
    assert RP.ulps(at_input[e], m["chi2"][idx[e]]) > 100 * tol.chi2
    k = int(idx[0])

    def pose(r):
        for _ in range(tol.pose + 1):
            r["Tcw_out"][7] = np.nextafter(r["Tcw_out"][7], F(np.inf))

    def flag(r): r["outlier"][k] ^= 1
    def chi(r): r["chi2"][idx[e]] = at_input[e]
    def n_bad(r): r["header"][1] += 1
    def rounds(r): r["header"][3] = 3
    def trials(r): r["header"][5] = 401
    def final(r): r["final_chi2"] = m["final_chi2"] * (1.0 + 2.0 * tol.final)

    for mutate, word in ((pose, "Tcw_out"), (flag, "outlier"), (chi, "chi2 "), (n_bad, "header[0:4]"), (rounds, "header[0:4]"), (trials, "header[4:8]"), (final, "final_chi2")):
        r = copy()
        mutate(r)
        bad = RP.outputs_agree(r, m, tol)
        assert len(bad) == 1 and bad[0].startswith(word), (mutate.__name__, bad)
        assert RP.outputs_agree(m, r, tol) != []
    r = copy()                                                            # at the tolerance itself: not reported
    for _ in range(tol.pose):
        r["Tcw_out"][7] = np.nextafter(r["Tcw_out"][7], F(np.inf))
    assert RP.outputs_agree(r, m, tol) == []


def _asan_exe(tmp_path_factory):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "xfeatslam_amd", "csrc"), "asan", "-s", "-j8"])
    exe = str(tmp_path_factory.mktemp("poseopt") / "asan_poseopt_test")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "xfeatslam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "asan_poseopt_test.cpp"),
                           "-L" + os.path.join(ROOT, "xfeatslam_amd"), "-lxfeat_hip_asan", "-Wl,-rpath," + os.path.join(ROOT, "xfeatslam_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    return exe


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    return _asan_exe(tmp_path_factory)


def test_header_helper_under_sanitizers(asan_exe):
    """a stand-alone program built with AddressSanitizer + UBSan against the sanitizer build of the HOST code (device code is not instrumented,
    nothing runs on a GPU, nothing is loaded into Python)"""
    r = subprocess.run([asan_exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "asan_poseopt_test ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


WEIGHTED = [n for n, kw in R.SCENES.items() if "w" in kw]


@pytest.mark.parametrize("name", ["n2", "n9_mixed", "n63_mono_lost", "n64_stereo", "n65_mixed", "n257", "identical", "big"] + WEIGHTED + list(R.EDGE_SCENES) + list(R.MONO_SCENES))
def test_the_kernels_loop_on_the_host_equals_the_rule(asan_exe, tmp_path, models, mono_models, name):
    """the state machine, the per-edge lines and the fold of k_pose_optimize, run by one thread of the sanitizer program: every output byte equals
    the rule's (the host's libm is the restatement's, so here even the doubles agree) -- on the all-mono scenes too, whose trajectory is decided in
    rounding noise: same fold, same libm, same noise"""
    models = dict(models, **mono_models)
    s = R.scene(name)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<3i", s["nt"], s["nq"], int(s["uright"] is not None)) + s["Tcw"].astype(F).tobytes() + np.array(R.CAM, F).tobytes() + struct.pack("<f", s["w"]))
        f.write(s["xy_un"].tobytes() + (s["uright"].tobytes() if s["uright"] is not None else b"") + s["assigned"].tobytes() + s["points"].tobytes())
    r = subprocess.run([asan_exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    m = models[name][1]
    want = m["Tcw_out"].tobytes() + m["outlier"].tobytes() + m["chi2"].tobytes() + m["header"].tobytes() + struct.pack("<d", m["final_chi2"])
    got = open(tmp_path / "out.bin", "rb").read()
    assert got == want, (name, np.frombuffer(got[-40:-8], np.int32), m["header"])
