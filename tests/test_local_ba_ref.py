"""xfh_local_ba_host and the piece entry points (xfh_lba_edge, _point_block, _solve) against the Python rule (tests/ref_local_ba.py): the host form by
bits on the rig and on 200 random small scenes, every piece against the rule and against an independent statement (central differences, numpy.linalg),
a hand-made one-step case solved as ONE dense system without the Schur complement, every class of refusal, both early statuses, the scenes in which every
factorisation fails (a NaN) or none does although b is NaN (an Inf) with their written-out headers, the sanitizer program,
and the condition the rig's scenes must hold for the GPU comparison to be a fair one.  CPU only."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import local_ba_rig as G
import ref_local_ba as R
import ref_poseopt as RP
from xfeatslam_amd import capi, local_ba

D, F = np.float64, np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
OUT = ("Tcw_out", "points_out", "erase", "chi2", "header")


def bits_equal(a, b):
    bad = [k for k in OUT if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()]
    if struct.pack("d", a["final_chi2"]) != struct.pack("d", b["final_chi2"]):
        bad.append("final_chi2")
    return bad


@pytest.mark.parametrize("name", list(G.SCENES) + list(G.EARLY) + list(G.LIMIT))
def test_host_form_equals_the_rule_by_bits(name):
    assert bits_equal(G.host_of(name), G.rule_of(name)) == []


def nan_matched(a, b):
    """bits_equal where neither holds a NaN; a NaN for a NaN, whatever its bits (numpy's and the C++ default NaN differ in sign)"""
    bad = []
    for k in OUT + ("final_chi2",):
        x, y = np.atleast_1d(np.asarray(a[k])), np.atleast_1d(np.asarray(b[k]))
        if x.dtype.kind != "f":
            if x.tobytes() != y.tobytes():
                bad.append(k)
            continue
        nx, ny = np.isnan(x), np.isnan(y)
        if not np.array_equal(nx, ny) or x[~nx].tobytes() != y[~ny].tobytes():
            bad.append(k)
    return bad


# header: iterations, trials, rejected trials, factorisation failures; edges to erase; NaN chi2 among the outputs.  Where every factorisation fails x
# stays zero, so every trial estimate IS the input: Tcw_out = the input, the flags are those of the input, a NaN chi2 is no flag and a NaN depth is one.
FAILING_TABLE = {"nan_obs_free": ([10, 10, 10, 10], 128, 1), "nan_obs_fixed": ([10, 10, 10, 10], 128, 1), "nan_point": ([10, 10, 10, 10], 129, 4),
                 "inf_obs_free": ([10, 10, 10, 0], 0, 160)}


@pytest.mark.parametrize("name", list(G.FAILING))
def test_failing_factorisations(name):
    """a NaN observation at a free and at a fixed keyframe, a NaN point: S holds a NaN, all ten trials of all ten iterations fail at a pivot, the update
    is applied all the same (x = 0) and tempChi = DBL_MAX.  An Inf observation: chi2 = Inf, rho1 = delta / sqrt(Inf) = 0, so H stays finite while
    b = 0 * Inf is NaN -- no pivot fails, x is NaN, every trial is rejected on a NaN rho, and the stale-error rule leaves 160 NaN chi2.  The host form
    equals the rule: header and flags exactly, the outputs by bits with NaNs matched by position."""
    p, host, rule = G.scene(name), G.host_of(name), G.rule_of(name)
    assert nan_matched(host, rule) == [], name
    counts, erase, nans = FAILING_TABLE[name]
    for got in (host, rule):
        assert got["header"][0] == R.OK and got["header"][5:9].tolist() == counts and got["header"][9] == erase == int(got["erase"].sum()), (name, got["header"])
        assert int(np.isnan(got["chi2"]).sum()) == nans, name
        assert np.array_equal(got["Tcw_out"].view(np.uint32), np.asarray(p["pose_table"], F)[p["kf_row"]].view(np.uint32)), name
        assert np.isnan(got["final_chi2"]) if name != "inf_obs_free" else got["final_chi2"] == np.inf, (name, got["final_chi2"])
    e = int(np.nonzero(np.isnan(rule["chi2"]))[0][0])
    if nans == 1:
        assert not rule["erase"][e] and p["kf_fixed"][p["edge_kf"][e]] == (name == "nan_obs_fixed")


def test_host_form_equals_the_rule_by_bits_on_200_random_scenes():
    seen = set()
    for k in range(200):
        h, r = G.host_of(k), G.rule_of(k)
        assert bits_equal(h, r) == [], k
        seen.add((int(r["header"][7]) > 0, int(r["header"][9]) > 0))
    assert len(seen) == 4, "the stream reaches rejected trials and erase flags, with and without each other"


def test_write_back_of_the_host_form():
    p = G.scene("special")
    a, b = G.run_host(p), G.run_host(p, write_back=True)
    assert bits_equal(a, b) == []
    assert np.array_equal(a["pose_table"], p["pose_table"]) and np.array_equal(a["point_table"], p["point_table"])
    free = np.asarray(p["kf_fixed"]) == 0
    T, X = np.asarray(p["pose_table"], F).copy(), np.asarray(p["point_table"], F).copy()
    T[p["kf_row"][free]] = b["Tcw_out"][free]
    moved = np.any(b["points_out"] != X[p["point_row"]], 1)
    X[p["point_row"]] = b["points_out"]
    assert np.array_equal(b["pose_table"], T) and np.array_equal(b["point_table"], X) and moved.sum() >= len(moved) - 3


# ---- the pieces --------------------------------------------------------------------------------------------------------------------------------------
def lib_edge(pose, X, obs, w=1.0):
    L = capi.lib()
    cam = G.cam_struct()
    e, c, Jp, Jl, r1 = np.zeros(3, D), np.zeros(1, D), np.zeros(18, D), np.zeros(9, D), np.zeros(1, D)
    assert L.xfh_lba_edge(np.asarray(pose, D).ctypes.data, np.asarray(X, D).ctypes.data, C.byref(cam), np.asarray(obs, F).ctypes.data, w, e.ctypes.data, c.ctypes.data,
                          Jp.ctypes.data, Jl.ctypes.data, r1.ctypes.data) == 0
    return e, c[0], Jp, Jl, r1[0]


def test_edge_against_the_rule_and_central_differences():
    rng = np.random.RandomState(5)
    cam = RP.cam_of(G.CAM)
    for n in range(60):
        pose = RP.from_tcw(np.concatenate([G._rot(rng.uniform(-0.3, 0.3, 3)), rng.uniform(-1, 1, (3, 1))], 1).reshape(12))
        X = rng.uniform(-1, 1, 3) + [0, 0, 5]
        stereo = bool(n % 2)
        obs = np.array([rng.uniform(0, 640), rng.uniform(0, 480), rng.uniform(0, 600) if stereo else -1.0], F)
        if n % 5 == 0:
            obs[:2] += 300                                                   # beyond the Huber delta
        e, c, Jp, Jl, r1 = lib_edge(pose, X, obs)
        re, rc, r0, rr1, rJp, rJl = R.linearize(pose, cam, X[None], obs.astype(D)[None], np.array([stereo]), 1.0)
        assert np.array_equal(e, np.array([float(v[0]) for v in re])) and c == float(rc[0]) and r1 == float(rr1[0])
        assert np.array_equal(Jp, np.array([float(np.ravel(v)[0]) for v in rJp])) and np.array_equal(Jl, np.array([float(np.ravel(v)[0]) for v in rJl]))
        assert (r1 < 1.0) == (c > (7.815 if stereo else 5.991))
        # central differences of the error: in the point, and in the pose through exp(u) * pose.  The stereo error's invz is a float: its step is
        # 6e-8 relative, so the difference quotient over 2e-4 carries about 1e-3 px
        err = lambda ps, Xs: np.array([float(v) for v in RP.edge_error(ps, cam, np.asarray(Xs, D), obs.astype(D), stereo, 1.0)[1]])
        h = 1e-4
        tol = 0.05 if stereo else 1e-4
        for a in range(3):
            d = np.zeros(3)
            d[a] = h
            assert np.allclose((err(pose, X + d) - err(pose, X - d)) / (2 * h), Jl.reshape(3, 3)[:, a], atol=tol, rtol=1e-4), (n, "point", a)
        for a in range(6):
            u = np.zeros(6)
            u[a] = h
            assert np.allclose((err(RP.oplus(u, pose), X) - err(RP.oplus(-u, pose), X)) / (2 * h), Jp.reshape(3, 6)[:, a], atol=tol * 10, rtol=1e-4), (n, "pose", a)
    assert capi.lib().xfh_lba_edge(None, None, None, None, 1.0, None, None, None, None, None) == INVALID


def test_point_block_against_the_rule_and_numpy():
    L, rng = capi.lib(), np.random.RandomState(6)
    for n in range(50):
        A = rng.normal(0, 1, (3, 3))
        H = A @ A.T * 10.0 ** rng.randint(-3, 6)
        H6 = np.array([H[0, 0], H[0, 1], H[0, 2], H[1, 1], H[1, 2], H[2, 2]], D)
        lam = float(10.0 ** rng.randint(-8, 2))
        out = np.zeros(9, D)
        assert L.xfh_lba_point_block(H6.ctypes.data, lam, out.ctypes.data) == 0
        assert np.array_equal(out, R.point_block(H6, lam)[0])
        assert np.allclose(out.reshape(3, 3) @ (H + lam * np.eye(3)), np.eye(3), atol=1e-6)
    out = np.zeros(9, D)                                                     # a singular block makes what it makes
    assert L.xfh_lba_point_block(np.zeros(6, D).ctypes.data, 0.0, out.ctypes.data) == 0 and not np.isfinite(out).any()
    assert np.array_equal(out, R.point_block(np.zeros(6, D), 0.0)[0], equal_nan=True)
    assert L.xfh_lba_point_block(None, 1.0, out.ctypes.data) == INVALID


def test_solve_against_the_rule_and_numpy():
    L, rng = capi.lib(), np.random.RandomState(7)
    for n in (1, 5, 6, 12, 66, 132):
        A = rng.normal(0, 1, (n, n))
        S = A @ A.T + n * np.eye(n)
        b = rng.normal(0, 1, n)
        x, Sc = np.full(n, 7.0, D), np.tril(S).copy()
        assert L.xfh_lba_solve(n, Sc.ctypes.data, b.ctypes.data, x.ctypes.data) == 1
        ok, xr, _ = R.ldlt_solve(np.tril(S), b, np.zeros(n))
        assert ok and np.array_equal(x, xr) and np.allclose(x, np.linalg.solve(S, b), rtol=1e-9, atol=1e-12)
        S[n // 2, n // 2] = -1.0 if n % 2 else np.nan                        # a pivot that is not > 0: x is untouched
        x, Sc = np.full(n, 7.0, D), np.tril(S).copy()
        assert L.xfh_lba_solve(n, Sc.ctypes.data, b.ctypes.data, x.ctypes.data) == 0 and np.all(x == 7.0)
        assert not R.ldlt_solve(np.tril(S), b, np.zeros(n))[0]
    assert L.xfh_lba_solve(0, Sc.ctypes.data, b.ctypes.data, x.ctypes.data) == 0 and L.xfh_lba_solve(769, Sc.ctypes.data, b.ctypes.data, x.ctypes.data) == 0


# ---- a hand-made case: one point, two keyframes, one step, solved as ONE dense 9 x 9 system ---------------------------------------------------------------
def test_one_point_two_keyframes_one_step():
    """Keyframe 0 is fixed at the origin, keyframe 1 is free; one point, seen by both, stereo.  optimize(1): errors, H and b at the start, lambda = 1e-5 max
    |diag|, ONE solve of the full (H + lambda I) x = b over the 6 + 3 unknowns -- no Schur complement, no block inverse -- and the update.  The call's
    Tcw_out and points_out must be that update, its final_chi2 the robust chi2 there."""
    cam = RP.cam_of(G.CAM)
    T0 = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F)
    T1 = np.array([1, 0, 0, -0.5, 0, 1, 0, 0.01, 0, 0, 1, 0.02], F)
    X = np.array([0.4, -0.2, 5.0], F)
    obs = np.array([[361.0, 219.5, 353.2], [310.5, 221.0, 302.4]], F)
    p = dict(pose_table=np.stack([T0, T1]), point_table=X[None], kf_row=np.array([0, 1], np.int32), kf_fixed=np.array([1, 0], np.uint8),
             point_row=np.array([0], np.int32), edge_begin=np.array([0, 2], np.int32), edge_kf=np.array([0, 1], np.int32), edge_obs=obs, cam=G.CAM, inv_sigma2=1.0,
             max_iterations=1)
    poses, Xd = [RP.from_tcw(T0), RP.from_tcw(T1)], X.astype(D)
    H, b, chi = np.zeros((9, 9)), np.zeros(9), 0.0
    for k in range(2):
        e, c, Jp, Jl, r1 = lib_edge(poses[k], Xd, obs[k])
        assert c < 7.815 and r1 == 1.0                                       # inside the Huber delta: plain least squares
        J = np.concatenate([Jp.reshape(3, 6) if k == 1 else np.zeros((3, 6)), Jl.reshape(3, 3)], 1)
        H += J.T @ J
        b -= J.T @ e
        chi += c
    lam = 1e-5 * np.max(np.abs(np.diag(H)))
    x = np.linalg.solve(H + lam * np.eye(9), b)
    new_pose, new_X = RP.oplus(x[:6], poses[1]), Xd + x[6:]
    new_chi = sum(lib_edge(q, new_X, obs[k])[1] for k, q in enumerate([poses[0], new_pose]))
    assert new_chi < chi
    for got in (G.run_host(p), R.rule(p)):
        assert got["header"].tolist() == [0, 1, 1, 0, 2, 1, 1, 0, 0, 0]
        assert np.array_equal(got["Tcw_out"][0], T0) and np.allclose(got["Tcw_out"][1], RP.to_tcw(new_pose), atol=2e-7) and np.allclose(got["points_out"][0], new_X, atol=1e-6)
        assert abs(got["final_chi2"] - new_chi) < 1e-9 * max(1.0, new_chi) and np.allclose(got["chi2"], [lib_edge(poses[0], new_X, obs[0])[1], lib_edge(new_pose, new_X, obs[1])[1]], rtol=1e-6)


# ---- refusals and early statuses ---------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_of_the_host_form():
    L, p = capi.lib(), G.scene("one_free")
    nK, nP, nE = G.dims(p)
    arrays = [np.ascontiguousarray(np.asarray(p[k], dt)).copy() for k, dt in G.INPUTS]
    outs = local_ba.local_ba_layout(nK, nP, nE).zeros()
    ws = np.zeros(int(L.xfh_local_ba_workspace_bytes(nK, nP, nE, 1)) + 32, np.uint8)
    wsp = (ws.ctypes.data + 15) & ~15
    cam = G.cam_struct()

    def call(nK=nK, nf=1, nP=nP, nE=nE, rows=(len(arrays[0]), len(arrays[1])), ptrs=None, w=1.0, its=10, wb=0, wsp=wsp, outp=None, cam=C.byref(cam)):
        ptrs = ptrs or [a.ctypes.data for a in arrays]
        outp = outp or [outs[k].ctypes.data for k in local_ba.NAMES]
        return L.xfh_local_ba_host(nK, nf, nP, nE, ptrs[0], rows[0], ptrs[1], rows[1], *ptrs[2:], cam, w, its, wb, wsp, *outp)

    assert call() == 0
    assert call(nf=local_ba.MAX_FREE + 1, nK=200) == INVALID and call(nf=-1) == INVALID and call(nf=nK + 1) == INVALID
    for kw in (dict(nK=0), dict(nP=0), dict(nE=0), dict(nK=65536), dict(rows=(0, 5)), dict(rows=(5, 0)), dict(its=0), dict(its=11), dict(wb=2), dict(wb=-1)):
        assert call(**kw) == INVALID, kw
    for w in (0.0, -1.0, np.nan, np.inf, -np.inf):
        assert call(w=w) == INVALID, w
    assert call(cam=None) == INVALID and call(wsp=None) == INVALID and call(wsp=wsp + 8) == INVALID
    for i in range(len(arrays)):
        ptrs = [a.ctypes.data for a in arrays]
        ptrs[i] = None
        assert call(ptrs=ptrs) == INVALID, i
        if G.INPUTS[i][1] != np.uint8:
            ptrs[i] = arrays[i].ctypes.data + 2
            assert call(ptrs=ptrs) == INVALID, i
    for i, k in enumerate(local_ba.NAMES):
        outp = [outs[n].ctypes.data for n in local_ba.NAMES]
        outp[i] = None
        assert call(outp=outp) == INVALID, k
    assert L.xfh_local_ba_workspace_bytes(0, 1, 1, 0) == 0 and L.xfh_local_ba_workspace_bytes(3, 1, 1, 4) == 0 and L.xfh_local_ba_workspace_bytes(200, 1, 1, 129) == 0
    assert L.xfh_local_ba_workspace_bytes(200, 1, 1, 128) > 768 * 768 * 8


@pytest.mark.parametrize("name,status", [("aborted", R.ABORTED), ("nothing_free", R.NOTHING_FREE)])
def test_early_statuses_leave_every_output_at_its_input(name, status):
    p = G.scene(name)
    for got in (G.run_host(p, write_back=True), G.rule_of(name)):
        assert got["header"][0] == status and got["header"][5:].tolist() == [0] * 5 and got["final_chi2"] == 0.0
        assert np.array_equal(got["Tcw_out"], np.asarray(p["pose_table"], F)[p["kf_row"]]) and np.array_equal(got["points_out"], np.asarray(p["point_table"], F)[p["point_row"]])
        assert not got["erase"].any() and not got["chi2"].any()
    h = G.run_host(p, n_free=G.n_free_of(p) + 1 if name == "nothing_free" else 0)
    assert h["header"][0] == R.FREE_MISMATCH


# ---- the condition of the rig -----------------------------------------------------------------------------------------------------------------------------
def test_rig_reaches_what_the_gpu_tests_name():
    free = {n: G.n_free_of(G.scene(n)) for n in list(G.SCENES) + list(G.LIMIT)}
    assert {1, 2, 11, 22, 128} <= set(free.values())
    p = G.scene("kf_edges")
    assert sorted(np.bincount(p["edge_kf"], minlength=8).tolist())[:5] == [0, 1, 255, 256, 257]
    assert G.scene("two_free_mono")["edge_obs"][:, 2].max() < 0 and G.scene("stereo_only")["edge_obs"][:, 2].min() >= 0
    p = G.scene("seen_by_all")
    assert np.any(np.diff(p["edge_begin"]) == len(p["kf_row"]))
    s, r = G.scene("special"), G.rule_of("special")
    deg = np.array([np.sum((s["edge_kf"][a:b] >= 0) & (s["edge_kf"][a:b] < len(s["kf_row"]))) for a, b in zip(s["edge_begin"][:-1], s["edge_begin"][1:])])
    assert 0 in deg and 1 in deg and 2 in deg and (s["edge_kf"] < 0).any() and (s["edge_kf"] >= len(s["kf_row"])).any()
    behind = [e for e in range(len(s["edge_kf"])) if r["erase"][e] and r["chi2"][e] <= 5.991]
    assert behind, "no edge is erased for its depth alone"
    assert all(G.scene(n)["kf_fixed"][0] == 1 and G.scene(n)["kf_fixed"][1] == 0 for n in ("eleven_mixed", "outliers")), "the initial keyframe, fixed inside the local set"
    assert G.rule_of("far_start")["header"][7] > 0 and G.rule_of("outliers")["header"][9] > 10
    # the wraps: chi2 folds of more than 256 terms, a second and a third pass of the 256 lanes over a keyframe's edges (by one lane and by whole waves),
    # nK the largest dimension, and iteration limits other than 10 and 2
    w, idle = G.scene("wide"), G.scene("idle_keyframes")
    assert G.dims(w) == (266, 520, 3496) and np.bincount(w["edge_kf"], minlength=266)[:6].tolist() == [520, 400, 511, 512, 513, 520]
    assert G.dims(idle) == (300, 6, 27) and max(G.dims(idle)) == 300 and int((np.bincount(idle["edge_kf"], minlength=300) == 0).sum()) == 295
    assert G.rule_of("idle_keyframes")["header"][5:8].tolist() == [7, 15, 8] and G.rule_of("wide_far")["header"][9] > 100
    assert G.rule_of("far_start_1it")["header"][5] == 1 and G.rule_of("far_start_3it")["header"][5] == 3
    # weights other than 1 decide differently
    assert [int(G.rule_of(n)["header"][9]) for n in ("outliers", "outliers_w0694", "outliers_w4")] == [31, 30, 34]
    assert G.scene("outliers_w0694")["inv_sigma2"] == float(F(1 / 1.44)) and G.scene("outliers_w4")["inv_sigma2"] == 4.0
    assert any(ev[0] == "trial" and not ev[3] for ev in G.rule_of("far_start")["events"])


@pytest.mark.parametrize("name", list(G.SCENES) + list(G.LIMIT))
def test_rig_condition(name):
    """every chi2 is farther from its threshold, every depth from 0 and every rho from 0 than 8 x the deviation between the float64 forms: measured on the
    literal form alone (tests/ref_local_ba_literal.py shares no summation order with the kernels), against the spread of all the forms.  rho is
    (currentChi - tempChi) / (scale + 1e-3), so two forms' rho differ by at most their chi2 sums' difference over 1e-3."""
    forms = G.forms_of(name)
    lit, rule = forms[0], forms[1]
    sp = G.spread(forms)
    m = rule["margins"]
    th = 5.991
    chi_dev = sp["chi2"] * float(np.spacing(F(th))) / th                     # float32 steps at max(chi2, th) -> relative to the threshold
    assert m["classify"] > 8 * chi_dev, (name, m["classify"], chi_dev)
    assert m["depth"] > 8 * max(sp["points"], sp["tcw"]) * float(np.spacing(F(64.0))), (name, m["depth"])
    rho_dev = sp["final"] * max(rule["final_chi2"], th) / 1e-3
    assert m["rho"] > 8 * rho_dev, (name, m["rho"], rho_dev)
    assert G.decisions_differ(lit, rule) == [] and lit["events"] == rule["events"], name


# ---- the sanitizer program ----------------------------------------------------------------------------------------------------------------------------------
def problem_file(path, p, expected=None, write_back=0):
    nK, nP, nE = G.dims(p)
    arrays = [np.ascontiguousarray(np.asarray(p[k], dt)) for k, dt in G.INPUTS]
    with open(path, "wb") as f:
        f.write(np.array([nK, G.n_free_of(p), nP, nE, len(arrays[0]), len(arrays[1]), p.get("max_iterations", 10), write_back, 1 if expected else 0], np.int32).tobytes())
        f.write(np.array(list(p["cam"]) + [p["inv_sigma2"]], F).tobytes())
        for a in arrays:
            f.write(a.tobytes())
        if expected:
            for k in OUT:
                f.write(np.ascontiguousarray(expected[k]).tobytes())
            f.write(struct.pack("d", expected["final_chi2"]))
        else:
            P = R.Plan(p) if "plan_ok" in p else None
            f.write(np.array([0, G.n_free_of(p), P.fixed_with_edge, P.mono, P.stereo_n] if P else [0] * 5, np.int32).tobytes())
    return path


def test_lba_math_under_sanitizers(tmp_path):
    """tests/cpp/asan_local_ba_test.cpp, a stand-alone program built from lba_math.h alone with AddressSanitizer + UBSan: the two Levenberg machines
    (geo_lm_* and the distributed restatement) driven with the same chi2 sequences and compared field by field; the stale-error rule with a FORCED
    rejected last trial; and the whole rule in buffers of exact size -- good problems byte for byte against the Python rule, problems with NaN, Inf and 1e30
    in every float array against the plan's counts (the Python rule and C++ do not give a NaN the same bits).  Nothing of the library is linked, nothing
    runs on a GPU, nothing is loaded into Python."""
    exe = str(tmp_path / "asan_local_ba_test")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "xfeatslam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "asan_local_ba_test.cpp"), "-o", exe])
    files = []
    for n in ("one_free", "kf_edges", "special", "far_start", "outliers", "aborted", "nothing_free", 3, 8):
        files.append(problem_file(str(tmp_path / ("good_%s.bin" % n)), G.problem_of(n), G.rule_of(n), write_back=1 if n in ("special", 8) else 0))
    rng = np.random.RandomState(9)
    bad = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0, 1e-30], F)
    for s in range(4):
        p = dict(G.random_small(300 + s), plan_ok=True)
        for k in ("pose_table", "point_table", "edge_obs"):
            a = np.asarray(p[k], F).copy()
            m = rng.rand(*a.shape) < (0.1, 0.3, 1.0, 0.02)[s]
            a[m] = rng.choice(bad, int(m.sum()))
            if k == "edge_obs":
                a[:, 2] = np.asarray(p[k], F)[:, 2]                           # the kind of an edge is a decision of the plan: kept
            p[k] = a
        files.append(problem_file(str(tmp_path / ("nan_%d.bin" % s)), p))
    r = subprocess.run([exe] + files, capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "asan_local_ba_test ok (%d files)" % len(files) in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


def test_kernels_use_no_scratch():
    """kernels_lba.hip: no kernel may spill to scratch (clang's kernel-resource-usage remarks; no GPU needed)"""
    import re
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("needs hipcc")
    src = os.path.join(ROOT, "xfeatslam_amd", "csrc", "kernels_lba.hip")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", os.devnull], capture_output=True, text=True, timeout=600)
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) >= 14 and all(v == 0 for v in scratch), list(zip(names, scratch))
