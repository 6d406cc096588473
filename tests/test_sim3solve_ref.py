"""CPU tests of the Sim3 solver and the merge in front of it (xfh_sim3_solve*, xfh_sim3_merge_matches*): the library's host code -- the very lines
the kernels compile, sim3solve_math.h -- against the rule form of tests/ref_sim3solve.py BY BITS on the scenes of tests/sim3solve_rig.py and on 200
random small scenes; each stateless piece against the rule on every iteration; the set generator against the shrinking-vector loop; the iteration
function against the reference's expression; the order-free decision and merge against the literal loops of tests/ref_sim3solve_literal.py;
hand-made cases with written-out answers; the recovered similarity against the one the scenes were made with; every refusal that needs no device;
and the stand-alone sanitizer program.  No GPU is used."""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_sim3solve as R
import ref_sim3solve_literal as LIT
import sim3solve_rig as G
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
bits = lambda a: np.ascontiguousarray(a).view(np.uint8).ravel()
eq = lambda a, b: bits(G.canonical_nan(a)).tobytes() == bits(G.canonical_nan(b)).tobytes()          # floats by bits, a NaN equal to any NaN


@pytest.fixture(scope="module")
def scenes():
    """the rig's scenes and the rule's answer for each: computed once, never changed"""
    s = G.rig()
    return s, {k: G.rule_of(v) for k, v in s.items()}


def test_host_form_equals_the_rule_by_bits_and_every_status_is_reached(scenes):
    s, want = scenes
    seen = set()
    for n, sc in s.items():
        prior = dict(floats=np.full(32, 7.5, F), inliers=np.full(len(sc["point1"]), 9, np.uint8), Tcw=np.full(12, -2.0, F), Ow=np.full(3, 4.0, F))
        got = G.host_of(sc, prior=prior)
        G.assert_equals_rule(got, want[n], 0)
        for k, v in prior.items():                                         # what the call leaves alone comes back as it was
            if want[n][k] is None:
                assert bits(got[k][0]).tobytes() == bits(v).tobytes(), (n, k)
        assert R.STATUS_NAMES[want[n]["header"][1]] == G.EXPECT[n], (n, dict(zip(R.HEADER, want[n]["header"].tolist())))
        seen.add(int(want[n]["header"][1]))
    assert seen == {0, 1, 2}


def test_conditions_of_the_scenes(scenes):
    """what each scene is in the rig for"""
    s, want = scenes
    h = lambda n: dict(zip(R.HEADER, want[n]["header"].tolist()))
    assert h("first")["winner"] == 0 and h("first")["consumed"] == 1
    assert h("after20")["winner"] == 25 and h("after64")["winner"] == 70 and h("after64")["its"] == 92         # past a chunk of 20, past a wave of 64
    assert all(c <= 15 for c in want["after64"]["counts"][:70])
    g, r = h("no_more"), want["no_more"]                                    # the largest count occurs twice: the LAST one is the best
    mx = r["counts"].max()
    assert g["status"] == R.NO_MORE and (r["counts"] == mx).sum() >= 2 and g["best"] == np.nonzero(r["counts"] == mx)[0][-1] == g["its"] - 1 and 0 < mx <= 30
    assert g["best_count"] == mx and g["its"] == 10 == R.iterations(0.99, 30, 300, 41)                       # a count below the cap, from the formula
    assert h("n_equals_min") == dict(N=15, status=R.NO_MORE, its=1, winner=-1, n_inliers=0, best=0, best_count=15, consumed=1)
    assert h("n_below_min")["N"] == 10 and h("n2")["N"] == 2 and s["n2"]["min_inliers"] == 0
    assert h("capped")["its"] == 20 and s["capped"]["table"][41] == 92 and h("its65")["its"] == 65
    assert h("big")["N"] == 261 and h("big")["its"] == 300 and h("big_outliers")["consumed"] == 300 and R.iterations(0.99, 15, 10 ** 9, 261) > 300
    r, sc = want["collinear"], s["collinear"]                              # iteration 0 fits three collinear points
    P = r["X1"][r["sets"][0]].astype(np.float64)
    assert np.linalg.matrix_rank(P - P.mean(0), tol=1e-4) == 1 and r["sets"][0].tolist() == [0, 40, 39]
    r = want["equal_points"]                                                # draws outside 0 .. rand_max: first and last position, the same two points
    assert r["sets"][0].tolist() == [0, 40, 38] and eq(r["X1"][0], r["X1"][40]) and eq(r["X2"][0], r["X2"][40])
    r = want["zero_rotation"]                                               # X1 == X2 by bits: the identity, exactly, where the reference divides 0 by 0
    assert eq(r["X1"], r["X2"]) and eq(r["floats"][R.F_R12:R.F_R12 + 9], np.eye(3).ravel()) and r["header"][3] == 0 and r["floats"][R.F_S] != 0
    r = want["nan_point"]
    assert np.isnan(r["X2"][0]).any() and r["counts"][0] == 0 and np.isnan(r["hyps"][0][:12]).any() and r["header"][1] == R.CONVERGED and r["inliers"][s["nan_point"]["slots"][0]] == 0
    assert h("fixed")["status"] == R.NO_MORE and want["fixed"]["hyps"][:, R.F_S].tolist() == [1.0] * 92 and want["fixed_unit"]["floats"][R.F_S] == 1.0


def test_converged_scenes_recover_the_similarity_they_were_made_with(scenes):
    """T12 against the scene's (R, t, s).  Bounds from the noise: 2e-3 units on points a few units apart is a milliradian per point; a similarity refit
    on three of them is inside 1 degree, 2 % of scale and 0.15 units of translation (points 3 .. 9 units from the camera: 1 degree there is 0.1)."""
    s, want = scenes
    for n in ("first", "after20", "after64", "scaled", "fixed_unit", "big", "nan_point", "equal_points", "collinear"):
        r, (Rm, t, sc) = want[n], s[n]["S"][0]
        got_R, got_t, got_s = r["floats"][R.F_R12:R.F_R12 + 9].reshape(3, 3).astype(np.float64), r["floats"][R.F_T:R.F_T + 3], float(r["floats"][R.F_S])
        ang = np.degrees(np.arccos(np.clip((np.trace(got_R @ Rm.T) - 1) / 2, -1, 1)))
        assert ang < 1.0 and abs(got_s / sc - 1) < 0.02 and np.abs(got_t - t).max() < 0.15, (n, ang, got_s, got_t, t)
        assert abs(np.linalg.det(got_R) - 1) < 1e-5
        T12 = r["floats"][:12].reshape(3, 4)
        assert eq(T12[:, :3], F(r["floats"][R.F_S]) * r["floats"][R.F_R12:R.F_R12 + 9].reshape(3, 3)) and eq(T12[:, 3], got_t)
        # the composed pose maps the candidate's world points into the current camera as T12 o T2w does
        Tcw, Ow = r["Tcw"].reshape(3, 4).astype(np.float64), r["Ow"].astype(np.float64)
        p = s[n]["points"][s[n]["matched"][0][s[n]["slots"][1:4]]].astype(np.float64)
        X2 = p @ s[n]["T2w"][0].reshape(3, 4)[:, :3].astype(np.float64).T + s[n]["T2w"][0].reshape(3, 4)[:, 3]
        want_X = (X2 @ T12[:, :3].astype(np.float64).T + T12[:, 3]) / got_s
        assert np.abs(p @ Tcw[:, :3].T + Tcw[:, 3] - want_X).max() < 1e-4 and np.abs(Tcw[:, :3] @ Ow + Tcw[:, 3]).max() < 1e-5


def test_random_scenes_host_form_equals_the_rule():
    seen = set()
    for sc in G.random_scenes():
        w = G.rule_of(sc)
        G.assert_equals_rule(G.host_of(sc), w, 0)
        seen.add(int(w["header"][1]))
    assert seen == {R.NO_MORE, R.CONVERGED}


def test_host_pieces_equal_the_rule_on_every_iteration(scenes):
    s, want = scenes
    ran = 0
    for n, sc in s.items():
        r = want[n]
        if r["its"] == 0:
            continue
        ran += 1
        cam1, cam2, N = G.camera(sc["cam1"]), G.camera(sc["cam2"]), len(r["cm"])
        for it in range(r["its"]):
            assert Context.sim3_solve_set(sc["draws"][0][it], G.RAND_MAX, N).tolist() == r["sets"][it].tolist(), (n, it)
            hyp = Context.sim3_solve_horn(r["X1"][r["sets"][it]], r["X2"][r["sets"][it]], sc["fix_scale"])
            assert eq(hyp, r["hyps"][it]), (n, it)
            err, flags = R.check(r["hyps"][it], sc["cam1"], sc["cam2"], r["X1"], r["X2"], r["P1"], r["P2"], 9.0, 9.0)
            ks = range(N) if it in (r["header"][3], r["header"][5]) else sorted({(7 * it) % N, (13 * it + 5) % N, N - 1 - it % N})
            for k in ks:
                e, f = Context.sim3_solve_check(r["hyps"][it][:12], r["hyps"][it][R.F_T21:R.F_T21 + 12], cam1, cam2, r["X1"][k], r["X2"][k])
                assert eq(e, err[k]) and f == int(flags[k]), (n, it, k)
    assert ran == len(s) - 2


def test_set_generator_equals_the_shrinking_vector_loop():
    rng = np.random.RandomState(5)
    for rand_max in (32767, 2147483647, 1):
        for N in (3, 4, 41, 1000):
            for k in range(60):
                d = rng.randint(0, rand_max + 1, 3, dtype=np.int64).astype(np.int32)
                if k == 0:
                    d[:] = 0
                elif k == 1:
                    d[:] = rand_max
                got = Context.sim3_solve_set(d, rand_max, N).tolist()
                assert got == R.set_of_iteration(d, rand_max, N), (rand_max, N, d.tolist())
                assert len(set(got)) == 3 and min(got) >= 0 and max(got) < N
    assert Context.sim3_solve_set([0, 0, 0], 32767, 10).tolist() == [0, 9, 8]                # position 0 is refilled from the back each time
    assert Context.sim3_solve_set([32767] * 3, 32767, 10).tolist() == [9, 8, 7]              # always the last position
    assert Context.sim3_solve_set([16384] * 3, 32767, 8).tolist() == [4, 3, 6]               # int(0.5 * d) of the shrinking vector, by hand
    assert Context.sim3_solve_set([40000, -3, 0], 32767, 9).tolist() == [8, 0, 7]            # outside 0 .. rand_max: clamped into the vector
    assert Context.sim3_solve_set([0, 0, 0], 32767, 3).tolist() == [0, 2, 1]


def test_iteration_function_equals_the_reference_expression():
    """every N up to 4096 at the caller's parameters (0.99, 15, 300), the expression of Sim3Solver.cc:134-144 evaluated with math; where it is not
    finite (N = 0: epsilon = inf; N < 15: the logarithm of a negative number) the function returns max_its"""
    def reference(prob, mn, mx, N):
        if mn == N:
            return 1
        with np.errstate(all="ignore"):
            eps = float(F(mn) / F(N))
        x = 1.0 - math.pow(eps, 3)
        if not x > 0.0 or math.log(x) == 0.0:
            return mx                                                       # log of a non-positive number, or a division by zero: not finite
        v = math.ceil(math.log(1 - prob) / math.log(x))
        return max(1, min(v, mx))
    table = Context.sim3_solve_iterations_table(0.99, 15, 300, 4096)
    for N in range(4097):
        assert Context.sim3_solve_iterations(0.99, 15, 300, N) == reference(0.99, 15, 300, N) == R.iterations(0.99, 15, 300, N) == table[N], N
    assert table[15] == 1 and table[0] == 300 and table[14] == 300 and table[16] == 3 and table[41] == 92 and table[4096] == 300
    for prob, mn, mx in ((0.99, 0, 300), (0.5, 3, 7), (0.999999, 100, 100000), (1.0, 15, 300), (0.0, 15, 300), (0.99, 15, 0), (float("nan"), 15, 300)):
        for N in (0, 1, 2, 3, 50, 100, 101, 5000):
            assert Context.sim3_solve_iterations(prob, mn, mx, N) == R.iterations(prob, mn, mx, N), (prob, mn, mx, N)
    assert Context.sim3_solve_iterations(0.99, 15, 10 ** 9, 10 ** 6) == 10 ** 9              # the double does not fit an int


def test_order_free_decision_equals_the_sequential_loop_with_chunks_of_20():
    """the literal iterate(20) loop under `while(!bConverge && !bNoMore)` with mnBestInliers carried across the chunks, on random count sequences that
    cross the chunk ends, against the first-above / last-of-the-largest form"""
    rng = np.random.RandomState(11)
    for trial in range(3000):
        its, mn = int(rng.randint(1, 90)), int(rng.randint(0, 12))
        counts = rng.randint(0, mn + (2 if trial % 3 else 1), its)
        if trial % 7 == 0:
            counts[:] = rng.randint(0, 3)
        best_n, best_it, done, conv, no_more, winner = 0, -1, 0, False, False, -1
        while not conv and not no_more:                                     # LoopClosing.cc:706-710
            cur = 0
            while done < its and cur < 20:                                  # Sim3Solver.cc:240
                cur += 1
                n = counts[done]
                done += 1
                if n >= best_n:
                    best_n, best_it = n, done - 1
                    if n > mn:
                        conv, winner = True, done - 1
                        break
            if not conv and done >= its:
                no_more = True
        w, b = R.decide(counts, mn)
        assert (w, b) == (winner, best_it) and (done == (w + 1 if w >= 0 else its)), (counts.tolist(), mn)


def test_rule_decisions_equal_the_literal_solver_with_chunks_of_other_sizes(scenes):
    """the literal solver's outcome does not depend on the chunk length: 20, 1, 7 and all at once give the winner of the order-free rule"""
    s, want = scenes
    for n in ("after20", "after64", "no_more", "capped", "first"):
        sc, r = s[n], want[n]
        for chunk in (20, 1, 7, 1000):
            lit = LIT.solve(sc["points"], sc["point1"], sc["matched"][0], sc["T1w"], sc["T2w"][0], sc["cam1"], sc["cam2"], sc["draws"][0], G.RAND_MAX,
                            min_inliers=sc["min_inliers"], fix_scale=sc["fix_scale"], chunk=chunk)
            assert lit["winner"] == r["header"][3] and lit["iterations"] == r["header"][7] and lit["converged"] == (r["header"][1] == R.CONVERGED), (n, chunk)


def test_merge_equals_the_literal_loop():
    m = G.merge_scene()
    got = Context.sim3_merge_matches_host(m["match12"], m["point2"], m["M"])
    want, lit = R.merge(m["match12"], m["point2"], m["M"]), LIT.merge(m["match12"], m["point2"], m["M"])
    for a, b, c in zip(got, want, lit):
        assert np.array_equal(a, b) and np.array_equal(b, c)
    matched, kf, num = got
    M = m["M"]
    assert (matched[3], kf[3]) == (M - 8, 1) and (matched[9], kf[9]) == (M - 7, 0) and (matched[20], kf[20]) == (M - 6, 0) and (matched[40], kf[40]) == (-1, -1)
    assert matched[30] == -1 or kf[30] != 2
    assert num == len({int(v) for j in range(3) for k, v in enumerate(np.where((m["match12"][j] >= 0) & (m["match12"][j] < 80), m["point2"][j][np.clip(m["match12"][j], 0, 79)], -1))
                       if 0 <= v < m["M"]})
    rng = np.random.RandomState(3)
    for trial in range(200):
        J, n1, n2, M = int(rng.randint(1, 6)), int(rng.randint(1, 40)), int(rng.randint(1, 40)), int(rng.randint(1, 30))
        m12, p2 = rng.randint(-3, n2 + 3, (J, n1)), rng.randint(-3, M + 3, (J, n2))
        got, lit = Context.sim3_merge_matches_host(m12, p2, M), LIT.merge(m12, p2, M)
        assert all(np.array_equal(a, b) for a, b in zip(got, lit)), trial


def test_hand_made_cases_with_written_out_answers():
    # three points and their images under a rotation of 90 degrees about z, scale 2, translation (1, 2, 3): X1 = 2 Rz X2 + t
    X2 = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], F)
    Rz = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float64)
    X1 = (2 * X2.astype(np.float64) @ Rz.T + [1, 2, 3]).astype(F)
    h = Context.sim3_solve_horn(X1, X2, False)
    assert np.allclose(h[R.F_R12:R.F_R12 + 9].reshape(3, 3), Rz, atol=1e-6) and abs(h[R.F_S] - 2) < 1e-6 and np.allclose(h[R.F_T:R.F_T + 3], [1, 2, 3], atol=1e-5)
    assert np.allclose(h[R.F_T21:R.F_T21 + 12].reshape(3, 4), np.concatenate([0.5 * Rz.T, (-0.5 * Rz.T @ [1, 2, 3])[:, None]], 1), atol=1e-5)
    h = Context.sim3_solve_horn(X1, X2, True)                               # fix_scale: s = 1.0f exactly, the same rotation
    assert h[R.F_S] == 1.0 and np.allclose(h[R.F_R12:R.F_R12 + 9].reshape(3, 3), Rz, atol=1e-6)
    h = Context.sim3_solve_horn(X2, X2, False)                              # a zero rotation: the identity by bits, no NaN
    assert eq(h[R.F_R12:R.F_R12 + 9], np.eye(3).ravel()) and h[R.F_S] == 1.0 and not h[R.F_T:R.F_T + 3].any()
    h = Context.sim3_solve_horn(np.zeros((3, 3), F), np.zeros((3, 3), F), False)             # three equal points: R = I, s = 0 / 0
    assert eq(h[R.F_R12:R.F_R12 + 9], np.eye(3).ravel()) and np.isnan(h[R.F_S])
    cam = G.camera((F(100), F(100), F(50), F(50)))
    eye = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F)
    shift = np.array([1, 0, 0, 0.02, 0, 1, 0, 0, 0, 0, 1, 0], F)            # T12 moves X2 by 0.02 along x: at depth 1 that is 2 pixels, err1 = 4
    err, inl = Context.sim3_solve_check(shift, eye, cam, cam, [0, 0, 1], [0, 0, 1])
    assert abs(err[0] - 4) < 1e-3 and err[1] == 0 and inl == 1
    shift[3] = 0.03                                                          # 3 pixels: 9 < 9 is false
    err, inl = Context.sim3_solve_check(shift, eye, cam, cam, [0, 0, 1], [0, 0, 1])
    assert abs(err[0] - 9) < 1e-3 and inl == int(err[0] < 9)
    err, inl = Context.sim3_solve_check(eye, eye, cam, cam, [0, 0, 1], [0, float("nan"), 1])  # a NaN never passes
    assert inl == 0 and np.isnan(err[0])
    assert Context.sim3_max_err(1.0) == 9.0 and Context.sim3_max_err(1.44) == 13.0


def test_batches_strides_and_the_merge_count_on_the_host():
    fam = G.family()
    got = G.host_of(fam)
    for b, st in enumerate((R.CONVERGED, R.NO_MORE, R.TOO_FEW)):
        w = G.rule_of(fam, b)
        G.assert_equals_rule(got, w, b)
        assert w["header"][1] == st, (b, w["header"][:8])
    d = fam["draws"][0]
    shared, copies = G.host_of(dict(fam, draws=d[None])), G.host_of(dict(fam, draws=np.stack([d, d, d])))
    assert all(bits(shared[k]).tobytes() == bits(copies[k]).tobytes() for k in R.OUTPUTS)
    per = G.host_of(dict(fam, T1w=np.stack([fam["T1w"]] * 3)))
    assert all(bits(per[k]).tobytes() == bits(got[k]).tobytes() for k in R.OUTPUTS)
    one = dict(fam, matched=fam["matched"][:1], T2w=fam["T2w"][:1], draws=fam["draws"][:1])
    assert G.host_of(one, num_matches=19, min_matches=20)["header"][0, :2].tolist() == [41, R.TOO_FEW]          # nBoWMatches at LoopClosing.cc:691
    assert G.host_of(one, num_matches=20, min_matches=20)["header"][0, 1] == R.CONVERGED
    hostile = dict(one, point1=one["point1"].copy(), matched=one["matched"].copy(), draws=one["draws"].copy(), table=one["table"].copy())
    sl = hostile["slots"]
    hostile["point1"][sl[2]], hostile["matched"][0, sl[3]], hostile["matched"][0, sl[4]] = 300, 2 ** 31 - 1, -2 ** 31
    hostile["draws"][0, 0], hostile["draws"][0, 1, 1] = (-5, 2 ** 31 - 1, -2 ** 31), 40000
    hostile["table"][:] = 2 ** 31 - 1
    G.assert_equals_rule(G.host_of(hostile), G.rule_of(hostile), 0)


def test_refusals_without_a_device_and_kernel_names():
    L = capi.lib()
    cam = G.camera()
    a = np.zeros(1 << 17, np.float64)
    p = a.ctypes.data

    def hostcall(B=1, n1=8, M=8, e1=9.0, e2=9.0, mi=3, iters=2, dstride=0, tstride=0, rand_max=7, cam1=cam, cam2=cam, bad=None, off=0):
        ptrs = [p] * 14
        if bad is not None:
            ptrs[bad] = None if off == 0 else p + off
        return L.xfh_sim3_solve_host(B, n1, M, ptrs[0], ptrs[1], ptrs[2], ptrs[3], tstride, ptrs[4], None if cam1 is None else C.byref(cam1),
                                     None if cam2 is None else C.byref(cam2), e1, e2, 0, mi, 0, ptrs[5], ptrs[6], iters, ptrs[7], dstride, rand_max, *ptrs[8:])
    bad = [hostcall(B=0), hostcall(B=65536), hostcall(n1=0), hostcall(n1=capi.GRID_MAX_N + 1), hostcall(M=0), hostcall(mi=-1), hostcall(e1=float("nan")),
           hostcall(e2=float("inf")), hostcall(rand_max=0), hostcall(iters=0), hostcall(iters=capi.SIM3_SOLVE_MAX_ITERS + 1), hostcall(B=2, dstride=5),
           hostcall(B=2, tstride=11), hostcall(cam1=None), hostcall(cam2=None)]
    bad += [hostcall(bad=k) for k in (0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13)] + [hostcall(bad=k, off=2) for k in (0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 12, 13)]
    bad += [hostcall(bad=8, off=8)]
    assert all(rc == 1 for rc in bad), bad
    assert hostcall() == 0 and hostcall(bad=5) == 0                         # the merge's count is optional
    assert L.xfh_sim3_solve_device(None, 1, 8, 8, p, p, p, p, 0, p, C.byref(cam), C.byref(cam), 9.0, 9.0, 0, 3, 0, None, p, 2, p, 0, 7, *([p] * 6)) == 1
    assert L.xfh_sim3_solve(None, 8, 8, p, p, p, p, p, C.byref(cam), C.byref(cam), 9.0, 9.0, 0, 3, p, 2, p, 7, *([p] * 5)) == 1
    assert L.xfh_sim3_solve_set(None, 7, 8, p) == 1 and L.xfh_sim3_solve_set(p, 0, 8, p) == 1 and L.xfh_sim3_solve_set(p, 7, 2, p) == 1
    assert L.xfh_sim3_solve_horn(None, p, 0, p) == 1 and L.xfh_sim3_solve_horn(p, p, 0, None) == 1
    assert L.xfh_sim3_solve_check(p, p, None, C.byref(cam), p, p, 9.0, 9.0, p, p) == 1 and L.xfh_sim3_solve_check(p, None, C.byref(cam), C.byref(cam), p, p, 9.0, 9.0, p, p) == 1
    assert L.xfh_sim3_solve_iterations_table(0.99, 15, 300, 8, None) == 1
    mh = lambda J=1, n1=8, n2=8, M=8, ptrs=(p,) * 6: L.xfh_sim3_merge_matches_host(J, n1, n2, M, *ptrs)
    assert [mh(J=0), mh(J=65536), mh(n1=0), mh(n2=0), mh(n2=capi.GRID_MAX_N + 1), mh(M=0)] == [1] * 6
    assert all(mh(ptrs=tuple(None if i == k else p for i in range(6))) == 1 for k in range(6)) and mh(ptrs=(p, p, p + 8, p, p, p)) == 1 and mh() == 0
    assert L.xfh_sim3_merge_matches_device(None, 1, 8, 8, 8, *([p] * 6)) == 1 and L.xfh_sim3_merge_matches(None, 1, 8, 8, 8, *([p] * 5)) == 1
    assert L.xfh_sim3_solve_workspace_bytes(0, 8, 1) == 0 and L.xfh_sim3_solve_workspace_bytes(8, 0, 1) == 0 and L.xfh_sim3_solve_workspace_bytes(8, 8, 65536) == 0
    assert L.xfh_sim3_solve_workspace_bytes(8, 8, 1) % 16 == 0 and L.xfh_sim3_solve_workspace_bytes(capi.GRID_MAX_N, 1 << 20, 8) > 0
    names = [L.xfh_kernel_name(capi.K[k]) for k in ("SIM3SOLVE_PREPARE", "SIM3SOLVE_FIT", "SIM3SOLVE_COUNT", "SIM3SOLVE_DECIDE", "SIM3SOLVE_MERGE")]
    assert names == [b"k_sim3solve_prepare", b"k_sim3solve_fit", b"k_sim3solve_count", b"k_sim3solve_decide", b"k_sim3merge"]
    assert capi.K["SIM3SOLVE_PREPARE"] == 45 and L.xfh_kernel_name(44) == b"k_twoview_final"                 # existing ids keep their values


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sim3solve") / "asan_sim3solve_test")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "xfeatslam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "asan_sim3solve_test.cpp"), "-o", exe])
    return exe


def test_rule_under_sanitizers_on_hostile_inputs(asan_exe):
    """a stand-alone program built from this repository's header alone with AddressSanitizer + UBSan: nothing of the library is linked, nothing
    runs on a GPU, nothing is loaded into Python"""
    r = subprocess.run([asan_exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "asan_sim3solve_test ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


def test_rule_under_sanitizers_equals_the_python_rule(asan_exe, tmp_path, scenes):
    s, want = scenes
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    for n, sc in s.items():
        n1, M, iters = len(sc["point1"]), len(sc["points"]), len(sc["draws"][0])
        with open(tmp_path / "in.bin", "wb") as f:
            f.write(struct.pack("<6i10f", n1, M, iters, G.RAND_MAX, sc["min_inliers"], int(sc["fix_scale"]), *[float(c) for c in sc["cam1"]], *[float(c) for c in sc["cam2"]], 9.0, 9.0))
            for a, dt in ((sc["points"], F), (sc["point1"], np.int32), (sc["matched"][0], np.int32), (sc["T1w"], F), (sc["T2w"][0], F), (sc["table"], np.int32),
                          (sc["draws"][0], np.int32)):
                f.write(np.ascontiguousarray(a, dt).tobytes())
        r = subprocess.run([asan_exe, "solve", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=env)
        assert r.returncode == 0, (n, r.stdout[-1000:], r.stderr[-3000:])
        w = want[n]
        sizes = dict(header=64, floats=128, inliers=n1, Tcw=48, Ow=12)
        blob = b"".join(b"\xa5" * sizes[k] if w[k] is None else np.ascontiguousarray(np.asarray(w[k], G.OUT_DTYPES[k])).tobytes() for k in R.OUTPUTS)
        assert open(tmp_path / "out.bin", "rb").read() == blob, n
    m = G.merge_scene()
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<4i", 3, 70, 80, m["M"]) + m["match12"].tobytes() + m["point2"].tobytes())
    r = subprocess.run([asan_exe, "merge", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    matched, kf, num = R.merge(m["match12"], m["point2"], m["M"])
    assert open(tmp_path / "out.bin", "rb").read() == matched.tobytes() + kf.tobytes() + struct.pack("<i", num)
