"""CPU tests of the MLPnP solver (xfh_mlpnp_*): the library's host code -- the very lines the kernels compile, mlpnp_math.h -- against the rule form of
tests/ref_mlpnp.py on the scenes of tests/mlpnp_rig.py (integers and flags equal, floats within one float32 step: the C library's libm and Python's
differ in last bits); each stateless piece against the rule; the iteration table against the literal SetRansacParameters; the order-free decision
and the stateless resume against the sequential loop with members of tests/ref_mlpnp_literal.py; the condition every GPU scene must satisfy (no
decision within reach of a libm's last bits); every refusal that needs no device; and the stand-alone sanitizer program.  No GPU is used."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import mlpnp_rig as G
import ref_mlpnp as R
import ref_mlpnp_literal as LIT
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NUDGE_ULP = 4          # no ulp bound for the fp64 device functions is documented in the toolkit's files: the fallback (profiles/mlpnp.md)


@pytest.fixture(scope="module")
def scenes():
    """the rig's scenes and the rule's answer for each, with every inlier test and Gauss-Newton decision traced: computed once, never changed"""
    s = G.rig()
    s["family"], s["hostile"] = G.family(), G.hostile()
    want, traces = {}, {}
    for k, v in s.items():
        R.trace = []
        try:
            want[k] = [G.rule_of(v, b) for b in range(len(v["assigned"]))]
            traces[k] = R.trace
        finally:
            R.trace = None
    return s, want, traces


def test_host_form_equals_the_rule_and_every_status_is_reached(scenes):
    s, want, _ = scenes
    seen = set()
    for name, sc in s.items():
        B, n = sc["assigned"].shape
        prior = dict(Tcw=np.full((B, 12), -2.0, F), inliers=np.full((B, n), 9, np.uint8), assigned_out=np.full((B, n), 77, np.int32))
        got = G.host_of(sc, prior=prior)
        for b in range(B):
            G.assert_equals_rule(got, want[name][b], b)
            for k, v in prior.items():                                      # what the call leaves alone comes back as it was
                if want[name][b][k] is None:
                    assert np.array_equal(got[k][b], v[b]), (name, k)
            seen.add(int(want[name][b]["header"][1]))
        if name in G.EXPECT:
            assert R.STATUS[want[name][0]["header"][1]] == G.EXPECT[name], (name, dict(zip(R.HEADER, want[name][0]["header"].tolist())))
    assert seen == {0, 1, 2, 3}


def test_conditions_of_the_scenes(scenes):
    """what each scene is in the rig for"""
    s, want, _ = scenes
    h = lambda name, b=0: dict(zip(R.HEADER, want[name][b]["header"].tolist()))
    for name, its in G.ITS.items():
        assert h(name)["its"] == its, name
    assert h("n70")["N"] == 41 and h("n300")["N"] == 261 and h("n9")["N"] == 9 and h("n5")["N"] == 5
    g = h("n_equals_min")                                                   # table entry 1, the loop still runs chunk = 5, and 10 > 10 never holds
    assert g["N"] == 10 == g["min_inliers"] and g["its"] == 1 and g["consumed"] == 5 and g["best_count"] == 10 and g["refines"] == 1
    assert h("none")["consumed"] == 35 and h("none")["best"] == -1
    for name, size in G.REFINE_SETS.items():                                 # the Refine that wins runs on exactly that many inliers
        r = want[name][0]
        assert r["counts"][h(name)["best"]] == size and h(name)["best"] in r["refined"], name
    assert h("planar")["planar"] == 1 and any(pl for _, pl in want["planar"][0]["hyps"]) and not all(pl for _, pl in want["planar"][0]["hyps"])
    sc, r = s["behind"], want["behind"][0]                                   # an inlier behind the camera
    T = r["Tcw"].astype(np.float64).reshape(3, 4)
    z = [T[2, :3] @ sc["points"][0, sc["assigned"][0, i]].astype(np.float64) + T[2, 3] for i in np.nonzero(r["inliers"])[0]]
    assert min(z) < 0 < max(z)
    assert [h("family", b)["status"] for b in range(3)] == [R.REFINED, R.NONE, R.TOO_FEW]
    for name in G.REFINE_SETS:                                               # noise-free scenes: the reported pose is the camera pose the scene was made with
        Rm, t = s[name]["poses"][0]
        T = want[name][0]["Tcw"].astype(np.float64).reshape(3, 4)
        assert np.abs(T[:, :3] - Rm).max() < 1e-4 and np.abs(T[:, 3] - t).max() < 1e-4, (name, T, Rm, t)
    assert h("hostile")["N"] == 39                                            # the two indices of +-2^31 are no correspondences


def test_rig_condition_no_decision_hangs_on_a_libm(scenes):
    """Every libm result nudged NUDGE_ULP up, then down: identical headers and flags, Tcw within one float32 step; no inlier test of any iteration or
    Refine within 64 float32 steps of max_err; no :744 / :748 decision within a relative 1e-6 of its bound.  A scene that fails is replaced by
    another seed in tests/mlpnp_rig.py, never exempted."""
    s, want, traces = scenes
    base = dict(R.LIBM)
    try:
        for sign in (+1, -1):
            R.LIBM.update({k: (lambda x, f=f: float(np.float64(f(x)) + sign * NUDGE_ULP * np.spacing(np.float64(f(x))))) for k, f in base.items()})
            for name, sc in s.items():
                for b in range(len(sc["assigned"])):
                    r, w = G.rule_of(sc, b), want[name][b]
                    assert np.array_equal(r["header"], w["header"]), (name, b, sign)
                    for k in ("inliers", "assigned_out"):
                        assert (w[k] is None and r[k] is None) or np.array_equal(r[k], w[k]), (name, b, k, sign)
                    if w["Tcw"] is not None:
                        assert G.float_steps(r["Tcw"], w["Tcw"]).max() <= 1, (name, b, sign)
    finally:
        R.LIBM.update(base)
    for name, tr in traces.items():
        e = np.array([v for k, v, _ in tr if k == "inlier"], F)
        bound = np.array([bd for k, _, bd in tr if k == "inlier"], F)
        ok = ~np.isnan(e)
        assert len(e) == 0 or G.float_steps(e[ok], bound[ok]).min() >= 64, (name, "an inlier test within 64 float32 steps of max_err")
        for kind in ("gn744", "gn748"):
            for k, v, bd in tr:
                if k == kind and v == v:
                    assert abs(v - bd) > 1e-6 * bd, (name, kind, v, bd)


def test_iteration_table_equals_the_literal_set_ransac_parameters():
    for eps in (0.5, 0.2, 0.9):
        ti, tm = Context.mlpnp_iterations_table(400, 0.99, 10, 300, 6, eps)
        ri, rm = R.iterations_table(400, 0.99, 10, 300, 6, eps)
        assert np.array_equal(ti, ri) and np.array_equal(tm, rm)
        for N in range(1, 401):
            lit = LIT.set_ransac_parameters(N, 0.99, 10, 300, 6, eps)
            assert (int(ti[N]), int(tm[N])) == (300 if lit[0] is None else lit[0], lit[1]), (eps, N)         # the stated cap where the reference's cast is undefined
    ti, tm = Context.mlpnp_iterations_table(60)
    assert ti[10] == 1 and tm[10] == 10 and ti[41] == 35 and tm[41] == 20 and tm[5] == 10 and ti[0] == 300     # N == minInliers; the cap where the double is not finite
    assert Context.mlpnp_iterations_table(41, eps=0.4)[0][41] == 70 and Context.mlpnp_iterations_table(41, eps=0.85)[0][41] == 5


def test_order_free_decision_and_stateless_resume_equal_the_loop_with_members():
    """200 random scenes, chunk 1 / 5 / 20, up to three resumed calls: the rule called with start_iter = the previous call's consumed count against ONE
    literal solver object that keeps mnIterations, mnBestInliers and the best flags across its iterate() calls"""
    rng = np.random.RandomState(7)
    statuses, resumed = set(), 0
    for k in range(200):
        N = int(rng.randint(12, 30))
        sc = G.scene(5000 + k, n=N + int(rng.randint(0, 8)), N=N, inlier_frac=float(rng.uniform(0.3, 1.0)), noise=float(rng.choice([0.0, 0.5, 1.5])), max_iters=12, invalid=1)
        cache = {}
        first = G.rule_of(sc, cache=cache, chunk=1)
        if first["header"][1] == R.TOO_FEW:
            continue
        N_, its, min_eff = int(first["header"][0]), int(first["header"][2]), int(first["header"][3])
        for chunk in (1, 5, 20):
            lit = LIT.Solver(N_, its, min_eff, lambda i: cache["fits"][i][2], lambda i: sum(cache["refined"][i][2]), 12)
            start = 0
            for call in range(4):
                r = G.rule_of(sc, cache=cache, chunk=chunk, start_iter=start)
                h = dict(zip(R.HEADER, r["header"].tolist()))
                ret, no_more, n_inl, at = lit.iterate(chunk)
                want = R.REFINED if ret and not no_more else (R.BEST if ret else R.NONE)
                assert (h["status"], h["winner"], h["n_inliers"], h["consumed"]) == (want, at, n_inl, lit.mnIterations), (k, chunk, call, h)
                assert (h["best"], h["best_count"]) == (lit.best, lit.mnBestInliers), (k, chunk, call, h)
                statuses.add(h["status"])
                if no_more:
                    break
                start, resumed = h["consumed"], resumed + 1
    assert statuses == {R.NONE, R.BEST, R.REFINED} and resumed > 100


def test_pieces_equal_the_rule(scenes):
    s, want, _ = scenes
    rng = np.random.RandomState(3)
    for _ in range(300):                                                      # the set: the shrinking vector, draws out of range included
        N = int(rng.randint(6, 50))
        d = rng.randint(0, 32768, 6)
        if rng.rand() < 0.2:
            d[rng.randint(6)] = rng.choice([-5, 2 ** 31 - 1, -2 ** 31, 40000])
        got = Context.mlpnp_set(d, 32767, N)
        assert got.tolist() == R.make_set(d, 32767, N) and len(set(got.tolist())) == 6
    for _ in range(100):                                                      # the basis: equal to the rule, orthonormal, orthogonal to f
        f = [float(F(rng.uniform(-1, 1))), float(F(rng.uniform(-1, 1))), 1.0]
        r, sv = Context.mlpnp_nullspace(f)
        rr, rs = R.nullspace(f)
        assert r.tolist() == rr and sv.tolist() == rs
        assert abs(r @ f) < 1e-15 and abs(sv @ f) < 1e-15 and abs(r @ sv) < 1e-15 and abs(r @ r - 1) < 1e-15 and abs(sv @ sv - 1) < 1e-15
    cam = G.camera()
    for name in ("n70", "planar", "refine65"):
        sc, w = s[name], want[name][0]
        idx = np.nonzero(sc["assigned"][0] >= 0)[0]
        idx = [i for i in idx if sc["assigned"][0, i] < sc["points"].shape[1] and sc["valid"][0, sc["assigned"][0, i]]]
        f = np.array([R.bearing(sc["cam"], *sc["xy"][i]) for i in idx], F)
        p = sc["points"][0, sc["assigned"][0, idx]]
        fd, pd = [[float(v) for v in row] for row in f], [[float(v) for v in row] for row in p]
        rs = [R.nullspace(row) for row in fd]
        st = R.make_set(sc["draws"][0][0], G.RAND_MAX, len(idx))
        Rt, pl = Context.mlpnp_compute_pose(f[st], p[st])
        wRt, wpl = R.compute_pose(list(range(6)), [fd[c] for c in st], [pd[c] for c in st], [rs[c] for c in st], False)
        assert pl == wpl and np.allclose(Rt.ravel(), wRt, rtol=0, atol=1e-9 * max(1.0, np.abs(wRt).max())), name
        use = w["inliers"][idx]
        Rt, pl = Context.mlpnp_compute_pose(f, p, use, fold=True)
        wRt, wpl = R.compute_pose([c for c in range(len(idx)) if use[c]], fd, pd, rs, True)
        assert pl == wpl and np.allclose(Rt.ravel(), wRt, rtol=0, atol=1e-9 * max(1.0, np.abs(wRt).max())), name
        for c in range(len(idx)):
            e, inl = Context.mlpnp_check(np.array(wRt), cam, p[c], sc["xy"][idx[c]], sc["max_err"])
            we, winl = R.check(wRt, sc["cam"], p[c], sc["xy"][idx[c]], sc["max_err"])
            assert inl == winl and G.float_steps(e, we).max() == 0, (name, c)


def test_closed_form_jacobian_equals_central_differences():
    """step 5 (g): the rows of the rule's Jacobian against (r(x + h) - r(x - h)) / 2h of its own residuals, h = 1e-6, at random poses and points"""
    rng = np.random.RandomState(11)
    for _ in range(50):
        x = [float(v) for v in np.concatenate([rng.uniform(-0.8, 0.8, 3), rng.uniform(-2, 2, 3)])]
        X = [float(v) for v in (rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(3, 9))]
        r, sv = R.nullspace([float(rng.uniform(-0.6, 0.6)), float(rng.uniform(-0.4, 0.4)), 1.0])
        _, J = R.gn_rows(R.gn_begin(x), X, r, sv)
        for k in range(6):
            xp, xm = list(x), list(x)
            xp[k] += 1e-6; xm[k] -= 1e-6
            a, _ = R.gn_rows(R.gn_begin(xp), X, r, sv)
            b, _ = R.gn_rows(R.gn_begin(xm), X, r, sv)
            for row in range(2):
                assert abs((a[row] - b[row]) / 2e-6 - J[6 * row + k]) < 1e-8, (x, X, k, row)


def test_gating_by_the_bow_match_count(scenes):
    s, want, _ = scenes
    sc = s["n70"]
    few = G.host_of(sc, n_matches=[14], min_matches=15, prior=dict(Tcw=np.full(12, 3.0, F)))
    assert few["header"][0].tolist() == [41, R.TOO_FEW, 0, 0, -1, 0, -1] + [0] * 9 and np.all(few["Tcw"] == 3.0)
    G.assert_equals_rule(G.host_of(sc, n_matches=[15], min_matches=15), want["n70"][0], 0)
    assert G.rule_of(sc, n_matches=14, min_matches=15)["header"].tolist() == few["header"][0].tolist()


def test_refusals_without_a_device_and_kernel_names():
    L = capi.lib()
    cam = G.camera()
    a = np.zeros(1 << 17, np.float64)
    p = a.ctypes.data

    def hostcall(B=1, n=8, nq=8, err=5.991, chunk=5, iters=2, dstride=0, rand_max=7, camera=cam, bad=None, off=0):
        ptrs = [p] * 13                      # xy assigned points valid | n_matches iters mins | start | draws | ws header Tcw inliers assigned_out
        if bad is not None:
            ptrs[bad] = None if off == 0 else p + off
        return L.xfh_mlpnp_solve_host(B, n, nq, ptrs[0], ptrs[1], ptrs[2], ptrs[3], None if camera is None else C.byref(camera), err, 0, ptrs[4], ptrs[5], ptrs[6],
                                      chunk, ptrs[7], iters, ptrs[8], dstride, rand_max, *ptrs[9:], p)
    bad = [hostcall(B=0), hostcall(B=65536), hostcall(n=0), hostcall(n=capi.GRID_MAX_N + 1), hostcall(nq=0), hostcall(nq=(1 << 24) + 1), hostcall(err=float("nan")),
           hostcall(err=float("inf")), hostcall(chunk=-1), hostcall(rand_max=0), hostcall(iters=0), hostcall(iters=capi.MLPNP_MAX_ITERS + 1),
           hostcall(B=2, dstride=11), hostcall(camera=None)]
    bad += [hostcall(bad=k) for k in (0, 1, 2, 5, 6, 8, 9, 10, 11, 12)] + [hostcall(bad=k, off=2) for k in (0, 1, 2, 4, 5, 6, 7, 8, 10, 11)] + [hostcall(bad=9, off=8)]
    assert all(rc == 1 for rc in bad), bad
    assert hostcall() == 0 and hostcall(bad=3) == 0 and hostcall(bad=4) == 0 and hostcall(bad=7) == 0 and hostcall(B=2, dstride=12) == 0     # the optional pointers
    assert L.xfh_mlpnp_solve_device(None, 1, 8, 8, p, p, p, p, C.byref(cam), 5.991, 0, None, p, p, 5, None, 2, p, 0, 7, *([p] * 5)) == 1
    assert L.xfh_mlpnp_solve(None, 8, 8, p, p, p, p, C.byref(cam), 5.991, p, p, 5, 0, 2, p, 7, *([p] * 4)) == 1
    assert L.xfh_mlpnp_set(None, 7, 8, p) == 1 and L.xfh_mlpnp_set(p, 0, 8, p) == 1 and L.xfh_mlpnp_set(p, 7, 5, p) == 1
    assert L.xfh_mlpnp_nullspace(None, p) == 1 and L.xfh_mlpnp_nullspace(p, None) == 1
    assert L.xfh_mlpnp_compute_pose(5, p, p, None, 0, p, p) == 1 and L.xfh_mlpnp_compute_pose(6, None, p, None, 0, p, p) == 1
    none = np.zeros(8, np.uint8)
    assert L.xfh_mlpnp_compute_pose(8, p, p, none.ctypes.data, 1, p, p) == 1    # no point in use
    assert L.xfh_mlpnp_check(p, None, p, p, 5.991, p, p) == 1 and L.xfh_mlpnp_check(None, C.byref(cam), p, p, 5.991, p, p) == 1
    assert L.xfh_mlpnp_iterations_table(0.99, 10, 300, 6, 0.5, 8, None, p) == 1 and L.xfh_mlpnp_iterations_table(0.99, 10, 300, 5, 0.5, 8, p, p) == 1     # min_set != 6
    assert L.xfh_mlpnp_iterations_table(0.99, 10, 300, 6, 1.5, 8, p, p) == 1 and L.xfh_mlpnp_iterations_table(0.99, 10, 300, 6, float("nan"), 8, p, p) == 1
    assert L.xfh_mlpnp_workspace_bytes(0, 8, 1, 4) == 0 and L.xfh_mlpnp_workspace_bytes(8, 0, 1, 4) == 0 and L.xfh_mlpnp_workspace_bytes(8, 8, 65536, 4) == 0
    assert L.xfh_mlpnp_workspace_bytes(8, 8, 1, 0) == 0 and L.xfh_mlpnp_workspace_bytes(8, 8, 1, capi.MLPNP_MAX_ITERS + 1) == 0
    assert L.xfh_mlpnp_workspace_bytes(8, 8, 1, 4) % 16 == 0 and L.xfh_mlpnp_workspace_bytes(capi.GRID_MAX_N, 1 << 20, 8, capi.MLPNP_MAX_ITERS) > 0
    names = [L.xfh_kernel_name(capi.K[k]) for k in ("MLPNP_PREPARE", "MLPNP_FIT", "MLPNP_COUNT", "MLPNP_RECORDS", "MLPNP_REFINE", "MLPNP_DECIDE")]
    assert names == [b"k_mlpnp_prepare", b"k_mlpnp_fit", b"k_mlpnp_count", b"k_mlpnp_records", b"k_mlpnp_refine", b"k_mlpnp_decide"]
    assert capi.K["MLPNP_PREPARE"] == 50 and L.xfh_kernel_name(49) == b"k_sim3merge"                       # existing ids keep their values


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mlpnp") / "asan_mlpnp_test")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "xfeatslam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "asan_mlpnp_test.cpp"), "-o", exe])
    return exe


def test_rule_under_sanitizers_on_hostile_inputs(asan_exe):
    """a stand-alone program built from this repository's header alone with AddressSanitizer + UBSan: nothing of the library is linked, nothing
    runs on a GPU, nothing is loaded into Python"""
    r = subprocess.run([asan_exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "asan_mlpnp_test ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


def test_rule_under_sanitizers_equals_the_python_rule(asan_exe, tmp_path, scenes):
    s, want, _ = scenes
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    for name, sc in s.items():
        n, nq, iters = sc["assigned"].shape[1], sc["points"].shape[1], sc["draws"].shape[1]
        with open(tmp_path / "in.bin", "wb") as f:
            f.write(struct.pack("<7i5f", n, nq, iters, G.RAND_MAX, sc["chunk"], 0, 1, *[float(c) for c in sc["cam"]], sc["max_err"]))
            for a, dt in ((sc["xy"], F), (sc["assigned"][0], np.int32), (sc["points"][0], F), (sc["valid"][0], np.uint8), (sc["tables"][0], np.int32),
                          (sc["tables"][1], np.int32), (sc["draws"][0], np.int32)):
                f.write(np.ascontiguousarray(a, dt).tobytes())
        r = subprocess.run([asan_exe, "solve", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=env)
        assert r.returncode == 0, (name, r.stdout[-1000:], r.stderr[-3000:])
        raw = np.frombuffer(open(tmp_path / "out.bin", "rb").read(), np.uint8)
        cut = {"header": raw[:64].view(np.int32)[None], "Tcw": raw[64:112].view(F)[None], "inliers": raw[112:112 + n][None], "assigned_out": raw[112 + n:].view(np.int32)[None]}
        G.assert_equals_rule(cut, want[name][0], 0, prior_byte=0xA5)
