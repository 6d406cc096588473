"""xfh_sim3_optimize_host and the piece functions of the OptimizeSim3 call against the Python rule (tests/ref_optsim3.py), without a GPU: by bits
where no libm enters, otherwise within one double step; the numeric Jacobian against a closed form; hand-made cases; every class of refusal; the
sanitizer program; and the condition the rig's scenes must hold for the GPU comparison to be a fair one."""
import ctypes as C
import math
import os
import subprocess
import warnings

import numpy as np
import pytest

import optsim3_rig as G
import ref_optsim3 as R
from xfeatslam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64
INVALID = 1


@pytest.fixture(scope="module")
def L():
    return capi.lib()


def dptr(a):
    return a.ctypes.data


def steps64(a, b):
    """distance in double steps, elementwise (finite values)"""
    a, b = np.asarray(a, D).reshape(-1), np.asarray(b, D).reshape(-1)
    ia, ib = a.view(np.int64), b.view(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffffffffffff), ia), np.where(ib < 0, -(ib & 0x7fffffffffffffff), ib)
    return np.abs(ia - ib)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def random_state(rng, scale=True):
    return R.oplus(np.r_[rng.uniform(-1.5, 1.5, 3), rng.uniform(-2, 2, 3), rng.uniform(-0.4, 0.4) if scale else 0.0], [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], 0)


# ---- the pieces -----------------------------------------------------------------------------------------------------------------------------------
def test_state_map_and_oplus_against_the_rule(L):
    rng = np.random.RandomState(1)
    for n in range(200):
        st = np.array(random_state(rng), D)
        S13 = R.state_to(list(st))
        back, got13 = np.zeros(8, D), np.zeros(13, F)
        assert L.xfh_sim3_state_to(dptr(st), dptr(got13)) == 0 and same_bits(got13, S13)          # products and sums only: by bits
        assert L.xfh_sim3_state_from(dptr(S13), dptr(back)) == 0
        assert steps64(back, R.state_from(S13)).max() <= 1                                        # sqrt
        X, out = rng.uniform(-5, 5, 3), np.zeros(3, D)
        assert L.xfh_sim3_map(dptr(st), dptr(X), dptr(out)) == 0 and same_bits(out, np.array(R.smap(list(st), list(X)), D))
        assert L.xfh_sim3_inverse_map(dptr(st), dptr(X), dptr(out)) == 0 and same_bits(out, np.array(R.smap(R.inverse(list(st)), list(X)), D))
        # all four branches of the exponential: tiny / ordinary rotation x tiny / ordinary log-scale, and the 1e-9 steps of the numeric Jacobian
        w = rng.uniform(-1, 1, 3) * (1e-7 if n % 2 else 0.3)
        u = np.r_[w, rng.uniform(-1, 1, 3), rng.uniform(-1, 1) * (1e-7 if (n // 2) % 2 else 0.2)]
        if n % 10 == 9:
            u = np.zeros(7); u[n % 7] = 1e-9 * (-1) ** n
        for fix in (0, 1):
            o = np.zeros(8, D)
            assert L.xfh_sim3_oplus(dptr(st), dptr(u), fix, dptr(o)) == 0
            ref = np.array(R.oplus(u, list(st), fix), D)
            assert steps64(o, ref).max() <= 1, (n, fix, o, ref)
            if fix:
                assert o[7] == st[7]                                                               # u[6] = 0: the scale is multiplied by exp(0)


def test_solve7_against_the_rule_by_bits(L):
    rng = np.random.RandomState(2)
    for n in range(100):
        A = rng.randn(9, 7)
        M = A.T @ A
        if n % 5 == 4:
            M[6, :] = M[:, 6] = 0.0                                       # fix_scale: row and column 6 are zero, H_66 is lambda alone
        H = np.array([M[i, j] for i in range(7) for j in range(i, 7)], D)
        b, lam = rng.randn(7), 10.0 ** rng.uniform(-6, 1)
        x = np.full(7, 7.0)
        ok = L.xfh_sim3_solve7(dptr(H), lam, dptr(b), dptr(x))
        rok, rx, _ = R.ldlt_solve(H, lam, b, [7.0] * 7)
        assert ok == int(rok) == 1 and same_bits(x, np.array(rx, D))
    H = np.zeros(28)
    H[0] = -1.0
    x = np.full(7, 7.0)
    assert L.xfh_sim3_solve7(dptr(H), 0.5, dptr(np.ones(7)), dptr(x)) == 0 and np.all(x == 7.0)      # a pivot that is not > 0: x untouched
    H[0] = np.nan
    assert L.xfh_sim3_solve7(dptr(H), 0.5, dptr(np.ones(7)), dptr(x)) == 0 and np.all(x == 7.0)


def edge_inputs(rng, fix):
    st = random_state(rng, scale=not fix)
    P2 = np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(2, 9)], F)
    P1 = np.array(R.smap(st, [float(v) for v in P2]), D).astype(F)
    if P1[2] < 0.5:
        return None
    fx, fy, cx, cy = G.CAM
    o1 = np.array([fx * P1[0] / P1[2] + cx, fy * P1[1] / P1[2] + cy], F) + rng.randn(2).astype(F) * 2
    o2 = np.array([fx * P2[0] / P2[2] + cx, fy * P2[1] / P2[2] + cy], F) + rng.randn(2).astype(F) * 2
    return st, P1, P2, o1, o2


def call_edge(L, st, P1, P2, o1, o2, fix, robust, w=(1.0, 1.0)):
    cam = G.cam_struct()
    e, c, J, r1 = np.zeros(4, D), np.zeros(2, D), np.zeros(28, D), np.zeros(2, D)
    s8 = np.array(st, D)
    assert L.xfh_sim3_edge(dptr(s8), C.byref(cam), C.byref(cam), dptr(P1), dptr(P2), dptr(o1), dptr(o2), w[0], w[1], G.TH2, fix, robust, dptr(e), dptr(c), dptr(J),
                           dptr(r1)) == 0
    return e, c, J, r1


def test_edge_against_the_rule(L):
    """errors, chi2 and rho by bits (products, sums, one division per coordinate; sqrt is correctly rounded everywhere); the numeric Jacobian by bits
    as well on this host, where the rule's exp is the library's exp -- its entries are differences of errors divided by 2e-9, so one double step
    in a perturbed similarity would be about 1e-7 relative in an entry, which is why no tighter statement than `the same lines` can be made of it"""
    rng = np.random.RandomState(3)
    cam, n = R.cam_of(G.CAM), 0
    while n < 100:
        fix = n % 2
        got = edge_inputs(rng, fix)
        if got is None:
            continue
        n += 1
        st, P1, P2, o1, o2 = got
        w = (1.0, 0.69444) if n % 3 else (1.0, 1.0)
        e, c, J, r1 = call_edge(L, st, P1, P2, o1, o2, fix, 1, w)
        w = [float(F(v)) for v in w]
        X1, X2 = [float(v) for v in P1], [float(v) for v in P2]
        e12, c12 = R.edge_error(st, cam, X2, [float(v) for v in o1], w[0])
        e21, c21 = R.edge_error(R.inverse(st), cam, X1, [float(v) for v in o2], w[1])
        assert same_bits(e, np.array(e12 + e21, D)) and same_bits(c, np.array([c12, c21], D))
        pert, pinv = R.perturbed(st, fix)
        Jr = R.edge_jacobian(pert, cam, X2, [float(v) for v in o1]) + R.edge_jacobian(pinv, cam, X1, [float(v) for v in o2])
        assert same_bits(J, np.array(Jr, D)), (n, J - np.array(Jr))
        delta = float(F(math.sqrt(F(G.TH2))))
        assert same_bits(r1, np.array([float(R.huber(D(c12), delta)[1]), float(R.huber(D(c21), delta)[1])], D))
        if fix:
            assert J[6] == 0.0 and J[13] == 0.0 and J[20] == 0.0 and J[27] == 0.0               # column 6 is exactly zero under fix_scale
        assert np.all(call_edge(L, st, P1, P2, o1, o2, fix, 0, w)[3] == 1.0)


def closed_form_jacobian(st, cam, X1, X2):
    """d e12 / d u and d e21 / d u for the update exp(u) * S, u = (omega, upsilon, sigma).  p = S.map(X2): to first order exp(u) moves it by omega x p +
    upsilon + sigma p, so dp/du = [-[p]x | I | p].  p' = S^-1.map(X1) and (exp(u) S)^-1 = S^-1 exp(-u), so dp'/du = -(1/s) R^T [-[X1]x | I | X1].
    e = obs - project(p): de/dp = -[[fx/z, 0, -fx x/z^2], [0, fy/z, -fy y/z^2]]."""
    def skew(v):
        return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], D)

    def dproj(p):
        return np.array([[cam[0] / p[2], 0, -cam[0] * p[0] / p[2] ** 2], [0, cam[1] / p[2], -cam[1] * p[1] / p[2] ** 2]], D)
    Rm = np.array(R.RP.matrix_from_quat(st[:4]), D).reshape(3, 3)
    p = np.array(R.smap(st, X2), D)
    J12 = -dproj(p) @ np.hstack([-skew(p), np.eye(3), p[:, None]])
    pi = np.array(R.smap(R.inverse(st), X1), D)
    X1 = np.array(X1, D)
    J21 = -dproj(pi) @ (-(1.0 / st[7]) * Rm.T @ np.hstack([-skew(X1), np.eye(3), X1[:, None]]))
    return J12, J21, p, pi


def test_numeric_jacobian_against_closed_form(L):
    """The bound.  Column d is (e(+) - e(-)) / (2 delta), delta = 1e-9.  Truncation: the central difference drops the third-order term, delta^2 / 6
    times a third derivative that is a few times the first for these points (depth >= 0.5, |u| < 1): below 1e-17 relative, nothing.  Rounding: each
    e(+/-) = obs - (f x / z + c) is computed from a perturbed similarity whose entries carry their own rounding; every one of the K <= 16 roundings
    between the update vector and the error is relative to a magnitude of at most M = max(|obs|, |f x / z| + |c|, f |p| / z) pixels, so an error is off
    by at most K eps M and a column entry by 2 K eps M / (2 delta) = K eps M / delta.  With eps = 2^-52 and M as measured per pair that is about
    16 * 2.2e-16 * 1e3 / 1e-9 = 3.6e-3 on entries of size 1e2 .. 1e4: 1e-7 relative, the noise the contract names.  The noise is measured too: the
    worst entry must also be ABOVE 1e-3 of the bound somewhere, or the bound is not about this Jacobian."""
    rng = np.random.RandomState(4)
    cam, eps, K, n, worst = R.cam_of(G.CAM), 2.0 ** -52, 16, 0, 0.0
    while n < 200:
        got = edge_inputs(rng, 0)
        if got is None:
            continue
        st, P1, P2, o1, o2 = got
        X1, X2 = [float(v) for v in P1], [float(v) for v in P2]
        J12, J21, p, pi = closed_form_jacobian(st, cam, X1, X2)
        if pi[2] < 0.5:
            continue
        n += 1
        _, _, J, _ = call_edge(L, st, P1, P2, o1, o2, 0, 0)
        for Jn, Jc, q, obs in ((J[:14].reshape(2, 7), J12, p, o1), (J[14:].reshape(2, 7), J21, pi, o2)):
            M = max(float(np.abs(obs).max()), cam[0] * abs(q[0] / q[2]) + cam[2], cam[1] * abs(q[1] / q[2]) + cam[3], cam[0] * float(np.linalg.norm(q)) / q[2])
            bound = K * eps * M / R.DELTA + 1e-12 * float(np.abs(Jc).max())
            err = float(np.abs(Jn - Jc).max())
            assert err <= bound, (n, err, bound, Jn, Jc)
            worst = max(worst, err / bound)
    print(f"numeric Jacobian: worst error / bound {worst:.3f}")
    assert worst > 1e-3


# ---- the host form ----------------------------------------------------------------------------------------------------------------------------------
OUT_KEYS = ("assigned_out", "status", "chi2", "state", "S12_out", "Tcw", "Ow", "header")


def assert_same_result(a, b, tag):
    """host form against rule: every output by bits (a NaN compares by position: its payload is not the rule's business)"""
    for k in OUT_KEYS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), (tag, k, x, y)
    fa, fb = a["final_chi2"], b["final_chi2"]
    assert fa == fb or (fa != fa and fb != fb), (tag, fa, fb)


@pytest.mark.parametrize("name", list(G.SCENES))
def test_host_form_against_the_rule(L, name):
    """The fold, the edge arithmetic, the solve and the classifications are libm-free; exp / sin / cos enter through the update alone, where this
    host's libm is the rule's.  So the comparison is by bits, trajectory included."""
    p = G.scene(name)
    h, = G.run_host([p], L=L)
    assert_same_result(h, R.rule(p), name)


def test_host_form_batch_and_shared_side(L):
    ps = G.batch([G.scene(n) for n in G.BATCH3])
    alone = [G.run_host([p], L=L)[0] for p in ps]
    for a, b in zip(G.run_host(ps, L=L), alone):
        assert_same_result(a, b, "batch")
    assert [int(r["header"][7]) for r in alone] == [2, 1, 2]            # the middle one returns early
    shared = [dict(p, **{k: ps[0][k] for k, _ in G.SIDE1}) for p in ps]
    for a, b in zip(G.run_host(shared, side1_shared=True, L=L), G.run_host(shared, L=L)):
        assert_same_result(a, b, "shared")


# ---- hand-made cases ----------------------------------------------------------------------------------------------------------------------------------
def test_early_return_leaves_the_state_at_the_input(L):
    p = G.scene("keep9")
    h, = G.run_host([p], L=L)
    assert h["header"][:8].tolist() == [12, 12, 0, 3, 0, 10, 0, 1]      # 12 pairs, 3 bad, n_more 10, returns 0 after one classification
    assert same_bits(h["state"], np.array(R.state_from(p["S12"]), D))   # g2oS12 is not written before :2378
    assert same_bits(h["S12_out"], R.state_to(R.state_from(p["S12"])))
    assert (h["status"] == R.BAD_FIRST).sum() == 3 and (h["status"] == R.INLIER).sum() == 9 and (h["status"] == R.BAD_FINAL).sum() == 0
    assert np.all(h["assigned_out"][h["status"] == R.BAD_FIRST] == -1)  # the bad matches are already removed
    keep = h["status"] != R.BAD_FIRST
    assert np.array_equal(h["assigned_out"][keep], p["assigned"][keep])
    assert h["header"][8] > 0                                           # round 1 did run
    p10 = G.scene("keep10")
    h10, = G.run_host([p10], L=L)
    assert h10["header"][:8].tolist() == [13, 13, 0, 3, 0, 10, 10, 2] and not same_bits(h10["state"], np.array(R.state_from(p10["S12"]), D))


def test_pair_bad_in_one_direction_only(L):
    """Thirty exact pairs at the true similarity, and one whose keypoint in KF2 is 5 px to the right of where its point projects: at the truth e21 =
    (5, 0) and chi2_21 = 25 > 10 while e12 = 0.  The Huber kernel weighs that edge by sqrt(10) / 5, the other 60 edges pull back, so the estimate
    moves by a small fraction of a pixel: the pair leaves in the first classification on chi2_21 alone."""
    p = G.make(seed=21, n_pairs=31, n1=64, noise=0.0, start=(0.0, 0.0, 0.0))
    i = int(np.nonzero((p["assigned"] >= 0))[0][0])
    k2 = p["index2"][p["assigned"][i]]
    p["xy_un2"][k2, 0] += 5.0
    h, = G.run_host([p], L=L)
    assert h["status"][i] == R.BAD_FIRST and h["assigned_out"][i] == -1
    assert h["chi2"][i, 0] < 1.0 and 20.0 < h["chi2"][i, 1] < 25.5, h["chi2"][i]
    assert h["header"][:8].tolist() == [31, 31, 0, 1, 0, 10, 30, 2]
    p["xy_un2"][k2, 0] -= 5.0                                            # the other direction: the keypoint in KF1
    p["xy_un1"][i, 1] -= 5.0
    h, = G.run_host([p], L=L)
    assert h["status"][i] == R.BAD_FIRST and 20.0 < h["chi2"][i, 0] < 25.5 and h["chi2"][i, 1] < 1.0, h["chi2"][i]


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------
def host_args(p, ws, outs):
    """the argument list of xfh_sim3_optimize_host for one problem as a dict in call order"""
    c1, c2 = G.cam_struct(), G.cam_struct()
    a = dict(B=1, n1=len(p["assigned"]), M1=len(p["points1"]), nq=len(p["points2"]), n2=len(p["xy_un2"]), side1_shared=0)
    for k, dt in G.SIDE1 + G.SIDE2:
        a[k] = np.ascontiguousarray(np.asarray(p[k], dt))
    a.update(S12=np.asarray(p["S12"], F), S12_stride=13, Tmw=np.asarray(p["Tmw"], F), cam1=c1, cam2=c2, th2=p["th2"], fix_scale=0, all_points=0, w1=1.0, w2=1.0, ws=ws)
    a.update(assigned_out=outs[0], status=outs[1], chi2=outs[2], state=outs[3], S12_out=outs[4], S12_out_stride=13, Tcw=outs[5], Ow=outs[6], header=outs[7],
             final_chi2=outs[8])
    return a


def call_host(L, a):
    def conv(k, v):
        if isinstance(v, np.ndarray):
            return v.ctypes.data
        if k in ("cam1", "cam2"):
            return None if v is None else C.byref(v)
        return v
    return L.xfh_sim3_optimize_host(*[conv(k, v) for k, v in a.items()])


def test_refusals(L):
    p = G.scene("clean30")
    n1 = len(p["assigned"])
    outs = [np.zeros(n1, np.int32), np.zeros(n1, np.uint8), np.zeros(2 * n1, F), np.zeros(8, D), np.zeros(13, F), np.zeros(12, F), np.zeros(3, F), np.zeros(16, np.int32),
            np.zeros(1, D)]
    ws = np.zeros(int(L.xfh_sim3_optimize_workspace_bytes(n1, 1)) // 8 + 2, D)     # 16-byte aligned by numpy's allocator for this size
    assert ws.ctypes.data % 16 == 0
    good = host_args(p, ws, outs)
    assert call_host(L, good) == 0
    before = [o.copy() for o in outs]

    def refused(**kw):
        assert call_host(L, dict(good, **kw)) == INVALID, kw
        assert all(np.array_equal(a, b, equal_nan=a.dtype.kind == "f") for a, b in zip(outs, before)), ("an output was written", kw)
    for k in ("n1", "M1", "nq", "n2"):                                   # sizes outside 1 .. XFH_GRID_MAX_N
        for v in (0, -1, capi.GRID_MAX_N + 1):
            refused(**{k: v})
    for v in (0, -1, 65536):
        refused(B=v)
    for k, v in good.items():                                            # NULL pointers (Tmw may be NULL; Tcw and Ow only without it)
        if (isinstance(v, np.ndarray) or k in ("cam1", "cam2")) and k not in ("Tmw", "flags2", "status"):
            refused(**{k: None})
    refused(flags2=None)
    refused(status=None)
    assert call_host(L, dict(good, Tmw=None, Tcw=None, Ow=None)) == 0
    for k, v in good.items():                                            # misaligned pointers: 4 bytes for floats and ints, 8 for doubles, 16 for the workspace
        if isinstance(v, np.ndarray) and v.dtype != np.uint8:
            pad = np.zeros(v.nbytes + 16, np.uint8)
            off = {"ws": 8}.get(k, v.dtype.itemsize // 2)
            refused(**{k: pad.ctypes.data + (-pad.ctypes.data) % 16 + off})
    for k in ("th2", "w1", "w2"):                                        # not finite or not > 0
        for v in (0.0, -1.0, float("nan"), float("inf")):
            refused(**{k: v})
    for k in ("side1_shared", "fix_scale", "all_points"):                # flags outside 0 .. 1
        for v in (-1, 2):
            refused(**{k: v})
    refused(S12_stride=12)                                               # a stride that is not a whole problem
    refused(S12_out_stride=0)
    assert L.xfh_sim3_optimize_workspace_bytes(0, 1) == 0 and L.xfh_sim3_optimize_workspace_bytes(capi.GRID_MAX_N + 1, 1) == 0
    assert L.xfh_sim3_optimize_workspace_bytes(16, 0) == 0 and L.xfh_sim3_optimize_workspace_bytes(16, 65536) == 0
    assert L.xfh_sim3_state_from(None, None) == INVALID and L.xfh_sim3_oplus(None, None, 0, None) == INVALID and L.xfh_sim3_map(None, None, None) == INVALID
    assert L.xfh_sim3_edge(None, None, None, None, None, None, None, 1.0, 1.0, 10.0, 0, 0, None, None, None, None) == INVALID
    assert L.xfh_kernel_name(capi.K["SIM3_OPTIMIZE"]) == b"k_sim3_optimize"


# ---- the sanitizer program ------------------------------------------------------------------------------------------------------------------------------
def test_optsim3_math_under_sanitizers(tmp_path):
    """tests/cpp/asan_optsim3_test.cpp, a stand-alone program built from optsim3_math.h alone with AddressSanitizer + UBSan: the kernel's loop as 256
    lanes with register slots and wave butterflies on one host thread, over good, NaN and hostile problems (every array filled with anything, NaN,
    Inf and any int included), byte for byte against the host form, every buffer allocated at its exact size.  Its first case is the stale-error
    rule with a FORCED rejected last trial: the chi2 sum of a full Levenberg step is replaced by a NaN, the trial is popped, classification 1 follows,
    and the chi2 every removed pair reports must be, bit for bit, its errors at the rejected estimate (computed there edge by edge), not at the
    restored one -- a statement about the state machine that no libm and no trajectory enters.  Nothing of the library is linked,
    nothing runs on a GPU, nothing is loaded into Python."""
    exe = str(tmp_path / "asan_optsim3_test")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "xfeatslam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "asan_optsim3_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "asan_optsim3_test ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


def test_kernel_instances_use_no_scratch():
    """k_sim3_optimize lives in kernels_match.hip, whose kernels may use no scratch.  Both instances sit at 256 VGPRs with their spills in AGPRs (216
    and 150 with clang 22 / ROCm 7.2, profiles/optimize_sim3.md): an unrolled Jacobian column loop puts them at 628 and 1452 bytes of scratch per lane
    (optsim3_math.h, os3_edge_jacobian), so the two are named here.  tools/kres.sh reads clang's kernel-resource-usage remarks (no GPU needed)."""
    import re
    import shutil
    if not shutil.which("c++filt") or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("needs hipcc and c++filt")
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kres.sh"), "kernels_match.hip"], capture_output=True, text=True, timeout=600).stdout
    rows = {m.group(1): tuple(int(x) for x in m.groups()[1:]) for m in
            (re.match(r"(?:void )?(k_sim3_optimize<\d+>)\S*\s+vgpr\s+(\d+)\s+agpr\s+(\d+)\s+scratch\s+(\d+)\s+occ\s+(\d+)", line) for line in out.splitlines()) if m}
    assert set(rows) == {"k_sim3_optimize<4>", "k_sim3_optimize<0>"}, out[-2000:]
    for name, (vgpr, agpr, scratch, occ) in rows.items():
        print(f"{name}: vgpr {vgpr} agpr {agpr} scratch {scratch} occ {occ}")
        assert scratch == 0 and vgpr <= 256 and occ >= 1, (name, rows[name])


# ---- the rig's condition ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(G.SCENES))
def test_rig_condition(L, name):
    """What makes a scene fair for the GPU comparison, measured among the float64 forms (the literal, the rule, the rule under three libm jitters, the
    host form): every chi2 a classification read is farther from th2 than 8 x its own largest deviation between the forms; n_corr - n_bad and
    n_bad > 0 are equal in all forms; every LDL^T pivot is farther than 1e-9 from 0.  The device is one more such form."""
    p = G.scene(name)
    forms = list(G.forms_of(name)) + [R.rule(p)]
    h, = G.run_host([p], L=L)
    heads = {(int(f["header"][0] - f["header"][3]), bool(f["header"][3] > 0)) for f in forms} | {(int(h["header"][0] - h["header"][3]), bool(h["header"][3] > 0))}
    assert len(heads) == 1, heads
    for key in ("cls1", "cls2"):
        v = np.stack([f[key] for f in forms])                            # (forms, n1, 2)
        assert len({np.isnan(x).tobytes() for x in v}) == 1 or name == "nan_z", (name, key)
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)             # rows without a classification are all NaN
            dev = np.nanmax(v, 0) - np.nanmin(v, 0)
            margin = np.nanmin(np.abs(v - G.TH2), 0)
        ok = np.isnan(dev) | (margin > 8 * dev)
        assert ok.all(), (name, key, np.nonzero(~ok)[0][:5], margin[~ok][:5], dev[~ok][:5])
    assert all(f["min_pivot"] > 1e-9 for f in forms[1:]), [f["min_pivot"] for f in forms[1:]]
