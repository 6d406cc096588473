"""xfh_sim3_solve_device (k_sim3solve_prepare / _fit / _count / _decide) and xfh_sim3_merge_matches_device (k_sim3merge_*) against the rule form of
tests/ref_sim3solve.py on the scenes and with the guarded runs of tests/sim3solve_rig.py: the header as integers, every float by its bits (a NaN
equal to any NaN).  The device's fp64 and fp32 add, mul, div and sqrt are IEEE and the library is built without contraction, so no tolerance is
needed anywhere.  Shapes: n1 = 70 with N = 41 (a partial wave of correspondences), n1 = 300 with N = 261 (a second pass of the 256-lane
compaction, a fifth 64-lane pass of the count), iterations 1, 10, 20, 65, 92 and 300 (one lane block of the fit is 64 iterations, one workgroup
of the count is 4), B = 1 and B = 3 with shared and per-problem draws and T1w, M = 200 .. 700."""
import ctypes as C

import numpy as np
import pytest

import ref_sim3solve as R
import sim3solve_rig as G
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def rig(gpu_lib):
    r = G.Sim3SolveRig(gpu_lib)
    yield r
    r.close()


@pytest.fixture(scope="module")
def scenes():
    """the rig's scenes and the rule's answer for each: computed once, never changed"""
    s = G.rig()
    return s, {k: G.rule_of(v) for k, v in s.items()}


def test_every_scene_of_the_rig_equals_the_rule(rig, scenes):
    """every status and branch; what a call must leave alone still holds the bytes it held before"""
    s, want = scenes
    seen, its = set(), set()
    for n, sc in s.items():
        got, _ = rig.run(sc)
        G.assert_equals_rule(got, want[n], 0, prior_byte=0xA5)
        print(n, dict(zip(R.HEADER, got["header"][0].tolist())))
        assert R.STATUS_NAMES[got["header"][0, 1]] == G.EXPECT[n], n
        seen.add(int(got["header"][0, 1])); its.add(int(got["header"][0, 2]))
    assert seen == {0, 1, 2} and {1, 20, 65, 300} <= its


def test_three_candidates_against_separate_calls_and_two_runs(rig):
    fam = G.family()
    got, raw = rig.run(fam)
    for b, st in enumerate((R.CONVERGED, R.NO_MORE, R.TOO_FEW)):
        G.assert_equals_rule(got, G.rule_of(fam, b), b, prior_byte=0xA5)
        assert got["header"][b, 1] == st
    assert np.array_equal(rig.run(fam)[1], raw)                              # two runs give identical bytes
    lay3, lay1 = Context.sim3_solve_layout(3, 70, G.GUARD), Context.sim3_solve_layout(1, 70, G.GUARD)
    for b in range(3):
        one = dict(fam, matched=fam["matched"][b:b + 1], T2w=fam["T2w"][b:b + 1], draws=fam["draws"][b:b + 1])
        _, raw1 = rig.run(one)
        for k in Context.SIM3_SOLVE_OUT:
            per = lay1[k + "_bytes"]
            assert np.array_equal(raw1[lay1[k]:lay1[k] + per], raw[lay3[k] + b * per:lay3[k] + (b + 1) * per]), (b, k)


def test_shared_draws_and_poses_equal_per_problem_copies(rig):
    fam = G.family()
    d = fam["draws"][0]
    got, raw = rig.run(fam, draws=d)                                         # stride 0
    assert np.array_equal(rig.run(fam, draws=np.stack([d, d, d]))[1], raw)
    for b in range(3):
        G.assert_equals_rule(got, G.rule_of(dict(fam, draws=np.stack([d, d, d])), b), b, prior_byte=0xA5)
    assert np.array_equal(rig.run(fam, draws=d, T1w=np.stack([fam["T1w"]] * 3))[1], raw)
    T = np.stack([fam["T1w"]] * 3)                                           # own poses per problem
    T[1, 3] += F(0.25)
    got, _ = rig.run(fam, T1w=T)
    for b in range(3):
        G.assert_equals_rule(got, G.rule_of(dict(fam, T1w=T), b), b, prior_byte=0xA5)


def test_merge_count_gates_the_solver_on_the_device(rig, scenes):
    s, want = scenes
    sc = s["first"]
    got, _ = rig.run(sc, num_matches=19, min_matches=20)
    assert got["header"][0, :4].tolist() == [41, R.TOO_FEW, 0, -1] and np.all(got["floats"].view(np.uint8) == 0xA5) and np.all(got["inliers"] == 0xA5)
    got, _ = rig.run(sc, num_matches=20, min_matches=20)
    G.assert_equals_rule(got, want["first"], 0, prior_byte=0xA5)


def test_hostile_indices_draws_and_table(rig, scenes):
    s, _ = scenes
    sc = dict(s["after20"])
    sc.update(point1=sc["point1"].copy(), matched=sc["matched"].copy(), draws=sc["draws"].copy(), table=sc["table"].copy())
    sl = sc["slots"]
    sc["point1"][sl[2]], sc["matched"][0, sl[3]], sc["matched"][0, sl[4]], sc["matched"][0, sl[5]] = 200, 2 ** 31 - 1, -2 ** 31, 1 << 24
    sc["draws"][0, 1], sc["draws"][0, 2, 1] = (-5, 2 ** 31 - 1, -2 ** 31), 40000
    for v in (2 ** 31 - 1, -2 ** 31, 0):
        sc["table"][:] = v
        got, _ = rig.run(sc)
        w = G.rule_of(sc)
        G.assert_equals_rule(got, w, 0, prior_byte=0xA5)
        assert w["header"][0] == 37


def test_merge_equals_the_rule(rig):
    m = G.merge_scene()
    matched, kf, num, raw = rig.merge(m["match12"], m["point2"], m["M"])
    want = R.merge(m["match12"], m["point2"], m["M"])
    assert np.array_equal(matched, want[0]) and np.array_equal(kf, want[1]) and num == want[2]
    assert np.array_equal(rig.merge(m["match12"], m["point2"], m["M"])[3], raw)
    # every entry of eight covisibles races for ONE owner; then 300 slots over 700 points with the lists of four covisibles
    race = dict(match12=np.tile(np.arange(70, dtype=np.int32) % 80, (8, 1)), point2=np.full((8, 80), 7, np.int32))
    matched, kf, num, raw = rig.merge(race["match12"], race["point2"], 200)
    assert num == 1 and (matched[0], kf[0]) == (7, 0) and np.all(matched[1:] == -1) and np.all(kf[1:] == -1)
    assert np.array_equal(rig.merge(race["match12"], race["point2"], 200)[3], raw)
    rng = np.random.RandomState(9)
    m12, p2 = rng.randint(-40, 340, (4, 300)).astype(np.int32), rng.randint(-100, 800, (4, 330)).astype(np.int32)
    matched, kf, num, _ = rig.merge(m12, p2, 700)
    want = R.merge(m12, p2, 700)
    assert np.array_equal(matched, want[0]) and np.array_equal(kf, want[1]) and num == want[2] and num > 100


def test_host_pointer_forms(gpu_lib, scenes):
    s, want = scenes
    ctx = Context(nfeatures=1, max_height=32, max_width=32)
    try:
        for n in ("first", "after64", "no_more", "n_below_min", "big"):
            sc = s[n]
            prior = dict(floats=np.full(32, 7.5, F), inliers=np.full(len(sc["point1"]), 9, np.uint8), Tcw=np.full(12, -2.0, F), Ow=np.full(3, 4.0, F))
            got = ctx.sim3_solve(G.camera(sc["cam1"]), G.camera(sc["cam2"]), sc["points"], sc["point1"], sc["matched"][0], sc["T1w"], sc["T2w"][0], sc["table"],
                                 sc["draws"][0], G.RAND_MAX, min_inliers=sc["min_inliers"], fix_scale=sc["fix_scale"], prior=prior)
            G.assert_equals_rule(got, want[n], 0)
            for k, v in prior.items():
                if want[n][k] is None:
                    assert got[k][0].tobytes() == v.tobytes(), (n, k)
        m = G.merge_scene()
        got, w = ctx.sim3_merge_matches(m["match12"], m["point2"], m["M"]), R.merge(m["match12"], m["point2"], m["M"])
        assert np.array_equal(got[0], w[0]) and np.array_equal(got[1], w[1]) and got[2] == w[2]
    finally:
        ctx.close()


def test_every_refusal_returns_before_anything_is_queued(rig):
    L, ctx = rig.L, rig.ctx
    buf = capi.DeviceBuffer(1 << 16)
    cam = G.camera()
    p = buf.ptr

    def call(B=1, n1=8, M=8, e1=9.0, e2=9.0, mi=3, iters=2, dstride=0, tstride=0, rand_max=7, cam1=cam, cam2=cam, ptrs=None, h=None):
        q = dict(dict(pt=p, p1=p, m=p, t1=p, t2=p, nm=None, tb=p, dr=p, ws=p, hd=p, fl=p, il=p, tc=p, ow=p), **(ptrs or {}))
        return L.xfh_sim3_solve_device(ctx.h if h is None else h, B, n1, M, q["pt"], q["p1"], q["m"], q["t1"], tstride, q["t2"], None if cam1 is None else C.byref(cam1),
                                       None if cam2 is None else C.byref(cam2), e1, e2, 0, mi, 0, q["nm"], q["tb"], iters, q["dr"], dstride, rand_max, q["ws"], q["hd"],
                                       q["fl"], q["il"], q["tc"], q["ow"])
    try:
        bad = [call(B=0), call(B=65536), call(n1=0), call(n1=capi.GRID_MAX_N + 1), call(M=0), call(M=(1 << 24) + 1), call(mi=-1), call(e1=float("nan")),
               call(e2=float("inf")), call(rand_max=0), call(iters=0), call(iters=capi.SIM3_SOLVE_MAX_ITERS + 1), call(B=2, dstride=5), call(B=2, tstride=11),
               call(cam1=None), call(cam2=None)]
        bad += [call(ptrs={k: None}) for k in ("pt", "p1", "m", "t1", "t2", "tb", "dr", "ws", "hd", "fl", "il", "tc", "ow")]
        bad += [call(ptrs={k: p + 2}) for k in ("pt", "p1", "m", "t1", "t2", "nm", "tb", "dr", "hd", "fl", "tc", "ow")] + [call(ptrs=dict(ws=p + 8))]
        mg = lambda J=1, n1=8, n2=8, M=8, q=(p,) * 6: L.xfh_sim3_merge_matches_device(ctx.h, J, n1, n2, M, *q)
        bad += [mg(J=0), mg(J=65536), mg(n1=0), mg(n1=capi.GRID_MAX_N + 1), mg(n2=0), mg(M=0), mg(q=(p, p, p + 8, p, p, p)), mg(q=(p + 2, p, p, p, p, p))]
        bad += [mg(q=tuple(None if i == k else p for i in range(6))) for k in range(6)]
        assert all(rc == 1 for rc in bad), bad
        assert L.xfh_sim3_solve_workspace_bytes(capi.GRID_MAX_N + 1, 8, 1) == 0 and L.xfh_sim3_solve_workspace_bytes(capi.GRID_MAX_N, 1 << 20, 8) > 0
        ctx.synchronize()                                                   # nothing was queued: the stream is idle and no error is pending
    finally:
        buf.free()
