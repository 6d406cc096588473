"""xfh_essential_graph_host and the pieces xfh_sim3_log, xfh_eg_edge, xfh_eg_solve (include/xfeat_hip.h, xfeatslam_amd/csrc/essgraph_math.h) against
the Python rule of tests/ref_essential_graph.py, on the CPU: the host form by bits on the rig's scenes and on 200 random small graphs; Sim3::log in all
four branches and on both sides of each eps, with exp(log(S)) = S; the edge against the rule and against central differences of a separately written
error (tests/ref_essential_graph_literal.py) with another delta; the LDL^T against numpy.linalg.solve and, by bits, against xfh_lba_solve; a hand-made
three-vertex graph whose first step is solved by hand; every class of refusal and every status; a NaN pose entry; bFixScale; the fairness condition of the
rig (literal, rule and host form give the same header on every scene the GPU comparison uses); the sanitizer program.

The NaN scene: the issue expected "all 200 factorisations fail".  Under the rule as g2o states it a NaN pose makes chi2 NaN, so rho is NaN: not < 0, hence
no second trial in an iteration, not 0, hence no stop.  Each of the 20 iterations has exactly ONE trial and its factorisation fails: 20 of 20, which is
what the header says and what this file asserts."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import essential_graph_rig as G
import ref_essential_graph as R
import ref_essential_graph_literal as RL
import ref_optsim3 as RO
from xfeatslam_amd import capi, essential_graph as EG

F, D = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
GPU_SCENES = list(G.SCENES) + list(G.EARLY) + list(G.LIMIT) + list(G.FAILING)


@pytest.fixture(scope="module")
def L():
    return capi.lib()


def header_of(r):
    return dict(zip(R.H_KEYS, np.asarray(r["header"]).tolist()))


@pytest.mark.parametrize("name", GPU_SCENES)
def test_host_form_equals_the_rule_on_the_rig(name):
    h, r = G.host_of(name), G.rule_of(name)
    print(name, header_of(h), h["final_chi2"])
    assert G.same_bits(h, r) == [], (name, header_of(h), header_of(r))


def test_host_form_equals_the_rule_on_200_random_graphs():
    seen = set()
    for k in range(200):
        p = G.random_small(k)
        h, r = G.run_host(p, write_back=bool(k % 3 == 0)), R.rule(p)
        assert G.same_bits(h, r) == [], (k, header_of(h), header_of(r))
        if k % 3 == 0:
            assert np.array_equal(h["pose_table"].view(np.uint32), r["written_pose_table"].view(np.uint32)), k
            assert np.array_equal(h["point_table"].view(np.uint32), r["written_point_table"].view(np.uint32)), k
        seen.add(tuple(h["header"][4:7]))
    assert len(seen) > 3                                                    # not one trajectory 200 times


def c_log(L, S):
    s, o = np.array(S, D), np.zeros(7, D)
    assert L.xfh_sim3_log(s.ctypes.data, o.ctypes.data) == 0
    return o


def test_sim3_log_in_every_branch(L):
    """(|sigma| < eps, d > 1 - eps) x 2, and just on both sides of each eps: theta^2 / 2 = 1e-5 <=> theta = 0.004472.., |sigma| = 1e-5.  exp(log(S)) = S is
    asserted wherever the reference's lines invert each other.  They do not for 0 < theta < 0.00447 with |sigma| >= 1e-5: log takes its d > 1 - eps branch there
    while the exponential (theta >= 1e-5) takes its general one, and that branch's B = ((0.5 sigma^2 - sigma + 1) s) / sigma^3 (sim3.h:193, :107) lacks the
    - 1 of the series it stands for, so it grows like 1 / sigma^3.  The rule follows the reference branch for branch, so the library does the same by bits."""
    th_eps, cases = float(np.sqrt(2e-5)), []
    for sigma in (0.0, 0.5e-5, np.nextafter(1e-5, 0), 1e-5, np.nextafter(1e-5, 1), 2e-5, -0.5e-5, -2e-5, 0.3, -0.7):
        for theta in (0.0, 1e-4, th_eps * (1 - 1e-9), th_eps * (1 + 1e-9), 0.01, 0.7, 2.5, 3.1):
            for ax in ([1, 0, 0], [0.3, -0.5, 0.8], [-0.6, 0.64, 0.48]):
                u = [theta * a / float(np.linalg.norm(ax)) for a in ax] + [0.3, -1.2, 0.5, sigma]
                cases.append(RO.exp7(u))
    branches = set()
    for S in cases:
        got, ref = c_log(L, S), np.array(R.sim3_log(S), D)
        assert got.tobytes() == ref.tobytes(), S
        Rm = R.RP.matrix_from_quat(S[:4])
        branches.add((abs(float(np.log(S[7]))) < R.EPS, 0.5 * (((Rm[0] + Rm[4]) + Rm[8]) - 1.0) > 1.0 - R.EPS))
        if abs(float(np.log(S[7]))) >= R.EPS and 0.5 * (((Rm[0] + Rm[4]) + Rm[8]) - 1.0) > 1.0 - R.EPS and abs(got[0]) + abs(got[1]) + abs(got[2]) > 0:
            continue                                                        # the reference's own lines do not invert each other here, see the docstring
        back = RO.exp7(list(got))                                           # exp(log(S)) = S (q up to sign)
        sgn = 1.0 if np.dot(back[:4], S[:4]) > 0 else -1.0
        assert np.allclose(sgn * np.array(back[:4]), S[:4], atol=2e-7) and np.allclose(back[4:], S[4:], rtol=1e-6, atol=2e-6), (S, back)
    assert len(branches) == 4
    # hostile: the call returns whatever the entries hold
    for S in ([np.nan] * 8, [0, 0, 0, 0, 1, 1, 1, 0.0], [0, 0, 0, 1, np.inf, 0, 0, -1.0]):
        c_log(L, S)
    assert L.xfh_sim3_log(None, np.zeros(7).ctypes.data) == INVALID


def c_edge(L, C_, Si, Sj, free_i=1, free_j=1, fix_scale=0):
    m, a, b = (np.array(x, D) for x in (C_, Si, Sj))
    e, c, Ji, Jj = np.zeros(7), np.zeros(1), np.zeros((7, 7)), np.zeros((7, 7))
    assert L.xfh_eg_edge(m.ctypes.data, a.ctypes.data, b.ctypes.data, free_i, free_j, fix_scale, e.ctypes.data, c.ctypes.data, Ji.ctypes.data, Jj.ctypes.data) == 0
    return e, float(c[0]), Ji, Jj


def test_edge_against_the_rule_and_an_independent_statement(L):
    rng = np.random.RandomState(3)
    for k in range(40):
        Si, Sj = RO.exp7(list(rng.randn(6) * 0.8) + [rng.randn() * 0.2]), RO.exp7(list(rng.randn(6) * 0.8) + [rng.randn() * 0.2])
        Cm = RO.mul(RO.exp7(list(rng.randn(7) * 0.05)), RO.mul(Sj, RO.inverse(Si)))
        for fi, fj, fs in ((1, 1, 0), (1, 0, 0), (0, 1, 1), (1, 1, 1)):
            e, c, Ji, Jj = c_edge(L, Cm, Si, Sj, fi, fj, fs)
            re, rc, rJi, rJj = R.linearize(Cm, Si, Sj, fi, fj, fs)
            assert e.tobytes() == np.array(re, D).tobytes() and c == rc and Ji.tobytes() == rJi.tobytes() and Jj.tobytes() == rJj.tobytes(), (k, fi, fj, fs)
            if fs:
                assert not Ji[:, 6].any() and not Jj[:, 6].any()             # column 6 is exactly 0
            if not fi:
                assert not Ji.any()
        # the independent statement: the literal form's error, central differences with delta 1e-6
        lit = lambda S: RL.Sim3(S[:4], S[4:7], S[7])
        e, c, Ji, Jj = c_edge(L, Cm, Si, Sj)
        assert np.allclose(e, RL.error(lit(Cm), lit(Si), lit(Sj)), rtol=1e-9, atol=1e-12)
        for which, J in ((0, Ji), (1, Jj)):
            for d in range(7):
                u = np.zeros(7)
                u[d] = 1e-6
                ep = RL.error(lit(Cm), RL.oplus(u, lit(Si), 0), lit(Sj)) if which == 0 else RL.error(lit(Cm), lit(Si), RL.oplus(u, lit(Sj), 0))
                em = RL.error(lit(Cm), RL.oplus(-u, lit(Si), 0), lit(Sj)) if which == 0 else RL.error(lit(Cm), lit(Si), RL.oplus(-u, lit(Sj), 0))
                assert np.allclose(J[:, d], (ep - em) / 2e-6, rtol=1e-4, atol=2e-6), (k, which, d)
    assert L.xfh_eg_edge(None, None, None, 1, 1, 0, None, None, None, None) == INVALID


def c_solve(L, fn, S, b, x0):
    S, x = np.ascontiguousarray(S, D).copy(), np.array(x0, D)
    ok = getattr(L, fn)(len(b), S.ctypes.data, np.ascontiguousarray(b, D).ctypes.data, x.ctypes.data)
    return ok, x, S


@pytest.mark.parametrize("n", [1, 7, 63, 64, 65, 129, 300, 768, 896])
def test_solve_against_numpy_and_the_lba_solver(L, n):
    S, b = G.spd_system(n, n)
    ok, x, Lf = c_solve(L, "xfh_eg_solve", S, b, np.full(n, 7.0))
    assert ok == 1 and np.allclose(x, np.linalg.solve(S, b), rtol=1e-8, atol=1e-10)
    if n <= 768:
        ok2, x2, Lf2 = c_solve(L, "xfh_lba_solve", S, b, np.full(n, 7.0))
        assert ok2 == 1 and x2.tobytes() == x.tobytes() and Lf2.tobytes() == Lf.tobytes()
    okr, xr, _ = R.RB.ldlt_solve(S, b, np.full(n, 7.0))[:3]
    assert okr and xr.tobytes() == x.tobytes()
    for k, v in ((0, 0.0), (n // 2, -1.0), (n - 1, np.nan)):
        Sb = S.copy()
        Sb[k, k] = v
        ok, x, _ = c_solve(L, "xfh_eg_solve", Sb, b, np.full(n, 7.0))
        assert ok == 0 and np.all(x == 7.0), (n, k)
    assert L.xfh_eg_solve(0, S.ctypes.data, b.ctypes.data, b.ctypes.data) == 0 and L.xfh_eg_solve(7 * EG.MAX_FREE + 1, S.ctypes.data, b.ctypes.data, b.ctypes.data) == 0


def three_vertices():
    rng = np.random.RandomState(21)
    S = [RO.exp7(list(rng.randn(6) * 0.5) + [0.0]) for _ in range(3)]
    table = np.stack([RO.state_to(s)[[0, 1, 2, 9, 3, 4, 5, 10, 6, 7, 8, 11]] for s in S]).astype(F)
    corr = [RO.mul(RO.exp7(list(rng.randn(7) * 0.02)), RO.state_from(RO.state_to(S[2])))]
    return dict(pose_table=table, point_table=np.zeros((1, 3), F), kf_row=np.arange(3, dtype=np.int32), kf_fixed=np.array([1, 0, 0], np.uint8),
                corrected_index=np.array([-1, -1, 0], np.int32), noncorrected_index=np.array([-1, -1, -1], np.int32), sim3=np.array(corr, D),
                edge_i=np.array([1, 2, 2], np.int32), edge_j=np.array([0, 1, 0], np.int32), edge_kind=np.array([1, 1, 0], np.int32), point_row=np.zeros(1, np.int32),
                point_ref=np.array([2], np.int32), fix_scale=0, max_iterations=1)


def test_three_vertex_graph_first_step_by_hand(L):
    """v0 fixed, v1 and v2 free, edges (1 -> 0), (2 -> 1) normal and (2 -> 0) a loop connection whose measurement comes from the table while v2 starts at a
    corrected entry: H and b assembled here from xfh_eg_edge's Jacobians with numpy, solved with numpy, applied with the literal form's oplus"""
    p = three_vertices()
    P = R.Plan(p)
    # vertex 2's Smw is its corrected entry (no non-corrected one), so edge 1's measurement uses it; edge 2 (kind 0) uses vScw: also the corrected entry
    H, b, chi = np.zeros((14, 14)), np.zeros(14), 0.0
    idx = {1: 0, 2: 1}
    for e in range(3):
        i, j = int(P.ei[e]), int(P.ej[e])
        er, c, Ji, Jj = c_edge(L, P.meas[e], P.vScw[i], P.vScw[j], int(i in idx), int(j in idx))
        chi += c
        for J, v in ((Ji, i), (Jj, j)):
            if v in idx:
                f = idx[v]
                H[7 * f:7 * f + 7, 7 * f:7 * f + 7] += J.T @ J
                b[7 * f:7 * f + 7] -= J.T @ er
        if i in idx and j in idx:
            H[7 * idx[i]:7 * idx[i] + 7, 7 * idx[j]:7 * idx[j] + 7] += Ji.T @ Jj
            H[7 * idx[j]:7 * idx[j] + 7, 7 * idx[i]:7 * idx[i] + 7] += Jj.T @ Ji
    x = np.linalg.solve(H + 1e-16 * np.eye(14), b)
    h = G.run_host(p)
    assert header_of(h) == dict(status=0, free=2, edges=3, loop_edges=1, iterations=1, trials=1, rejected=0, ldlt_failures=0, points=1)
    lit = lambda S: RL.Sim3(S[:4], S[4:7], S[7])
    for v, f in idx.items():
        want = RL.oplus(x[7 * f:7 * f + 7], lit(P.vScw[v]), 0).vec()
        assert np.allclose(h["Sim3_out"][v], want, rtol=1e-7, atol=1e-9), v
    assert np.array_equal(h["Sim3_out"][0], np.array(P.vScw[0]))            # the fixed vertex
    # every edge error at the start is 0 except where the corrected entry disagrees with the table: the edges of vertex 2 through Smw
    assert chi > 0 and h["final_chi2"] < chi


def call_host(L, p, **kw):
    nV, nE, nP, nS = G.dims(p)
    a = EG.host_arrays(p)
    outs = EG.essential_graph_layout(nV, nP, nE).zeros()
    nf = kw.get("nf", G.n_free_of(p))
    ws = np.zeros(max(int(L.xfh_essential_graph_workspace_bytes(nV, nE, max(0, min(nf, nV, EG.MAX_FREE)))), 64) + 16, np.uint8)
    wsp = (ws.ctypes.data + 15) & ~15
    ptrs = kw.get("ptrs") or [x.ctypes.data for x in a]
    op = kw.get("outs") or [outs[k].ctypes.data for k in EG.NAMES]
    rows = kw.get("rows", (len(a[0]), len(a[1])))
    rc = L.xfh_essential_graph_host(kw.get("nV", nV), nf, kw.get("nE", nE), kw.get("nP", nP), kw.get("nS", nS), ptrs[0], rows[0], ptrs[1], rows[1], *ptrs[2:],
                                    kw.get("fs", 0), kw.get("its", 3), kw.get("wb", 0), kw.get("wsp", wsp), *op)
    return rc, outs, a


def test_every_refusal_and_every_status(L):
    p = G.scene("two_free")
    rc, outs, a = call_host(L, p)
    assert rc == 0 and outs["header"][0] == R.OK
    nV = len(p["kf_row"])
    # n_free = XFH_EG_MAX_FREE + 1 is refused before anything is touched (the device form returns the same code before any launch: the check is shared)
    assert call_host(L, p, nf=EG.MAX_FREE + 1, nV=2000)[0] == INVALID and L.xfh_essential_graph_workspace_bytes(2000, 10, EG.MAX_FREE + 1) == 0
    assert L.xfh_essential_graph_workspace_bytes(2000, 10, EG.MAX_FREE) > (7 * EG.MAX_FREE) ** 2 * 8
    for kw in (dict(nf=-1), dict(nf=nV + 1), dict(nV=0), dict(nE=0), dict(nP=0), dict(nS=0), dict(nV=65536), dict(nE=(1 << 20) + 1), dict(rows=(0, 5)), dict(rows=(5, 0)),
               dict(its=0), dict(its=21), dict(wb=2), dict(wb=-1), dict(fs=2), dict(fs=-1), dict(wsp=None)):
        assert call_host(L, p, **kw)[0] == INVALID, kw
    _, outs, a = call_host(L, p)
    assert call_host(L, p, wsp=a[0].ctypes.data + 8)[0] == INVALID
    for i, (k, dt) in enumerate(EG.INPUTS):
        ptrs = [x.ctypes.data for x in a]
        ptrs[i] = None
        assert call_host(L, p, ptrs=ptrs)[0] == INVALID, k
        if dt != np.uint8:
            ptrs[i] = a[i].ctypes.data + 2
            assert call_host(L, p, ptrs=ptrs)[0] == INVALID, k
    for i, k in enumerate(EG.NAMES):
        op = [outs[n].ctypes.data for n in EG.NAMES]
        op[i] = None
        assert call_host(L, p, outs=op)[0] == INVALID, k
        op[i] = outs[k].ctypes.data + 2
        assert call_host(L, p, outs=op)[0] == INVALID, k
    assert L.xfh_essential_graph_device(None, *([1] * 5), None, 1, None, 1, *([None] * 10), 0, 1, 0, *([None] * 7)) == INVALID     # a NULL ctx
    assert L.xfh_essential_graph(None, *([1] * 5), None, 1, None, 1, *([None] * 10), 0, 1, 0, *([None] * 6)) == INVALID
    assert L.xfh_debug_eg_solve(None, 7, None, None, None, None) == INVALID
    # the statuses
    assert G.host_of("no_edges")["header"][0] == R.NO_EDGES and G.host_of("all_fixed")["header"][0] == R.NOTHING_FREE
    mm = G.run_host(p, n_free=1, write_back=True)
    assert mm["header"][0] == R.FREE_MISMATCH and mm["header"][1] == 2 and mm["final_chi2"] == 0.0 and not mm["chi2"].any()
    assert np.array_equal(mm["pose_table"].view(np.uint32), np.asarray(p["pose_table"], F).view(np.uint32))              # nothing is written back
    for name in ("no_edges", "all_fixed"):
        h, q = G.host_of(name), G.scene(name)
        assert h["header"][4:8].tolist() == [0, 0, 0, 0] and h["final_chi2"] == 0.0 and not h["chi2"].any()
        assert np.array_equal(h["Sim3_out"], np.array(R.Plan(q).vScw))       # the recovery of the inputs
        plain = np.asarray(q["corrected_index"]) < 0                          # without a corrected entry vScw is the table's row
        assert np.allclose(h["Tcw_out"][plain], np.asarray(q["pose_table"], F)[q["kf_row"]][plain], atol=1e-6)
    assert [capi.lib().xfh_kernel_name(capi.K[k]) for k in ("EG_PLAN", "EG_LINEARIZE", "EG_FILL", "EG_FACTOR", "EG_SUBST", "EG_EVALUATE", "EG_FINISH")] == \
        [b"k_eg_plan", b"k_eg_linearize", b"k_eg_fill", b"k_eg_factor", b"k_eg_subst", b"k_eg_evaluate", b"k_eg_finish"]
    assert capi.K["EG_PLAN"] == 67 and capi.lib().xfh_kernel_name(66) == b"k_lba_finish"                               # existing ids keep their values


def test_nan_pose_entry_fails_every_factorisation():
    h = G.host_of("nan_pose")
    print("nan_pose:", header_of(h), h["final_chi2"])
    assert header_of(h) == dict(status=0, free=4, edges=8, loop_edges=1, iterations=20, trials=20, rejected=20, ldlt_failures=20, points=24)
    assert np.isnan(h["final_chi2"]) and np.array_equal(h["header"], G.rule_of("nan_pose")["header"])
    p = G.scene("nan_pose")
    ok = ~np.isnan(np.asarray(G.rule_of("nan_pose")["Sim3_out"])).any(1)
    assert np.array_equal(h["Sim3_out"][ok], np.array(R.Plan(p).vScw)[ok])   # x stayed zero: every estimate is where it started


def test_fix_scale_keeps_every_scale_exactly():
    for name in ("scale_fixed", 1, 3, 5):
        p = G.problem_of(name)
        assert p["fix_scale"] == 1
        h = G.run_host(p)
        assert h["header"][4] >= 1 and np.array_equal(h["Sim3_out"][:, 7], np.array(R.Plan(p).vScw)[:, 7]), name
    h = G.host_of("scale_free")
    assert not np.array_equal(h["Sim3_out"][:, 7], np.array(R.Plan(G.scene("scale_free")).vScw)[:, 7])


@pytest.mark.parametrize("name", GPU_SCENES)
def test_fairness_of_the_rig(name):
    """a scene belongs to the GPU comparison only if the literal form, the rule and the host form give the same header"""
    forms = [G.literal_of(name), G.rule_of(name), G.host_of(name)]
    hs = [f["header"].tolist() for f in forms]
    r = G.rule_of(name)
    print(name, hs[1], "smallest |rho| %.3g, stop margin %.3g" % (r["margin_rho"], r["margin_stop"]))
    assert hs[0] == hs[1] == hs[2], (name, hs)


def test_the_rig_reaches_what_it_claims():
    deg = lambda p: np.bincount(np.concatenate([p["edge_i"], p["edge_j"]]), minlength=len(p["kf_row"]))
    d = deg(G.scene("fold"))
    free = np.asarray(G.scene("fold")["kf_fixed"]) == 0
    assert {0, 1, 255, 256, 257} <= set(d[free].tolist())
    assert [G.n_free_of(G.scene(n)) for n in ("one_free", "two_free", "nine_free", "ten_free", "nineteen_free", "thirty_seven_free", "free_128")] == [1, 2, 9, 10, 19, 37, 128]
    assert any(G.rule_of(n)["header"][6] > 0 for n in G.SCENES) and G.scene("fixed_in_the_middle")["kf_fixed"][4] == 1
    p = G.scene("both_kinds")
    pairs = {}
    for i, j, k in zip(p["edge_i"], p["edge_j"], p["edge_kind"]):
        pairs.setdefault((min(i, j), max(i, j)), set()).add(int(k))
    assert any(v == {0, 1} for v in pairs.values())


# ---- the sanitizer program ----------------------------------------------------------------------------------------------------------------------------------
def problem_file(path, p, expected, write_back=0):
    nV, nE, nP, nS = G.dims(p)
    a = EG.host_arrays(p)
    with open(path, "wb") as f:
        f.write(np.array([nV, G.n_free_of(p), nE, nP, nS, len(a[0]), len(a[1]), p["fix_scale"], p["max_iterations"], write_back], np.int32).tobytes())
        for x in a:
            f.write(x.tobytes())
        for k in EG.NAMES[:-1]:
            f.write(np.ascontiguousarray(expected[k]).tobytes())
        f.write(struct.pack("d", expected["final_chi2"]))
    return path


def test_essgraph_math_under_sanitizers(tmp_path):
    """tests/cpp/asan_essgraph_test.cpp, a stand-alone program with its own main built from essgraph_math.h alone with AddressSanitizer + UBSan: the pieces
    (log of exp, the 3 x 3 LU, the solver on hostile pivots) and the whole rule in buffers of exact size on the rig's scenes, byte for byte against the
    Python rule.  Nothing of the library is linked, nothing runs on a GPU, nothing is loaded into Python."""
    exe = str(tmp_path / "asan_essgraph_test")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "xfeatslam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "asan_essgraph_test.cpp"), "-o", exe])
    files = []
    for n in ("one_free", "ten_free", "both_kinds", "partial", "out_of_range", "scale_fixed", "no_edges", "all_fixed", "nan_pose", 2, 7):
        files.append(problem_file(str(tmp_path / ("p_%s.bin" % n)), G.problem_of(n), G.rule_of(n) if isinstance(n, str) else R.rule(G.problem_of(n)),
                                  write_back=1 if n in ("partial", 7) else 0))
    r = subprocess.run([exe] + files, capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "asan_essgraph_test ok (%d files)" % len(files) in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


def test_kernels_use_no_scratch():
    """kernels_essgraph.hip: no kernel may spill to scratch (clang's kernel-resource-usage remarks; no GPU needed)"""
    import re
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("needs hipcc")
    src = os.path.join(ROOT, "xfeatslam_amd", "csrc", "kernels_essgraph.hip")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", os.devnull], capture_output=True, text=True, timeout=600)
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(names) >= 19 and len(scratch) == len(names) == len(lds), r.stderr[-2000:]
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))
    assert max(lds) <= 65536, dict(zip(names, lds))
