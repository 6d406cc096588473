"""Scenes, forms and the guarded device run for xfh_essential_graph*: a keyframe trajectory with accumulated drift, a loop closed between its ends
(CorrectedSim3 / NonCorrectedSim3 for the keyframes around the current one), the edges in the reference's creation order and map points with their
reference keyframes.  Shared by tests/test_essential_graph_ref.py, test_essential_graph_forms.py and test_gpu_essential_graph*.py.  No test lives here.

EG_TOL is TWICE the spread of the float64 forms among themselves (the literal form of tests/ref_essential_graph_literal.py, the rule of
tests/ref_essential_graph.py, that rule with its libm results moved by one ulp under three seeds, the host form xfh_essential_graph_host), measured by
tests/test_essential_graph_forms.py on SCENES and LIMIT with nothing from the device in it: Tcw_out and points_out in float32 steps at the magnitude of the
array, Sim3_out relative to max(1, |entry|max), chi2 in float32 steps at max(chi2, 1e-6), final_chi2 relative to max(final, 1e-6).  Measured spread:
see the figures beside EG_TOL."""
import collections
import functools

import numpy as np

import guarded
import ref_essential_graph as R
from xfeatslam_amd import capi, essential_graph as EG
from xfeatslam_amd.extractor import Context

F, D = np.float32, np.float64
GUARD = 256
JITTER_SEEDS = (11, 12, 13)
Tol = collections.namedtuple("Tol", "tcw sim3 points chi2 final")
# measured spread (tests/test_essential_graph_forms.py prints it), over SCENES and LIMIT: tcw 56 float32 steps (scale_free), sim3 4.46e-6 (far_start),
# points 55.25 steps (far_start), chi2 6.26e6 steps at the floor (thirty_seven_free), final 4.12e-5 (fold).  The spread is that wide because the Jacobians
# are numeric: a central difference over 2e-9 turns one ulp of an error (1e-16) into 1e-7 of a Jacobian entry, the last trial of most scenes is a REJECTED
# one whose step went through a pivot near 1e-4, and chi2 reports the error at that rejected estimate (the stale-error rule).
EG_TOL = Tol(tcw=112.0, sim3=8.92e-6, points=110.5, chi2=1.26e7, final=8.24e-5)


def _rot(rv):
    th = float(np.linalg.norm(rv))
    if th < 1e-12:
        return np.eye(3)
    k = np.asarray(rv, D) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], D)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def _sim_of(Rm, t, s):
    """(qx, qy, qz, qw, tx, ty, tz, s) of a rotation matrix by the library's own Quaterniond(Matrix3d)"""
    return R.RP.quat_from_matrix([float(v) for v in np.asarray(Rm, D).reshape(9)]) + [float(v) for v in t] + [float(s)]


def make(seed, n_free, fixed_at=0, covis=2, drift=0.01, scale=1.0, fix_scale=False, corrected=3, n_points=24, max_iterations=20, loop_edges=1, hubs=(), both_kinds=False,
         noise=0.0):
    """a circle of n_free + 1 keyframes (vertex fixed_at fixed) whose stored poses drift away from the truth; the last `corrected` keyframes carry a
    CorrectedSim3 (the truth side of the loop, scale `scale`) and a NonCorrectedSim3 (their stored pose); the current keyframe is the last one, the loop
    keyframe vertex 0.  hubs: for each count c a further FREE vertex joined by c normal edges to c further FIXED vertices."""
    rng = np.random.RandomState(seed)
    nC = n_free + 1
    true, stored = [], []
    dR, dt = np.eye(3), np.zeros(3)
    for k in range(nC):
        a = 2 * np.pi * k / (nC + 2)
        Rwc = _rot([0, a, 0])
        Ow = np.array([5 * np.cos(a), 0.1 * np.sin(3 * a), 5 * np.sin(a)])
        Rcw, tcw = Rwc.T, -Rwc.T @ Ow
        true.append((Rcw, tcw))
        dR = _rot(rng.randn(3) * drift) @ dR
        dt = dt + rng.randn(3) * drift * 3
        stored.append((dR @ Rcw, dR @ tcw + dt))
    poses = [np.hstack([Rm, t[:, None]]).reshape(12) for Rm, t in stored]
    fixed = [0] * nC
    fixed[fixed_at] = 1
    ci, ni, sim3 = [-1] * nC, [-1] * nC, []
    for v in range(nC - corrected, nC):
        Rm, t = true[v]
        Rn = _rot(rng.randn(3) * noise) @ Rm if noise else Rm
        ci[v] = len(sim3)
        sim3.append(_sim_of(Rn, scale * t, scale))
        ni[v] = len(sim3)
        Sm, ts = stored[v]
        sim3.append(_sim_of(np.asarray(Sm, F).astype(D), np.asarray(ts, F).astype(D), 1.0))
    ei, ej, kind = [], [], []
    cur = nC - 1
    for i in range(nC):
        if i == cur:
            for l in range(loop_edges):                                      # LoopConnections[pCurKF]: the loop keyframe and its neighbours
                ei.append(i); ej.append(l); kind.append(0)
                if both_kinds:
                    ei.append(l); ej.append(i); kind.append(1)
        if i > 0:
            ei.append(i); ej.append(i - 1); kind.append(1)                   # the spanning tree
        for c in range(2, covis + 1):
            if i - c >= 0:
                ei.append(i); ej.append(i - c); kind.append(1)               # covisibility
    for c in hubs:                                                           # a free hub and c fixed leaves of its own
        h = len(poses)
        Rm, t = stored[rng.randint(nC)]
        poses.append(np.hstack([Rm, t[:, None]]).reshape(12))
        fixed.append(0)
        if c:                                                                # the hub starts away from where its edges want it
            ci.append(len(sim3)); sim3.append(_sim_of(_rot(rng.randn(3) * 0.05) @ Rm, t + rng.randn(3) * 0.2, 1.0))
            ni.append(len(sim3)); sim3.append(_sim_of(np.asarray(Rm, F).astype(D), np.asarray(t, F).astype(D), 1.0))
        else:
            ci.append(-1); ni.append(-1)
        for _ in range(c):
            poses.append(np.hstack([_rot(rng.randn(3) * 0.3), rng.randn(3, 1) * 3]).reshape(12))
            fixed.append(1); ci.append(-1); ni.append(-1)
            ei.append(len(poses) - 1); ej.append(h); kind.append(1)
    nV = len(poses)
    # the stored poses of the edges' measurements come from the table; the estimate starts there too, so a graph without corrected entries is at its optimum
    perm = rng.permutation(nV + 3)[:nV]                                      # rows of the table in another order, three rows unused
    table = rng.randn(nV + 3, 12).astype(F)
    table[perm] = np.asarray(poses, F)
    pts = (rng.randn(n_points + 2, 3) * 2).astype(F)
    prow = rng.permutation(n_points + 2)[:n_points].astype(np.int32)
    pref = rng.randint(0, nV, n_points).astype(np.int32)
    return dict(pose_table=table, point_table=pts, kf_row=perm.astype(np.int32), kf_fixed=np.asarray(fixed, np.uint8), corrected_index=np.asarray(ci, np.int32),
                noncorrected_index=np.asarray(ni, np.int32), sim3=np.asarray(sim3, D).reshape(-1, 8), edge_i=np.asarray(ei, np.int32), edge_j=np.asarray(ej, np.int32),
                edge_kind=np.asarray(kind, np.int32), point_row=prow, point_ref=pref, fix_scale=int(fix_scale), max_iterations=max_iterations)


def _out_of_range():
    p = make(7, 6, n_points=16)
    p["edge_i"] = np.concatenate([p["edge_i"], [-1, 3, 99, 2, 2 ** 31 - 1]]).astype(np.int32)
    p["edge_j"] = np.concatenate([p["edge_j"], [2, 7, 1, 2, 0]]).astype(np.int32)
    p["edge_kind"] = np.concatenate([p["edge_kind"], [1, 1, 0, 1, 0]]).astype(np.int32)
    p["point_ref"][:4] = [-1, 7, 2 ** 31 - 1, -2 ** 31]
    p["point_row"][5] = 99
    return p


def _partial():
    """corrected and non-corrected entries for only some vertices: one with a corrected entry alone, one with a non-corrected entry alone"""
    p = make(8, 8, corrected=3, max_iterations=2)
    n = len(p["kf_row"])
    p["noncorrected_index"][n - 1] = -1
    p["corrected_index"][n - 3] = -1
    return p


def _nan_pose():
    p = make(9, 4, max_iterations=20)
    p["pose_table"][p["kf_row"][1], 5] = np.nan
    return p


def _no_edges():
    p = make(10, 3)
    p["edge_i"][:] = -1
    return p


def _all_fixed():
    p = make(11, 3)
    p["kf_fixed"][:] = 1
    return p


SCENES = {
    "one_free": lambda: make(1, 1, corrected=1, covis=1, max_iterations=2),
    "two_free": lambda: make(2, 2, corrected=1, max_iterations=3),
    "nine_free": lambda: make(3, 9),                                         # 63 unknowns: just under a 64-wide tile
    "ten_free": lambda: make(4, 10),                                         # 70: just over
    "nineteen_free": lambda: make(5, 19, covis=3, loop_edges=2),
    "thirty_seven_free": lambda: make(6, 37, covis=3, max_iterations=6),
    "chain_one_loop": lambda: make(12, 12, covis=1, corrected=1),            # a chain with one loop edge between its ends
    "both_kinds": lambda: make(13, 6, both_kinds=True),                      # a kind-0 and a kind-1 edge between the same pair
    "fold": lambda: make(14, 4, hubs=(0, 1, 255, 256, 257), max_iterations=2),   # vertices of 0, 1, 255, 256 and 257 edges
    "fixed_in_the_middle": lambda: make(15, 8, fixed_at=4),
    "scale_free": lambda: make(16, 8, scale=1.3),
    "scale_fixed": lambda: make(17, 8, scale=1.3, fix_scale=True, max_iterations=2),
    "partial": _partial,
    "out_of_range": _out_of_range,
    "far_start": lambda: make(18, 10, drift=0.12, noise=0.5, scale=1.3, max_iterations=5),
    "one_iteration": lambda: make(19, 5, max_iterations=1),
    "three_iterations": lambda: make(20, 5, max_iterations=3),
}
EARLY = {"no_edges": _no_edges, "all_fixed": _all_fixed}
LIMIT = {"free_128": lambda: make(30, 128, covis=2, max_iterations=1)}     # 896 unknowns, 14 block columns; one iteration: the rule in Python is slow here
FAILING = {"nan_pose": _nan_pose}
@functools.lru_cache(maxsize=None)
def scene(name):
    return {**SCENES, **EARLY, **LIMIT, **FAILING}[name]()


def random_small(k):
    rng = np.random.RandomState(5000 + k)
    return make(6000 + k, int(rng.randint(1, 5)), fixed_at=int(rng.randint(0, 2)), covis=int(rng.randint(1, 3)), drift=float(rng.choice([0.005, 0.03])),
                scale=float(rng.choice([1.0, 1.2])), fix_scale=bool(k % 2), corrected=1, n_points=6, max_iterations=int(rng.randint(1, 5)))


def problem_of(name):
    return scene(name) if isinstance(name, str) else random_small(name)


def n_free_of(p):
    return int(np.sum(np.asarray(p["kf_fixed"]) == 0))


def dims(p):
    """nV, nE, nP, nS"""
    return len(p["kf_row"]), len(p["edge_i"]), len(p["point_row"]), len(np.asarray(p["sim3"]).reshape(-1, 8))


def run_host(p, write_back=False, n_free=None, L=None):
    """xfh_essential_graph_host -> dict of outputs (+ the two tables as the call left them)"""
    L = L or capi.lib()
    nV, nE, nP, nS = dims(p)
    nf = n_free_of(p) if n_free is None else n_free
    a = EG.host_arrays(p)
    outs = EG.essential_graph_layout(nV, nP, nE).zeros()
    ws = np.zeros(int(L.xfh_essential_graph_workspace_bytes(nV, nE, nf)) + 16, np.uint8)
    wsp = (ws.ctypes.data + 15) & ~15
    rc = L.xfh_essential_graph_host(nV, nf, nE, nP, nS, a[0].ctypes.data, len(a[0]), a[1].ctypes.data, len(a[1]), *[x.ctypes.data for x in a[2:]], int(p["fix_scale"]),
                                    int(p["max_iterations"]), int(write_back), wsp, *[outs[k].ctypes.data for k in EG.NAMES])
    assert rc == 0, rc
    outs["final_chi2"] = float(outs["final_chi2"][0])
    outs["pose_table"], outs["point_table"] = a[0], a[1]
    return outs


@functools.lru_cache(maxsize=None)
def host_of(name):
    return run_host(problem_of(name))


@functools.lru_cache(maxsize=None)
def rule_of(name):
    return R.rule(problem_of(name))


@functools.lru_cache(maxsize=None)
def literal_of(name):
    import ref_essential_graph_literal as RL
    return RL.literal(problem_of(name))


@functools.lru_cache(maxsize=None)
def forms_of(name):
    """-> [literal, rule, rule with three libm jitters, host form]: the float64 forms, cached.  Under fix_scale the jittered rules are left out: the
    jitter is drawn afresh at every call, so the two perturbed estimates of the scale column, which are the same similarity, would differ and column 6
    of the Jacobians would be noise / 2e-9 -- no libm, being a function, does that"""
    p = problem_of(name)
    seeds = () if p["fix_scale"] else JITTER_SEEDS
    return [literal_of(name), rule_of(name)] + [R.rule(p, libm_jitter=s) for s in seeds] + [host_of(name)]


# ---- systems for the solver alone ------------------------------------------------------------------------------------------------------------------------
def spd_system(n, seed):
    """H + lambda I of a random connected pose graph's shape: 7 x 7 blocks J^T J on a chain with a few chords, so SPD and moderately conditioned"""
    rng = np.random.RandomState(seed)
    m = -(-n // 7)
    H = np.zeros((7 * m, 7 * m), D)
    pairs = [(i, i + 1) for i in range(m - 1)] + [(int(rng.randint(0, m)), int(rng.randint(0, m))) for _ in range(m // 2 + 1)]
    for i, j in pairs + [(0, 0)]:
        Ji, Jj = rng.randn(7, 7), rng.randn(7, 7)
        H[7 * i:7 * i + 7, 7 * i:7 * i + 7] += Ji.T @ Ji
        if i != j:
            H[7 * j:7 * j + 7, 7 * j:7 * j + 7] += Jj.T @ Jj
            H[7 * i:7 * i + 7, 7 * j:7 * j + 7] += Ji.T @ Jj
            H[7 * j:7 * j + 7, 7 * i:7 * i + 7] += Jj.T @ Ji
    H = H[:n, :n] + 0.5 * np.eye(n)
    return np.ascontiguousarray(H), rng.randn(n)


# ---- distances ----------------------------------------------------------------------------------------------------------------------------------------
def _apart(a, b):
    """|a - b| entry by entry; 0 where both hold the same value or both a NaN, inf where one alone holds a NaN"""
    a, b = np.asarray(a, D), np.asarray(b, D)
    na, nb = np.isnan(a), np.isnan(b)
    with np.errstate(all="ignore"):
        return np.where((a == b) | (na & nb), 0.0, np.where(na | nb, np.inf, np.abs(a - b)))


def _steps(a, b, mag):
    a, b = np.asarray(a, D), np.asarray(b, D)
    if a.size == 0:
        return 0.0
    with np.errstate(all="ignore"):
        return float(np.max(_apart(a, b) / np.spacing(F(mag))))


CHI_FLOOR = 1e-6


def distances(a, b):
    Ta, Tb = np.asarray(a["Tcw_out"], D).reshape(-1, 3, 4), np.asarray(b["Tcw_out"], D).reshape(-1, 3, 4)
    tmag = max(float(np.nanmax(np.abs(Ta[:, :, 3]), initial=1.0)), 1.0)
    tcw = max(_steps(Ta[:, :, :3], Tb[:, :, :3], 1.0), _steps(Ta[:, :, 3], Tb[:, :, 3], tmag))
    Sa, Sb = np.asarray(a["Sim3_out"], D), np.asarray(b["Sim3_out"], D)
    smag = max(float(np.nanmax(np.abs(Sa), initial=1.0)), 1.0)
    pmag = max(float(np.nanmax(np.abs(np.asarray(a["points_out"], D)), initial=1.0)), 1.0)
    ca, cb = np.asarray(a["chi2"], D), np.asarray(b["chi2"], D)
    with np.errstate(all="ignore"):
        mag = np.where(np.isfinite(ca) & np.isfinite(cb), np.maximum(np.maximum(ca, cb), CHI_FLOOR), CHI_FLOOR)
        chi = float(np.max(_apart(ca, cb) / np.spacing(mag.astype(F)).astype(D), initial=0.0))
    fa, fb = float(a["final_chi2"]), float(b["final_chi2"])
    fmag = max(fa, fb, CHI_FLOOR) if np.isfinite(fa) and np.isfinite(fb) else CHI_FLOOR
    return dict(tcw=tcw, sim3=float(np.max(_apart(Sa, Sb), initial=0.0)) / smag, points=_steps(a["points_out"], b["points_out"], pmag), chi2=chi,
                final=float(_apart(fa, fb)) / fmag)


def spread(forms):
    worst = dict.fromkeys(Tol._fields, 0.0)
    for i in range(len(forms)):
        for j in range(i + 1, len(forms)):
            for k, v in distances(forms[i], forms[j]).items():
                worst[k] = max(worst[k], v)
    return worst


def headers_differ(a, b):
    return not np.array_equal(np.asarray(a["header"]), np.asarray(b["header"]))


def outputs_agree(got, ref, tol=EG_TOL):
    d = distances(got, ref)
    return (["header"] if headers_differ(got, ref) else []) + [(k, d[k], getattr(tol, k)) for k in Tol._fields if not d[k] <= getattr(tol, k)]


def same_bits(a, b, names=EG.NAMES):
    """the names of the outputs in which two results differ by bits; a NaN stands for a NaN (Python and C++ do not give a NaN the same bits)"""
    bad = []
    for k in names:
        x, y = (np.asarray([r[k]], D) if k == "final_chi2" else np.ascontiguousarray(r[k]) for r in (a, b))
        if x.shape != y.shape or x.dtype != y.dtype:
            bad.append(k)
        elif x.dtype.kind == "f":
            u = {4: np.uint32, 8: np.uint64}[x.dtype.itemsize]
            if not np.all((x.view(u) == y.view(u)) | (np.isnan(x) & np.isnan(y))):
                bad.append(k)
        elif not np.array_equal(x, y):
            bad.append(k)
    return bad


# ---- the device ---------------------------------------------------------------------------------------------------------------------------------------
class EgRig:
    """run() -> dict of outputs and the raw output bytes; guards around the output block, the workspace and both tables are checked"""

    def __init__(self, L):
        self.L = L
        self.ctx = Context(nfeatures=1, max_height=32, max_width=32)

    def close(self):
        self.ctx.close()

    def run(self, p, write_back=False, fill=guarded.FILL, ws_fill=0x3C, n_free=None, expect_rc=0, max_iterations=None):
        L = self.L
        nV, nE, nP, nS = dims(p)
        nf = n_free_of(p) if n_free is None else n_free
        arrays = EG.host_arrays(p)
        tables = [guarded.Guarded(a.nbytes, GUARD, fill, inner=a, what=k) for a, k in zip(arrays[:2], ("the pose table", "the point table"))]
        dev = [capi.DeviceBuffer(max(a.nbytes, 8)).upload(a) for a in arrays[2:]]
        lay = EG.essential_graph_layout(nV, nP, nE, GUARD)
        out = guarded.outputs(lay, fill)
        ws_bytes = int(L.xfh_essential_graph_workspace_bytes(nV, nE, nf))
        assert ws_bytes > 0 and ws_bytes % 16 == 0
        ws = guarded.Guarded(ws_bytes, GUARD, fill, inner=ws_fill)
        try:
            rc = L.xfh_essential_graph_device(self.ctx.h, nV, nf, nE, nP, nS, tables[0].ptr, len(arrays[0]), tables[1].ptr, len(arrays[1]), *[d.ptr for d in dev],
                                              int(p["fix_scale"]), int(max_iterations or p["max_iterations"]), int(write_back), ws.ptr,
                                              *[out.ptr + lay[k] for k in EG.NAMES])
            assert rc == expect_rc, rc
            self.ctx.synchronize()
            raw = guarded.download(out, lay, fill)
            ws.download()
            a = lay.parse(raw)
            a["final_chi2"] = float(a["final_chi2"][0])
            a["pose_table"] = tables[0].download().view(F).reshape(-1, 12)
            a["point_table"] = tables[1].download().view(F).reshape(-1, 3)
        finally:
            for d in dev + [out, ws.buf, tables[0].buf, tables[1].buf]:
                d.free()
        return a, raw[lay.used()]                                           # the bytes of the arrays alone: the guards hold whatever fill the run chose
