"""Seeded scenes for xfh_local_ba_device and its restatements (tests/ref_local_ba.py, tests/ref_local_ba_literal.py): keyframes on a baseline that see a
cloud of points, mono and stereo, with noise, gross outliers, starts far from the optimum, keyframes of 0, 1, 255, 256 and 257 edges and the other
cases the tests name; wide / wide_far (nK 266, 520 points, 3496 edges: chi2 folds of more than 256 terms, keyframes of 400, 511, 512, 513 and 520 edges),
idle_keyframes (nK 300 the largest dimension, 295 keyframes without an edge), far_start at 1 and 3 iterations, outliers at inv_sigma2 = float32(1 / 1.44)
and 4 (30 and 34 edges to erase against 31 at 1); FAILING, three scenes in which a NaN makes every factorisation fail and one in which an Inf leaves b_S
NaN behind a factorisation that holds.  SCENES is the table whose condition tests/test_local_ba_ref.py::test_rig_condition measures on the CPU and which the GPU tests
compare under LBA_TOL; run_host() runs a problem through xfh_local_ba_host, LbaRig on the device with the outputs, the workspace and both tables
between guard bytes."""
import collections
import ctypes as C
import functools

import numpy as np

import guarded
import ref_local_ba as R
import ref_local_ba_literal as RL
from xfeatslam_amd import capi, local_ba
from xfeatslam_amd.extractor import Context

D, F = np.float64, np.float32
CAM = (500.0, 500.0, 320.0, 240.0, 40.0)
GUARD = 256
JITTER_SEEDS = (11, 12, 13)

Tol = collections.namedtuple("Tol", "tcw points chi2 final")
# LBA_TOL: twice the largest spread of the float64 forms among themselves (the literal form, the rule, the rule with sqrt / sin / cos jittered by one
# double step under three seeds, the library's host form) that tests/test_local_ba_forms.py::test_spread_of_the_forms sees on SCENES and on the 200
# random small scenes: Tcw_out, points_out and chi2 in float32 steps (at the magnitude of the rotation or translation block, of the largest
# coordinate, and of max(chi2, threshold)), final_chi2 relative to max(final_chi2, 5.991); not below 1 float step and 1e-13 relative.  Seen: Tcw_out 0.25
# and points_out 0.002 of a step, chi2 5 steps (random scene 112), final_chi2 4.8e-8 (random scene 134): both between the rule and its libm-jittered runs, on scenes of 6 to 24 points with two to four
# observations each.
# On the scenes added for the wraps and the weights: wide chi2 0.25 of a step and final_chi2 3.1e-11, wide_far 0.5 and 8.2e-12, idle_keyframes 0 and 2.4e-13,
# far_start_1it / _3it 0 and 9.3e-14, outliers_w0694 / _w4 0 and 5.9e-15; Tcw_out and points_out 0 on all of them.  FAILING: the forms agree NaN for NaN.
# That test fails if it sees more than half of these.  Nothing from the device is in them.
LBA_TOL = Tol(tcw=1, points=1, chi2=10, final=1e-7)


def _rot(rv):
    th = np.linalg.norm(rv)
    if th < 1e-12:
        return np.eye(3)
    k = rv / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def make(seed, n_free, n_fixed, nP, per_point, kind="mixed", noise=0.4, pose_noise=0.01, point_noise=0.03, outliers=0.0, init_fixed=True, sees=None,
         max_iterations=10, extra=None, inv_sigma2=1.0):
    """kind: mono | stereo | mixed.  Keyframe order: [the initial keyframe, fixed inside the local set] + free + fixed.  per_point: how many keyframes
    see a point (drawn), or None with sees = a bool matrix (nK, nP)."""
    rng = np.random.RandomState(seed)
    n_init = 1 if init_fixed else 0
    nK = n_init + n_free + n_fixed
    fixed = np.array([1] * n_init + [0] * n_free + [1] * n_fixed, np.uint8)
    fx, fy, cx, cy, bf = CAM
    centers = np.stack([0.25 * np.arange(nK) + rng.uniform(-0.05, 0.05, nK), rng.uniform(-0.1, 0.1, nK), rng.uniform(-0.1, 0.1, nK)], 1)
    Rs = [_rot(rng.uniform(-0.05, 0.05, 3)) for _ in range(nK)]
    ts = [-Rs[k] @ centers[k] for k in range(nK)]
    X = np.stack([rng.uniform(-1.5, 1.5 + 0.25 * nK, nP), rng.uniform(-1.2, 1.2, nP), rng.uniform(4.0, 8.0, nP)], 1)
    if sees is None:
        sees = np.zeros((nK, nP), bool)
        for p in range(nP):
            sees[rng.choice(nK, min(per_point, nK), replace=False), p] = True
        sees[nK - 1 if n_fixed else 0, ~sees[fixed != 0].any(0)] = True    # every point is tied to a fixed keyframe
    edge_begin, edge_kf, edge_obs = [0], [], []
    for p in range(nP):
        for k in np.nonzero(sees[:, p])[0]:
            pc = Rs[k] @ X[p] + ts[k]
            u, v = fx * pc[0] / pc[2] + cx, fy * pc[1] / pc[2] + cy
            st = kind == "stereo" or (kind == "mixed" and rng.rand() < 0.5)
            n3 = rng.normal(0, noise, 3)
            if outliers and rng.rand() < outliers:
                n3[:2] += rng.choice([-1, 1], 2) * rng.uniform(15, 40, 2)
            edge_kf.append(k)
            edge_obs.append((u + n3[0], v + n3[1], (u - bf / pc[2] + n3[2]) if st else -1.0))
        edge_begin.append(len(edge_kf))
    pose_rows, point_rows = nK + 3, nP + 5
    kf_row, point_row = rng.permutation(pose_rows)[:nK].astype(np.int32), rng.permutation(point_rows)[:nP].astype(np.int32)
    pose_table = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F), (pose_rows, 1))
    point_table = rng.uniform(-1, 1, (point_rows, 3)).astype(F)
    for k in range(nK):
        Rk, tk = Rs[k], ts[k]
        if not fixed[k]:
            Rk = _rot(rng.normal(0, pose_noise, 3)) @ Rk
            tk = tk + rng.normal(0, pose_noise * 3, 3)
        pose_table[kf_row[k]] = np.concatenate([Rk, tk[:, None]], 1).reshape(12).astype(F)
    point_table[point_row] = (X + rng.normal(0, point_noise, X.shape)).astype(F)
    p = dict(pose_table=pose_table, point_table=point_table, kf_row=kf_row, kf_fixed=fixed, point_row=point_row, edge_begin=np.array(edge_begin, np.int32),
             edge_kf=np.array(edge_kf, np.int32), edge_obs=np.array(edge_obs, F).reshape(-1, 3), cam=CAM, inv_sigma2=float(F(inv_sigma2)), max_iterations=max_iterations)
    if extra:
        extra(p, rng)
    return p


def _kf_edges_sees():
    """nK = 8: the initial keyframe and two fixed cameras see all 257 points; five free keyframes have 0, 1, 255, 256 and 257 edges"""
    s = np.zeros((8, 257), bool)
    s[0] = s[6] = s[7] = True
    for k, n in zip(range(1, 6), (0, 1, 255, 256, 257)):
        s[k, :n] = True
    return s


def _special(p, rng):
    """a point seen once (mono only), a point with no edge, an edge whose keyframe index is out of range (both ways), a point behind a camera"""
    b, kf, obs = p["edge_begin"].tolist(), p["edge_kf"].tolist(), p["edge_obs"].tolist()
    nK = len(p["kf_row"])
    kf[b[1] - 1] = nK                                                       # point 0 loses its last edge upwards,
    kf[b[2] - 1] = -1                                                       # point 1 downwards
    for e in range(b[2], b[3]):                                             # point 2 has no valid edge at all
        kf[e] = nK + 5
    lo, hi = b[3], b[4]                                                     # point 3 is seen once, mono, by the last fixed camera
    del kf[lo + 1:hi], obs[lo + 1:hi]
    kf[lo], obs[lo][2] = nK - 1, -1.0
    b[4:] = [v - (hi - lo - 1) for v in b[4:]]
    b.insert(5, b[4])                                                       # a new point 4 without an entry in the CSR
    unused = sorted(set(range(len(p["point_table"]))) - set(p["point_row"].tolist()))[0]
    p["point_row"] = np.insert(p["point_row"], 4, unused).astype(np.int32)
    row = p["kf_row"][kf[b[5]]]                                             # point 5 starts behind the first camera that sees it
    T = p["pose_table"][row].astype(D).reshape(3, 4)
    p["point_table"][p["point_row"][5]] = (T[:, :3].T @ (np.array([0.3, 0.2, -2.0]) - T[:, 3])).astype(F)
    p["edge_begin"], p["edge_kf"], p["edge_obs"] = np.array(b, np.int32), np.array(kf, np.int32), np.array(obs, F).reshape(-1, 3)


def _no_fixed_edge(p, rng):
    p["edge_kf"][p["kf_fixed"][np.clip(p["edge_kf"], 0, len(p["kf_row"]) - 1)] != 0] = -1


def _wide_sees():
    """nK = 266, 520 points: the initial keyframe and the first fixed camera see every point, the free keyframes 1 .. 4 the first 400, 511, 512 and 513 (a
    second and a third pass of the 256 lanes, by one lane and by whole waves), each of the other 260 fixed cameras two points"""
    s = np.zeros((266, 520), bool)
    s[0] = s[5] = True
    for k, n in zip(range(1, 5), (400, 511, 512, 513)):
        s[k, :n] = True
    for k in range(6, 266):
        s[k, (2 * k) % 520] = s[k, (2 * k + 1) % 520] = True
    return s


def _idle_sees():
    """nK = 300, six points, 27 edges: nK is the largest of (nK, nP, nE); 295 keyframes have no edge"""
    s = np.zeros((300, 6), bool)
    s[0] = s[1] = s[299] = True
    s[2, :4] = True
    s[150, 1:] = True
    return s


def _nth_edge_of(p, k, n):
    return int(np.nonzero(np.asarray(p["edge_kf"]) == k)[0][n])


def _bad_obs(k, column, value):
    """the sixth edge of keyframe k gets `value` in one entry of its observation"""
    def extra(p, rng):
        p["edge_obs"][_nth_edge_of(p, k, 5), column] = value
    return extra


def _nan_point(p, rng):
    p["point_table"][p["point_row"][7], 2] = np.nan


SCENES = {
    "one_free": lambda: make(1, 1, 1, 14, 2, "stereo", init_fixed=False),
    "two_free_mono": lambda: make(2, 2, 1, 40, 3, "mono"),
    "eleven_mixed": lambda: make(3, 11, 2, 120, 4, "mixed"),
    "twentytwo": lambda: make(4, 22, 3, 160, 5, "mixed"),
    "kf_edges": lambda: make(5, 5, 2, 257, None, "mixed", sees=_kf_edges_sees()),
    "stereo_only": lambda: make(16, 4, 2, 60, 4, "stereo"),
    "far_start": lambda: make(7, 3, 2, 50, 4, "mixed", pose_noise=0.08, point_noise=0.5),
    "outliers": lambda: make(8, 4, 2, 80, 4, "mixed", outliers=0.12),
    "special": lambda: make(9, 3, 2, 30, 3, "mixed", extra=_special),
    "seen_by_all": lambda: make(10, 3, 2, 25, 6, "mixed"),
    # the strides and grids no scene above wraps: chi2 folds over nK = 266 and 300 terms, keyframes of 400 .. 520 edges, nK the largest dimension
    "wide": lambda: make(40, 4, 261, 520, None, "mixed", sees=_wide_sees()),
    "wide_far": lambda: make(40, 4, 261, 520, None, "mixed", sees=_wide_sees(), pose_noise=0.08, point_noise=0.5, outliers=0.05),
    "idle_keyframes": lambda: make(42, 2, 297, 6, None, "mixed", sees=_idle_sees()),
    "far_start_1it": lambda: make(7, 3, 2, 50, 4, "mixed", pose_noise=0.08, point_noise=0.5, max_iterations=1),
    "far_start_3it": lambda: make(7, 3, 2, 50, 4, "mixed", pose_noise=0.08, point_noise=0.5, max_iterations=3),
    # an information weight other than 1 (the workload's own is 1: octave 0)
    "outliers_w0694": lambda: make(8, 4, 2, 80, 4, "mixed", outliers=0.12, inv_sigma2=1 / 1.44),
    "outliers_w4": lambda: make(8, 4, 2, 80, 4, "mixed", outliers=0.12, inv_sigma2=4.0),
}
EARLY = {
    "aborted": lambda: make(20, 2, 1, 20, 3, "mixed", extra=_no_fixed_edge),
    "nothing_free": lambda: make(21, 0, 2, 20, 2, "mixed"),
}
# every factorisation fails (a NaN reaches S), or none does although b_S is NaN (the Inf: rho1 = delta / sqrt(Inf) = 0 keeps H finite and makes b = 0 * Inf):
# keyframes 0 fixed (initial), 1 .. 3 free, 4 and 5 fixed
FAILING = {
    "nan_obs_free": lambda: make(41, 3, 2, 40, 4, "mixed", extra=_bad_obs(1, 0, np.nan)),
    "nan_obs_fixed": lambda: make(41, 3, 2, 40, 4, "mixed", extra=_bad_obs(5, 0, np.nan)),
    "nan_point": lambda: make(41, 3, 2, 40, 4, "mixed", extra=_nan_point),
    "inf_obs_free": lambda: make(41, 3, 2, 40, 4, "mixed", extra=_bad_obs(1, 1, np.inf)),
}
LIMIT = {"limit_128": lambda: make(30, 128, 2, 300, 4, "mixed", max_iterations=2)}     # S is 768 x 768: the refusal limit itself


@functools.lru_cache(maxsize=None)
def scene(name):
    return {**SCENES, **EARLY, **LIMIT, **FAILING}[name]()


def random_small(k):
    rng = np.random.RandomState(1000 + k)
    n_free, n_fixed = int(rng.randint(1, 5)), int(rng.randint(1, 3))
    return make(2000 + k, n_free, n_fixed, int(rng.randint(6, 25)), int(rng.randint(2, 5)), ("mono", "stereo", "mixed")[k % 3], pose_noise=float(rng.choice([0.005, 0.03])),
                outliers=float(rng.choice([0.0, 0.1])), init_fixed=bool(k % 2))


def problem_of(name):
    return scene(name) if isinstance(name, str) else random_small(name)


def n_free_of(p):
    return int(np.sum(np.asarray(p["kf_fixed"]) == 0))


def cam_struct(cam=CAM):
    c = capi.Camera()
    c.fx, c.fy, c.cx, c.cy, c.bf = cam
    c.width, c.height = 640, 480
    return c


INPUTS = (("pose_table", F), ("point_table", F), ("kf_row", np.int32), ("kf_fixed", np.uint8), ("point_row", np.int32), ("edge_begin", np.int32),
          ("edge_kf", np.int32), ("edge_obs", F))


def dims(p):
    return len(p["kf_row"]), len(p["point_row"]), len(p["edge_kf"])


def run_host(p, write_back=False, n_free=None, L=None):
    """xfh_local_ba_host -> dict of outputs (+ the two tables as the call left them)"""
    L = L or capi.lib()
    nK, nP, nE = dims(p)
    nf = n_free_of(p) if n_free is None else n_free
    arrays = [np.ascontiguousarray(np.asarray(p[k], dt)).copy() for k, dt in INPUTS]
    outs = local_ba.local_ba_layout(nK, nP, nE).zeros()
    ws = np.zeros(int(L.xfh_local_ba_workspace_bytes(nK, nP, nE, nf)) + 16, np.uint8)
    wsp = (ws.ctypes.data + 15) & ~15
    cam = cam_struct(p["cam"])
    rc = L.xfh_local_ba_host(nK, nf, nP, nE, arrays[0].ctypes.data, len(arrays[0]), arrays[1].ctypes.data, len(arrays[1]), *[a.ctypes.data for a in arrays[2:]],
                             C.byref(cam), p["inv_sigma2"], p.get("max_iterations", 10), int(write_back), wsp, *[outs[k].ctypes.data for k in local_ba.NAMES])
    assert rc == 0, rc
    outs["final_chi2"] = float(outs["final_chi2"][0])
    outs["pose_table"], outs["point_table"] = arrays[0], arrays[1]
    return outs


@functools.lru_cache(maxsize=None)
def host_of(name):
    return run_host(problem_of(name))


@functools.lru_cache(maxsize=None)
def rule_of(name):
    return R.rule(problem_of(name))


@functools.lru_cache(maxsize=None)
def forms_of(name):
    """-> [literal, rule, rule with three libm jitters, host form]: the float64 forms, cached"""
    p = problem_of(name)
    return [RL.literal(p), rule_of(name)] + [R.rule(p, libm_jitter=s) for s in JITTER_SEEDS] + [host_of(name)]


# ---- distances ----------------------------------------------------------------------------------------------------------------------------------------
def _apart(a, b):
    """|a - b| entry by entry; 0 where both hold the same value (the same infinity included) or both a NaN, inf where one alone holds a NaN"""
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


def distances(a, b):
    Ta, Tb = np.asarray(a["Tcw_out"], D).reshape(-1, 3, 4), np.asarray(b["Tcw_out"], D).reshape(-1, 3, 4)
    tmag = np.maximum(np.nanmax(np.abs(Ta[:, :, 3]), initial=1.0), 1.0)
    tcw = max(_steps(Ta[:, :, :3], Tb[:, :, :3], 1.0), _steps(Ta[:, :, 3], Tb[:, :, 3], tmag))
    pmag = max(float(np.nanmax(np.abs(a["points_out"]), initial=1.0)), 1.0)
    ca, cb = np.asarray(a["chi2"], D), np.asarray(b["chi2"], D)
    with np.errstate(all="ignore"):
        mag = np.where(np.isfinite(ca) & np.isfinite(cb), np.maximum(np.maximum(ca, cb), 5.991), 5.991)
        chi = float(np.max(_apart(ca, cb) / np.spacing(mag.astype(F)).astype(D), initial=0.0))
    fa, fb = float(a["final_chi2"]), float(b["final_chi2"])
    fmag = max(fa, fb, 5.991) if np.isfinite(fa) and np.isfinite(fb) else 5.991
    return dict(tcw=tcw, points=_steps(a["points_out"], b["points_out"], pmag), chi2=chi, final=float(_apart(fa, fb)) / fmag)


def spread(forms):
    worst = dict.fromkeys(Tol._fields, 0.0)
    for i in range(len(forms)):
        for j in range(i + 1, len(forms)):
            for k, v in distances(forms[i], forms[j]).items():
                worst[k] = max(worst[k], v)
    return worst


def decisions_differ(a, b):
    """the names of the decisions in which two results differ: every erase flag and the whole header"""
    return [k for k in ("erase", "header") if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]))]


def outputs_agree(got, ref, tol=LBA_TOL):
    d = distances(got, ref)
    return decisions_differ(got, ref) + [(k, d[k], getattr(tol, k)) for k in Tol._fields if not d[k] <= getattr(tol, k)]


# ---- the device ---------------------------------------------------------------------------------------------------------------------------------------
class LbaRig:
    """run() -> dict of outputs and the raw output bytes; guards around the output block, the workspace and both tables are checked"""

    def __init__(self, L):
        self.L = L
        self.ctx = Context(nfeatures=1, max_height=32, max_width=32)

    def close(self):
        self.ctx.close()

    def run(self, p, write_back=False, fill=guarded.FILL, ws_fill=0x3C, n_free=None, expect_rc=0):
        L = self.L
        nK, nP, nE = dims(p)
        nf = n_free_of(p) if n_free is None else n_free
        arrays = [np.ascontiguousarray(np.asarray(p[k], dt)) for k, dt in INPUTS]
        tables = [guarded.Guarded(a.nbytes, GUARD, fill, inner=a, what=k) for a, k in zip(arrays[:2], ("the pose table", "the point table"))]
        dev = [capi.DeviceBuffer(max(a.nbytes, 4)).upload(a) for a in arrays[2:]]
        lay = local_ba.local_ba_layout(nK, nP, nE, GUARD)
        out = guarded.outputs(lay, fill)
        ws_bytes = int(L.xfh_local_ba_workspace_bytes(nK, nP, nE, nf))
        assert ws_bytes > 0 and ws_bytes % 16 == 0
        ws = guarded.Guarded(ws_bytes, GUARD, fill, inner=ws_fill)
        cam = cam_struct(p["cam"])
        try:
            rc = L.xfh_local_ba_device(self.ctx.h, nK, nf, nP, nE, tables[0].ptr, len(arrays[0]), tables[1].ptr, len(arrays[1]), *[d.ptr for d in dev], C.byref(cam),
                                       p["inv_sigma2"], p.get("max_iterations", 10), int(write_back), ws.ptr, *[out.ptr + lay[k] for k in local_ba.NAMES])
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
        return a, raw[lay.used()]
