"""Seeded scenes for the Sim3 solver (xfh_sim3_solve*) and the merge in front of it (xfh_sim3_merge_matches*), and the guarded device runs the GPU
tests share.  A scene is one current keyframe against B candidate keyframes over ONE point table: the candidates' points are the current
keyframe's under a similarity (R, t, s) between the two CAMERA frames, X1 = s R X2 + t, with noise and outliers.  Two shapes, each across a boundary
of the kernels: n1 = 70 with N = 41 correspondences (a partial wave) and n1 = 300 with N = 261 (a second block of the 256-lane compaction)."""
import numpy as np

import ref_sim3solve as R

F = np.float32
CAM = (F(458.654), F(457.296), F(367.215), F(248.375))
CAM2 = (F(435.2), F(435.2), F(376.0), F(240.0))
RAND_MAX = 32767
PROB, MAX_ITS = 0.99, 300


def camera(cam=None):
    from xfeatslam_amd import capi
    c = CAM if cam is None else cam
    return capi.Camera(fx=float(c[0]), fy=float(c[1]), cx=float(c[2]), cy=float(c[3]), width=752, height=480)


def rot(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.radians(deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def pose(rng):
    Rm = rot(rng.randn(3), rng.uniform(5, 40))
    return np.concatenate([Rm, rng.uniform(-2, 2, (3, 1))], 1)


def scene(seed, n1=70, M=200, N=41, B=1, inlier_frac=0.7, noise=2e-3, scale=1.0, deg=8.0, min_inliers=15, fix_scale=False, max_iters=None, same_frame=False, T2w=None, tmax=0.3):
    """-> dict(points [M][3], point1 [n1], matched [B][n1], T1w [12], T2w [B][12], draws [B][max_iters][3], table [n1 + 1], S [B] = (R, t, s))"""
    rng = np.random.RandomState(seed)
    assert M >= n1 + B * n1
    T1w = pose(rng)
    slots = np.sort(rng.choice(n1, N, replace=False))
    point1 = np.full(n1, -1, np.int32)
    rows1 = rng.permutation(n1)                                                             # the current keyframe's points: rows 0 .. n1 - 1, shuffled
    has1 = np.zeros(n1, bool)
    has1[slots] = True
    extra = rng.choice(np.nonzero(~has1)[0], min(8, n1 - N), replace=False)                  # map points without a match
    has1[extra] = True
    point1[has1] = rows1[has1]
    points = rng.uniform(-50, 50, (M, 3))
    X1 = np.stack([rng.uniform(-2.5, 2.5, n1), rng.uniform(-1.6, 1.6, n1), rng.uniform(3, 9, n1)], 1)      # in camera 1
    inv = lambda T, X: (X - T[:, 3]) @ T[:, :3]
    points[rows1] = inv(T1w, X1)
    matched, T2ws, Ss = np.full((B, n1), -1, np.int32), [], []
    for b in range(B):
        T2w_b = T1w.copy() if same_frame else (pose(rng) if T2w is None else np.asarray(T2w, np.float64).reshape(3, 4))
        Rm, t = (np.eye(3), np.zeros(3)) if same_frame else (rot(rng.randn(3), deg), rng.uniform(-tmax, tmax, 3))
        rows2 = n1 + b * n1 + rng.permutation(n1)
        X2 = ((X1 - t) @ Rm) / scale                                                        # X1 = s R X2 + t
        X2 = X2 + noise * rng.randn(n1, 3)
        out = np.ones(n1, bool)
        out[slots[rng.permutation(N)[:int(round(inlier_frac * N))]]] = False
        X2[out] = np.stack([rng.uniform(-2.5, 2.5, out.sum()), rng.uniform(-1.6, 1.6, out.sum()), rng.uniform(3, 9, out.sum())], 1)
        points[rows2] = inv(T2w_b, X2)
        matched[b, slots] = rows2[slots]
        other = rng.choice(np.nonzero(point1 < 0)[0], min(5, int((point1 < 0).sum())), replace=False)      # a match where the current keyframe has no point
        matched[b, other] = rows2[other]
        T2ws.append(T2w_b.ravel()); Ss.append((Rm, t, scale))
    table = R.iterations_table(PROB, min_inliers, MAX_ITS, n1)
    max_iters = int(table[N]) if max_iters is None else max_iters
    draws = rng.randint(0, RAND_MAX + 1, (B, max_iters, 3)).astype(np.int32)
    return dict(points=points.astype(F), point1=point1, matched=matched, T1w=T1w.ravel().astype(F), T2w=np.array(T2ws, F), draws=draws, table=table, S=Ss,
                min_inliers=min_inliers, fix_scale=fix_scale, slots=slots, cam1=CAM, cam2=CAM2, max_err=9.0)


def rule_of(s, b=0, **kw):
    a = dict(min_inliers=s["min_inliers"], fix_scale=s["fix_scale"], max_err1=s["max_err"], max_err2=s["max_err"])
    a.update(kw)
    T1w = s["T1w"].reshape(-1, 12)
    return R.rule(s["points"], s["point1"], s["matched"][b], T1w[b if len(T1w) > 1 else 0], s["T2w"][b], s["cam1"], s["cam2"], s["table"], s["draws"][b], RAND_MAX, **a)


def bad_until(s, K, bad_compact=0, seed=0):
    """draws of iterations 0 .. K - 1 all hit compact correspondence `bad_compact` (draw 0 at position 0 while it is 0: an outlier put there), iteration K
    is redrawn until the rule converges there"""
    rng = np.random.RandomState(seed)
    d = s["draws"][0]
    d[:K, 0] = 0
    for _ in range(200):
        d[K] = rng.randint(0, RAND_MAX + 1, 3)
        r = rule_of(dict(s, draws=d[None, K:K + 1].copy(), table=np.ones_like(s["table"])))
        if r["header"][1] == R.CONVERGED:
            return
    raise AssertionError("no converging set found")


def make_outlier(s, compact_k, b=0):
    """moves the candidate's point of compact correspondence k far away"""
    i1 = s["slots"][compact_k]
    s["points"][s["matched"][b, i1]] += F(25.0)


def rig():
    s = {}
    s["first"] = scene(1, inlier_frac=1.0)                                                   # converges at iteration 0
    a = scene(2, inlier_frac=0.8)                                                            # N = 41: 92 iterations from the formula; the first 25 hit an outlier
    make_outlier(a, 0); bad_until(a, 25)
    s["after20"] = a
    a = scene(3, inlier_frac=0.8)
    make_outlier(a, 0); bad_until(a, 70)
    s["after64"] = a
    a = scene(4, inlier_frac=0.7, min_inliers=30)                                            # never above 30: NO_MORE; the best set drawn again later
    r = rule_of(a)
    k = int(np.argmax(r["counts"]))
    last = len(a["draws"][0]) - 1
    assert k < last
    a["draws"][0, last] = a["draws"][0, k]
    s["no_more"] = a
    s["n_equals_min"] = scene(5, N=15, inlier_frac=1.0)                                      # one iteration, and 15 > 15 never holds
    s["n_below_min"] = scene(6, N=10, max_iters=4)
    s["n2"] = scene(7, N=2, min_inliers=0, max_iters=4)
    s["capped"] = scene(8, inlier_frac=0.3, max_iters=20)                                    # the table says 92, the draws hold 20
    s["its65"] = scene(9, inlier_frac=0.3, max_iters=65)
    s["scaled"] = scene(10, scale=1.3, inlier_frac=0.9)
    s["fixed"] = scene(11, scale=1.3, inlier_frac=0.9, fix_scale=True)
    s["fixed_unit"] = scene(12, scale=1.0, inlier_frac=0.9, fix_scale=True)
    a = scene(13, inlier_frac=1.0, noise=0.0)                                                # iteration 0 draws (0, 0, 0): compact 0, N - 1, N - 2, made collinear
    sl = a["slots"]
    for k, lam in ((len(sl) - 1, 0.5), (len(sl) - 2, 1.75)):
        for rows in (a["point1"][sl], a["matched"][0][sl]):
            a["points"][rows[k]] = a["points"][rows[0]] + F(lam) * (a["points"][rows[1]] - a["points"][rows[0]])
    a["draws"][0, 0] = 0
    s["collinear"] = a
    a = scene(14, inlier_frac=1.0)                                                           # draws outside 0 .. rand_max are clamped; compact 0 and N - 1 are two equal points
    sl = a["slots"]
    a["point1"][sl[-1]] = a["point1"][sl[0]]; a["matched"][0, sl[-1]] = a["matched"][0, sl[0]]
    a["draws"][0, 0] = (-5, -7, 2 ** 31 - 1)                                                 # positions 0, 0 (now holding N - 1) and the last
    s["equal_points"] = a
    a = scene(15, inlier_frac=1.0, same_frame=True)                                          # an exactly zero rotation: both keyframes see the same rows in one frame
    a["matched"][0, a["slots"]] = a["point1"][a["slots"]]
    s["zero_rotation"] = a
    a = scene(16, inlier_frac=0.9)                                                           # a NaN point at compact 0, drawn by iteration 0
    a["points"][a["matched"][0, a["slots"][0]], 1] = np.nan
    a["draws"][0, 0] = 0
    s["nan_point"] = a
    s["big"] = scene(17, n1=300, M=700, N=261, inlier_frac=0.5)                              # 300 iterations: the formula's count is clamped by max_its
    s["big_outliers"] = scene(18, n1=300, M=700, N=261, inlier_frac=0.0)
    for k, v in s.items():
        v["name"] = k
    return s


EXPECT = dict(first="CONVERGED", after20="CONVERGED", after64="CONVERGED", no_more="NO_MORE", n_equals_min="NO_MORE", n_below_min="TOO_FEW", n2="TOO_FEW",
              capped="NO_MORE", its65="NO_MORE", scaled="CONVERGED", fixed="NO_MORE", fixed_unit="CONVERGED", collinear="CONVERGED", equal_points="CONVERGED",
              zero_rotation="CONVERGED", nan_point="CONVERGED", big="CONVERGED", big_outliers="NO_MORE")


def family(seed=30):
    """B = 3 candidates against one current keyframe: one converges, one is all outliers, one has too few correspondences"""
    s = scene(seed, M=300, B=3, inlier_frac=0.8)
    rng = np.random.RandomState(seed)
    for i1 in s["slots"]:                                                                    # candidate 1: every point moved away
        s["points"][s["matched"][1, i1]] += rng.uniform(5, 30, 3).astype(F)
    s["matched"][2, s["slots"][8:]] = -1                                                     # candidate 2: eight correspondences
    return s


def random_scenes(count=200, seed=2000):
    rng = np.random.RandomState(seed)
    out = []
    for k in range(count):
        N = int(rng.randint(16, 40))
        out.append(scene(seed + k, n1=N + int(rng.randint(0, 12)), M=120, N=N, inlier_frac=float(rng.uniform(0.5, 1.0)), scale=float(rng.uniform(0.7, 1.4)),
                         deg=float(rng.uniform(1, 30)), fix_scale=bool(k % 5 == 4), max_iters=12))
    return out


def merge_scene(seed=40, J=3, n1=70, n2=80, M=200):
    """match12 [J][n1], point2 [J][n2]: points seen by two covisibles (the first entry owns), a slot a later covisible overwrites with a new point,
    a slot whose later entry is no owner and so keeps the earlier point, matches outside 0 .. n2 - 1, keypoints without a point, rows outside the table"""
    rng = np.random.RandomState(seed)
    point2 = rng.randint(0, M - 20, (J, n2)).astype(np.int32)                                       # the rows of the hand-made entries below are above these
    point2[rng.rand(J, n2) < 0.2] = -1
    match12 = rng.randint(0, n2, (J, n1)).astype(np.int32)
    match12[rng.rand(J, n1) < 0.4] = -1
    match12[2, [3, 9, 20, 40]] = -1; match12[0, 40] = -1
    match12[0, 3], match12[1, 3], point2[0, 5], point2[1, 6] = 5, 6, M - 9, M - 8                          # slot 3: covisible 1 overwrites with a new point
    point2[0, 7] = M - 7; match12[0, 9] = 7; match12[1, 9] = 8; point2[1, 8] = M - 7                       # slot 9 at covisible 1 sees the same point again: no owner
    match12[0, 20], point2[0, 21] = 21, M - 6; match12[1, 40], point2[1, 41] = 41, M - 6                   # one point at two covisibles and two slots: (0, 20) owns
    for j, k in ((0, 3), (1, 3), (0, 9), (1, 9), (0, 20), (1, 40)):                                        # no other slot of the covisible reaches these keypoints
        dup = np.nonzero(match12[j] == match12[j, k])[0]
        match12[j, dup[dup != k]] = -1
    match12[2, 30], match12[2, 31] = n2, -4
    point2[2, 50], match12[2, 33] = M + 3, 50
    return dict(match12=match12, point2=point2, M=M)


# ---- running the library -------------------------------------------------------------------------------------------------------------------
GUARD = 256
OUT_DTYPES = dict(header=np.int32, floats=F, inliers=np.uint8, Tcw=F, Ow=F)


def host_of(s, **kw):
    from xfeatslam_amd.extractor import Context
    a = dict(min_inliers=s["min_inliers"], fix_scale=s["fix_scale"], max_err1=s["max_err"], max_err2=s["max_err"])
    a.update(kw)
    d = s["draws"] if len(s["draws"]) > 1 else s["draws"][0]
    return Context.sim3_solve_host(camera(s["cam1"]), camera(s["cam2"]), s["points"], s["point1"], s["matched"], s["T1w"], s["T2w"], s["table"], d, RAND_MAX, **a)


def canonical_nan(a):
    a = np.array(a, F)
    a[np.isnan(a)] = F(np.nan)
    return a


def assert_equals_rule(got, want, b=0, prior_byte=None):
    """problem b of a result against the rule's dict: integers equal, floats by their bits (a NaN equals any NaN: IEEE fixes no payload and the sign
    and payload of an invalid operation's result differ between processors).  prior_byte: what the buffers held before the call, for
    the outputs the call must leave alone (everything but the header when TOO_FEW, the pose unless CONVERGED)"""
    for k in R.OUTPUTS:
        g = np.ascontiguousarray(got[k][b])
        if want[k] is None:
            if prior_byte is not None:
                assert np.all(g.view(np.uint8) == prior_byte), (k, "written although the call must leave it alone")
            continue
        w = np.ascontiguousarray(np.asarray(want[k], OUT_DTYPES[k]).reshape(g.shape))
        if g.dtype == F:
            g, w = canonical_nan(g), canonical_nan(w)
        bad = np.argwhere(g.view(np.uint8 if g.dtype.itemsize == 1 else np.uint32) != w.view(np.uint8 if w.dtype.itemsize == 1 else np.uint32))
        assert len(bad) == 0, (k, bad[:8].tolist(), g.ravel()[:12], w.ravel()[:12])


class Sim3SolveRig:
    """guarded runs of xfh_sim3_solve_device and xfh_sim3_merge_matches_device: every output and the workspace sit between guard bytes that must
    come back untouched"""

    def __init__(self, L):
        from xfeatslam_amd.extractor import Context
        self.L, self.ctx = L, Context(nfeatures=1, max_height=32, max_width=32)

    def close(self):
        self.ctx.close()

    def run(self, s, draws=None, T1w=None, num_matches=None, min_matches=0):
        """a scene (B = its number of candidates; draws [max_iters][3] = shared, stride 0; T1w [12] shared or [B][12]) -> (parsed outputs, raw bytes)"""
        import guarded
        from xfeatslam_amd import capi
        from xfeatslam_amd.extractor import Context
        matched = np.ascontiguousarray(s["matched"], np.int32)
        B, n1 = matched.shape
        draws = np.ascontiguousarray(s["draws"] if draws is None else draws, np.int32)
        T1w = np.ascontiguousarray(s["T1w"] if T1w is None else T1w, F)
        max_iters, M = draws.shape[-2], len(s["points"])
        ins = [s["points"], s["point1"], matched, T1w, s["T2w"], s["table"], draws] + ([np.array([num_matches], np.int32)] if num_matches is not None else [])
        bufs = [capi.DeviceBuffer(max(np.asarray(a).nbytes, 16)).upload(np.ascontiguousarray(a)) for a in ins]
        lay = Context.sim3_solve_layout(B, n1, GUARD)
        wsb = self.L.xfh_sim3_solve_workspace_bytes(n1, M, B)
        assert wsb > 0
        ws, out = guarded.Guarded(wsb, GUARD), guarded.outputs(lay)
        try:
            self.ctx.sim3_solve_device(B, n1, M, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, 0 if T1w.ndim == 1 else 12, bufs[4].ptr, camera(s["cam1"]),
                                       camera(s["cam2"]), bufs[5].ptr, max_iters, bufs[6].ptr, 0 if draws.ndim == 2 else max_iters * 3, RAND_MAX, ws.ptr, out.ptr,
                                       min_inliers=s["min_inliers"], fix_scale=s["fix_scale"], max_err1=s["max_err"], max_err2=s["max_err"], min_matches=min_matches,
                                       d_num_matches=bufs[7].ptr if num_matches is not None else None, guard=GUARD)
            self.ctx.synchronize()
            raw = guarded.download(out, lay)
            ws.download()
        finally:
            for b in bufs + [ws, out]:
                b.free()
        return lay.parse(raw), raw

    def merge(self, match12, point2, M):
        """-> (matched, matched_kf, num, raw bytes of the three outputs with their guards)"""
        import guarded
        from xfeatslam_amd import capi
        from xfeatslam_amd.extractor import Context
        match12, point2 = np.ascontiguousarray(match12, np.int32), np.ascontiguousarray(point2, np.int32)
        J, n1 = match12.shape
        n2 = point2.shape[1]
        lay = Context.sim3_merge_layout(n1, GUARD)
        bufs = [capi.DeviceBuffer(a.nbytes).upload(a) for a in (match12, point2)]
        ws, out = guarded.Guarded(self.L.xfh_sim3_solve_workspace_bytes(n1, M, 1), GUARD), guarded.outputs(lay)
        try:
            self.ctx.sim3_merge_matches_device(J, n1, n2, M, bufs[0].ptr, bufs[1].ptr, ws.ptr, *[out.ptr + lay[k] for k in lay.names])
            self.ctx.synchronize()
            raw = guarded.download(out, lay)
            ws.download()
        finally:
            for b in bufs + [ws, out]:
                b.free()
        a = lay.parse(raw)
        return a["matched"], a["matched_kf"], int(a["num_matches"][0]), raw
