"""Seeded scenes for the MLPnP solver (xfh_mlpnp_*) and the guarded device runs the GPU tests share.  A scene is one frame (n undistorted keypoints)
against B candidate keyframes, each with its own block of nq world points and its own pose: the points are the keypoints back-projected at random
depths (after pixel noise; wrong matches get a gross pixel offset), so keypoint i of the frame sees point assigned[b][i] of candidate b.  Shapes across
the boundaries of the kernels: n = 70 with N = 41 correspondences (a partial wave), n = 300 with N = 261 (a second 256-lane pass of the compaction and
of every fold, a fifth 64-lane pass of the count), N = 10 (== min_inliers_eff), N = 9 and 5 (too few), Refine sets of 11, 64, 65 and 257 inliers."""
import numpy as np

import ref_mlpnp as R

F = np.float32
CAM = (F(458.654), F(457.296), F(367.215), F(248.375))
RAND_MAX = 32767
MAX_ERR = float(F(1.0) * F(5.991))                                                           # mvLevelSigma2[0] * th2 in float


def camera(cam=None):
    from xfeatslam_amd import capi
    c = CAM if cam is None else cam
    return capi.Camera(fx=float(c[0]), fy=float(c[1]), cx=float(c[2]), cy=float(c[3]), width=752, height=480)


def rot(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.radians(deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def scene(seed, n=70, N=41, B=1, inliers=None, inlier_frac=0.7, noise=0.5, eps=0.5, min_inliers=10, max_its=300, max_iters=None, chunk=5, planar=False,
          behind=0, invalid=3):
    """-> dict(xy [n][2], assigned [B][n], points [B][nq][3], valid [B][nq], tables, draws [B][max_iters][6], poses [B] = (R, t), ...).  inliers: the exact
    number of correct matches per candidate (they get no noise when noise == 0), else round(inlier_frac * N)"""
    rng = np.random.RandomState(seed)
    nq = n + 8
    xy = np.stack([rng.uniform(20, 732, n), rng.uniform(20, 460, n)], 1)
    assigned, points, valid, poses = np.full((B, n), -1, np.int32), rng.uniform(-30, 30, (B, nq, 3)), np.ones((B, nq), np.uint8), []
    slots = np.sort(rng.choice(n, N, replace=False))
    for b in range(B):
        Rm, t = rot(rng.randn(3), rng.uniform(5, 40)), rng.uniform(-1.5, 1.5, 3)
        if planar:
            t[2] = 5.0                                                                      # the plane z = 0 lies in front of the camera
        K = int(round(inlier_frac * N)) if inliers is None else inliers
        good = np.zeros(n, bool)
        good[slots[rng.permutation(N)[:K]]] = True
        px = xy + noise * rng.randn(n, 2)
        px[~good] += rng.uniform(25, 80, ((~good).sum(), 2)) * rng.choice([-1, 1], ((~good).sum(), 2))
        rays = np.stack([(px[:, 0] - float(CAM[2])) / float(CAM[0]), (px[:, 1] - float(CAM[3])) / float(CAM[1]), np.ones(n)], 1)
        if planar:                                                                          # world points on z = 0: the depth along the ray follows
            # Xw = R^T (d ray - t); z = 0  <=>  d (R^T ray)_z = (R^T t)_z
            depth = (Rm.T @ t)[2] / (rays @ Rm)[:, 2]
            good &= depth > 0.5
            depth[~good] = rng.uniform(3, 9, (~good).sum())                                 # the wrong matches leave the plane: a set that holds one is not planar
        else:
            depth = rng.uniform(3, 9, n)
        sign = np.ones(n)
        if behind:
            sign[slots[rng.permutation(N)[:behind]]] = -1.0                                  # the same ray, behind the camera: Pinhole::project has no depth test
        Xc = rays * (depth * sign)[:, None]
        Xw = (Xc - t) @ Rm
        if planar:
            Xw[good, 2] = 0.0
        rows = rng.permutation(nq)[:n]
        points[b, rows] = Xw
        assigned[b, slots] = rows[slots]
        spare = np.nonzero(assigned[b] < 0)[0]
        for i in spare[:invalid]:                                                           # matches to points flagged bad: no correspondence
            assigned[b, i] = rows[i]
            valid[b, rows[i]] = 0
        for i, v in zip(spare[invalid:invalid + 3], (nq, nq + 7, -3)):                       # indices outside the block: none
            assigned[b, i] = v
        poses.append((Rm, t))
    tables = R.iterations_table(n, 0.99, min_inliers, max_its, 6, eps)
    max_iters = max(int(tables[0][N]), chunk, 1) if max_iters is None else max_iters
    draws = rng.randint(0, RAND_MAX + 1, (B, max_iters, 6)).astype(np.int32)
    return dict(xy=xy.astype(F), assigned=assigned, points=points.astype(F), valid=valid, tables=tables, draws=draws, poses=poses, cam=CAM, max_err=MAX_ERR,
                chunk=chunk, slots=slots, N=N, seed=seed)


def rule_of(s, b=0, **kw):
    a = dict(max_err=s["max_err"], chunk=s["chunk"], point_valid=s["valid"][b])
    a.update(kw)
    return R.rule(s["xy"], s["assigned"][b], s["points"][b], s["cam"], s["tables"], s["draws"][b if len(s["draws"]) > 1 else 0], RAND_MAX, **a)


def rig():
    s = {}
    s["n70"] = scene(1)                                                                      # N = 41, its 35
    s["n300"] = scene(2, n=300, N=261, inlier_frac=0.6)
    s["n_equals_min"] = scene(3, N=10, inliers=10, noise=0.0)                                # its 1, the loop still runs chunk = 5; Refine never exceeds 10: BEST
    s["n9"] = scene(4, N=9, max_iters=5)
    s["n5"] = scene(5, N=5, max_iters=5)
    s["its5"] = scene(6, eps=0.85, inlier_frac=0.95)
    s["its70"] = scene(7, eps=0.4, inlier_frac=0.6)
    s["none"] = scene(8, inliers=0)
    s["refine11"] = scene(9, n=40, N=20, inliers=11, noise=0.0)
    s["refine64"] = scene(10, n=140, N=100, inliers=64, noise=0.0)
    s["refine65"] = scene(11, n=140, N=100, inliers=65, noise=0.0)
    s["refine257"] = scene(12, n=300, N=261, inliers=257, noise=0.0)
    s["planar"] = scene(13, planar=True, inlier_frac=0.8, noise=0.3)
    s["behind"] = scene(14, inlier_frac=0.8, behind=6)
    for k, v in s.items():
        v["name"] = k
    return s


EXPECT = dict(n70="REFINED", n300="REFINED", n_equals_min="BEST", n9="TOO_FEW", n5="TOO_FEW", its5="REFINED", its70="REFINED", none="NONE", refine11="REFINED",
              refine64="REFINED", refine65="REFINED", refine257="REFINED", planar="REFINED", behind="REFINED")
ITS = dict(n70=35, n_equals_min=1, its5=5, its70=70)
REFINE_SETS = dict(refine11=11, refine64=64, refine65=65, refine257=257)


def family(seed=30):
    """B = 3 candidates against one frame: one refines, one is all wrong matches, one has too few correspondences"""
    s = scene(seed, B=3, inlier_frac=0.8)
    rng = np.random.RandomState(seed)
    sl = s["slots"]
    s["points"][1, s["assigned"][1, sl]] += rng.uniform(5, 30, (len(sl), 3)).astype(F)
    s["assigned"][2, sl[8:]] = -1
    return s


def random_scenes(count=200, seed=7000):
    """well-posed small scenes: 0.5 px of noise, 30 % wrong matches, 12 iterations of draws"""
    rng = np.random.RandomState(seed)
    out = []
    for k in range(count):
        N = int(rng.randint(14, 32))
        out.append(scene(seed + k, n=N + int(rng.randint(0, 8)), N=N, inlier_frac=0.7, noise=0.5, max_iters=12, invalid=1))
    return out


def literal_of(s, b=0, store_refined=True, eps=0.5):
    import ref_mlpnp_literal as LIT
    return LIT.MLPnPsolver(s["xy"], s["assigned"][b], s["points"][b], s["valid"][b], s["cam"], s["draws"][b if len(s["draws"]) > 1 else 0], RAND_MAX, s["max_err"],
                           store_refined, eps=eps)


def forms_deviation(scenes):
    """the rule against the literal form (with Refine's result stored) over scenes -> (largest |Tcw rule - Tcw literal| over the rotation entries, over
    the translation entries, scenes compared, scenes exempt because the two least eigenvalues of A^T A of the reported solve are within 1e-6 relative)"""
    rot_d = tr_d = 0.0
    used = exempt = 0
    for s in scenes:
        r, o = rule_of(s), literal_of(s).iterate(s["chunk"])
        if r["Tcw"] is None or o["Tcw"] is None:
            continue
        if o["gap"] < 1e-6:
            exempt += 1
            continue
        d = np.abs(np.asarray(r["Tcw"], np.float64) - np.asarray(o["Tcw"], np.float64)).reshape(3, 4)
        rot_d, tr_d, used = max(rot_d, float(d[:, :3].max())), max(tr_d, float(d[:, 3].max())), used + 1
    return rot_d, tr_d, used, exempt


def hostile(seed=40):
    """any ints and any floats: indices of +-2^31, draws out of range, NaN and Inf points and keypoints"""
    s = scene(seed, inlier_frac=0.8)
    sl = s["slots"]
    s["assigned"][0, sl[0]] = 2 ** 31 - 1
    s["assigned"][0, sl[1]] = -2 ** 31
    s["draws"][0, 0] = (-5, -7, 2 ** 31 - 1, -2 ** 31, 40000, 0)
    s["draws"][0, 1] = 0
    s["points"][0, s["assigned"][0, sl[2]], 1] = np.nan
    s["points"][0, s["assigned"][0, sl[3]], 0] = np.inf
    s["points"][0, s["assigned"][0, sl[4]]] = -np.inf
    s["xy"][sl[5], 0] = np.nan
    return s


# ---- running the library -------------------------------------------------------------------------------------------------------------------
GUARD = 256
OUT_DTYPES = dict(header=np.int32, Tcw=F, inliers=np.uint8, assigned_out=np.int32)


def host_of(s, **kw):
    from xfeatslam_amd.extractor import Context
    a = dict(max_err=s["max_err"], chunk=s["chunk"], point_valid=s["valid"])
    a.update(kw)
    d = s["draws"] if len(s["draws"]) > 1 else s["draws"][0]
    return Context.mlpnp_solve_host(camera(s["cam"]), s["xy"], s["assigned"], s["points"], s["tables"], d, RAND_MAX, **a)


def float_steps(a, b):
    """the distance of two float32 arrays in representable steps (a NaN equals a NaN)"""
    a, b = np.ascontiguousarray(a, F).ravel(), np.ascontiguousarray(b, F).ravel()
    key = lambda v: np.where(v.view(np.int32) < 0, np.int64(-2 ** 31) - v.view(np.int32).astype(np.int64), v.view(np.int32).astype(np.int64))
    d = np.abs(key(a) - key(b))
    d[np.isnan(a) & np.isnan(b)] = 0
    return d


def assert_equals_rule(got, want, b=0, prior_byte=None, steps=1):
    """problem b of a result against the rule's dict: integers and flags equal, Tcw within `steps` float32 steps.  prior_byte: what the buffers held
    before the call, for the outputs the call must leave alone (everything but the header when TOO_FEW, the pose unless REFINED or BEST)"""
    for k in R.OUTPUTS:
        g = np.ascontiguousarray(got[k][b])
        if want[k] is None:
            if prior_byte is not None:
                assert np.all(g.view(np.uint8) == prior_byte), (k, "written although the call must leave it alone")
            continue
        w = np.ascontiguousarray(np.asarray(want[k], OUT_DTYPES[k]).reshape(g.shape))
        if k == "Tcw":
            d = float_steps(g, w)
            assert d.max() <= steps, (k, d.tolist(), g, w)
        else:
            bad = np.argwhere(g != w)
            assert len(bad) == 0, (k, bad[:8].tolist(), g.ravel()[:16], w.ravel()[:16])


class MlpnpRig:
    """guarded runs of xfh_mlpnp_solve_device: every output and the workspace sit between guard bytes that must come back untouched"""

    def __init__(self, L):
        from xfeatslam_amd.extractor import Context
        self.L, self.ctx = L, Context(nfeatures=1, max_height=32, max_width=32)

    def close(self):
        self.ctx.close()

    def run(self, s, draws=None, start_iter=None, n_matches=None, min_matches=0, tables=None, chunk=None, valid=True):
        """a scene (B = its number of candidates; draws [max_iters][6] = shared, stride 0) -> (parsed outputs, raw bytes)"""
        import guarded
        from xfeatslam_amd import capi
        from xfeatslam_amd.extractor import Context
        assigned = np.ascontiguousarray(s["assigned"], np.int32)
        B, n = assigned.shape
        nq = s["points"].shape[1]
        draws = np.ascontiguousarray(s["draws"] if draws is None else draws, np.int32)
        tables = s["tables"] if tables is None else tables
        max_iters = draws.shape[-2]
        ins = [s["xy"], assigned, s["points"], s["valid"], np.asarray(tables[0], np.int32), np.asarray(tables[1], np.int32), draws,
               np.zeros(B, np.int32) if start_iter is None else np.asarray(start_iter, np.int32), np.zeros(B, np.int32) if n_matches is None else np.asarray(n_matches, np.int32)]
        bufs = [capi.DeviceBuffer(max(np.asarray(a).nbytes, 16)).upload(np.ascontiguousarray(a)) for a in ins]
        lay = Context.mlpnp_layout(B, n, GUARD)
        wsb = self.L.xfh_mlpnp_workspace_bytes(n, nq, B, max_iters)
        assert wsb > 0
        ws, out = guarded.Guarded(wsb, GUARD), guarded.outputs(lay)
        try:
            self.ctx.mlpnp_solve_device(B, n, nq, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr if valid else None, camera(s["cam"]), s["max_err"], bufs[4].ptr,
                                        bufs[5].ptr, s["chunk"] if chunk is None else chunk, None if start_iter is None else bufs[7].ptr, max_iters, bufs[6].ptr,
                                        0 if draws.ndim == 2 else max_iters * 6, RAND_MAX, ws.ptr, out.ptr, min_matches=min_matches,
                                        d_n_matches=None if n_matches is None else bufs[8].ptr, guard=GUARD)
            self.ctx.synchronize()
            raw = guarded.download(out, lay)
            ws.download()
        finally:
            for b in bufs + [ws, out]:
                b.free()
        return lay.parse(raw), raw
