"""Scenes for the two-view reconstruction tests: two pinhole views of synthetic points, the match list of SearchForInitialization's
format (matches12 [n1], -1 = none) and the raw draws a caller's rand() would give.  Together the scenes reach every status of the call."""
from __future__ import annotations

import numpy as np

import ref_twoview as R

F = np.float32
CAM = (F(458.654), F(457.296), F(367.215), F(248.375))          # fx, fy, cx, cy
W, H = 752, 480
RAND_MAX = 2147483647


def camera(cam=None):
    """the xfh_camera of a scene (its "cam" when it has one of its own) or of the rig"""
    from xfeatslam_amd import capi
    c = capi.Camera()
    c.fx, c.fy, c.cx, c.cy = [float(v) for v in (CAM if cam is None else cam)]
    c.width, c.height = W, H
    return c


def draws_of(seed: int, iters: int, force=()):
    """iters x 8 raw draws; the first carry 0 and RAND_MAX themselves.  force: {iteration: draws8} written over the random ones"""
    rng = np.random.RandomState(seed)
    d = rng.randint(0, RAND_MAX, size=(iters, 8), dtype=np.int64).astype(np.int32)
    d[0, 0], d[0, 1] = 0, RAND_MAX
    for it, v in dict(force).items():
        d[it] = v
    return d


def rot(axis, deg):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    t = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def project(X, Rm, t):
    fx, fy, cx, cy = [float(c) for c in CAM]
    Y = X @ Rm.T + t
    return np.stack([fx * Y[:, 0] / Y[:, 2] + cx, fy * Y[:, 1] / Y[:, 2] + cy], -1)


def points(rng, n, kind):
    fx, fy, cx, cy = [float(c) for c in CAM]
    u, v = rng.uniform(40, W - 40, n), rng.uniform(40, H - 40, n)
    if kind == "plane":
        z = 4.0 + 0.002 * (u - cx) + 0.001 * (v - cy)
    elif kind == "fronto":                                          # a plane facing the camera, seen after a motion along the axis
        z = np.full(n, 5.0)
    else:
        z = rng.uniform(2.0, 9.0, n)
    return np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], -1)


def scene(seed, n1, n2, n_match, kind="general", Rm=None, t=None, noise=0.3, outliers=0.1, iters=200, force=(), shuffle=True):
    """-> dict(xy1 [n1][2], xy2 [n2][2], m12 [n1], draws [iters][8], R, t, name)"""
    rng = np.random.RandomState(seed)
    Rm = rot([0.2, 1.0, 0.1], 3.0) if Rm is None else Rm
    t = np.array([0.5, 0.05, 0.1]) if t is None else np.asarray(t, float)
    X = points(rng, n_match, kind)
    a = project(X, np.eye(3), np.zeros(3)) + rng.normal(0, noise, (n_match, 2))
    b = project(X, Rm, t) + rng.normal(0, noise, (n_match, 2))
    n_out = int(round(outliers * n_match))
    if n_out:
        b[:n_out] = np.stack([rng.uniform(0, W, n_out), rng.uniform(0, H, n_out)], -1)
    xy1 = np.stack([rng.uniform(0, W, n1), rng.uniform(0, H, n1)], -1)
    xy2 = np.stack([rng.uniform(0, W, n2), rng.uniform(0, H, n2)], -1)
    i1 = rng.permutation(n1)[:n_match] if shuffle else np.arange(n_match)
    i2 = rng.permutation(n2)[:n_match] if shuffle else np.arange(n_match)
    xy1[i1], xy2[i2] = a, b
    m12 = np.full(n1, -1, np.int32)
    m12[i1] = i2
    return dict(xy1=xy1.astype(F), xy2=xy2.astype(F), m12=m12, draws=draws_of(seed + 1, iters, force), R=Rm, t=t, name=kind)


def rig():
    """name -> scene; the status each is built for is EXPECT[name], asserted in the tests.  With the same inliers the F score is never below the H
    score (a point near its image under H is near its epipolar line), so H wins where the F of a minimal set is poor: the H scenes have one to
    three iterations, found by a search over seeds."""
    s = {}
    s["general"] = scene(1, 301, 515, 220)                                                   # F wins
    s["plane"] = scene(134, 120, 140, 100, kind="plane", t=[0.6, 0.1, 0.05], noise=0.3, outliers=0.05, iters=1)       # H wins, one iteration
    s["rotation"] = scene(40, 301, 515, 220, Rm=rot([0.1, 1.0, 0.0], 4.0), t=[0, 0, 0], noise=0.5, outliers=0.0)       # no baseline: no hypothesis stands out
    s["small_baseline"] = scene(52, 301, 515, 220, t=[0.05, 0.0, 0.0], noise=0.1, outliers=0.05)                      # 5 cm at 2 .. 9 m: a clear winner, low parallax
    s["rotation_h"] = scene(101, 120, 140, 100, Rm=rot([0.1, 1.0, 0.0], 4.0), t=[0, 0, 0], noise=0.3, outliers=0.0, iters=1)    # H, four hypotheses alike
    s["still"] = scene(101, 120, 140, 100, kind="fronto", Rm=np.eye(3), t=[0, 0, 0], noise=2e-4, outliers=0.0, iters=1)         # H = identity: equal singular values
    s["ambiguous"] = scene(60, 301, 515, 120, kind="plane", Rm=np.eye(3), t=[0.02, 0.0, 0.0], noise=0.5, outliers=0.0)  # two hypotheses above 0.7 maxGood
    s["outliers"] = dict(scene(6, 301, 515, 200, outliers=1.0), sigma=1e-6)                  # nothing agrees with anything: both scores 0
    s["n7"] = scene(7, 65, 65, 7)
    s["n8"] = scene(8, 65, 65, 8, noise=0.0, outliers=0.0, iters=3)
    s["few"] = scene(9, 65, 65, 40, noise=0.1, outliers=0.0, iters=24)                       # fewer than 51 good points
    col = scene(10, 301, 515, 220)                                                           # iteration 0 draws eight collinear points
    cm1 = np.nonzero(col["m12"] >= 0)[0]
    i1 = [cm1[0]] + [cm1[len(cm1) - 1 - k] for k in range(7)]
    for k, i in enumerate(i1):
        col["xy1"][i] = (100.0 + 40.0 * k, 200.0)
        col["xy2"][col["m12"][i]] = (120.0 + 40.0 * k, 210.0)
    col["draws"][0] = 0                                                                       # draw 0 eight times: compact matches 0, N-1, N-2, ..
    s["collinear"] = col
    eq = scene(11, 301, 515, 220)                                                            # the best set of F (iteration 198) drawn again by 199
    eq["draws"][199] = eq["draws"][198]
    s["equal"] = eq
    nf = scene(12, 301, 515, 220)                                                           # one match at the epipole of both images: its A has rank 2
    i = np.nonzero(nf["m12"] >= 0)[0][3]
    fx, fy, cx, cy = [float(c) for c in CAM]
    c1 = -nf["R"].T @ nf["t"]                                                                 # centre of camera 2 seen by camera 1, and the reverse
    nf["xy1"][i] = (fx * c1[0] / c1[2] + cx, fy * c1[1] / c1[2] + cy)
    nf["xy2"][nf["m12"][i]] = (fx * nf["t"][0] / nf["t"][2] + cx, fy * nf["t"][1] / nf["t"][2] + cy)
    nf["epipole_idx1"] = int(i)
    s["epipole"] = nf
    # Non-finite triangulations.  With finite coordinates and a finite calibration the skip of CheckRT is out of reach: x3Dh is a unit vector from
    # the fp64 Jacobi, so |w| would have to fall below 3e-39 of it for x / w to overflow, and a non-finite COORDINATE spreads through Normalize
    # into every score (BOTH_ZERO, no CheckRT).  The calibration is not read before the motion step, so a NaN cy leaves matches, sets, fits, scores
    # and inliers as they are and makes E, every motion hypothesis and so the point of EVERY inlier non-finite: (1 / 0, 0 / 0, 0 / 0).
    s["nonfinite"] = dict(scene(13, 301, 515, 220), cam=(CAM[0], CAM[1], CAM[2], F(np.nan)))
    for k, v in s.items():
        v["name"] = k
        v.setdefault("sigma", 1.0)
    return s


EXPECT = dict(general="OK_F", plane="OK_H", rotation="F_NO_WINNER", small_baseline="LOW_PARALLAX", rotation_h="H_GATES", still="H_DEGENERATE", ambiguous="F_NO_WINNER", outliers="BOTH_ZERO",
              n7="TOO_FEW", n8="F_NO_WINNER", few="F_NO_WINNER", collinear="OK_F", equal="OK_F", epipole="OK_F", nonfinite="F_NO_WINNER")


def random_scenes(count=200, seed=1000):
    rng = np.random.RandomState(seed)
    out = []
    for k in range(count):
        kind = ("general", "plane")[k % 2]
        n = int(rng.randint(60, 120))
        out.append(dict(scene(seed + k, n + int(rng.randint(0, 20)), n + int(rng.randint(0, 20)), n, kind=kind, noise=0.2, outliers=0.1, iters=16), sigma=1.0))
    return out


# ---- running the library -------------------------------------------------------------------------------------------------------------------
GUARD = 256
OUT_DTYPES = dict(header=np.int32, floats=F, inl_h=np.uint8, inl_f=np.uint8, tri=np.uint8, p3d=F, matches_out=np.int32)


def rule_of(s, **kw):
    return R.rule(s["xy1"], s["xy2"], s["m12"], s.get("cam", CAM), s["draws"], RAND_MAX, sigma=s["sigma"], **kw)


def stack(scenes):
    """B scenes of one shape -> xy1 [B][n1][2], xy2 [B][n2][2], m12 [B][n1], draws [B][iters][8]"""
    return tuple(np.stack([np.asarray(s[k]) for s in scenes]) for k in ("xy1", "xy2", "m12", "draws"))


def assert_equals_rule(got, want, b=0, prior_byte=None):
    """problem b of a parsed result against the rule's dict: integers equal, floats by their bits.  prior_byte: what the buffers held before the call,
    for the outputs a TOO_FEW call must leave alone"""
    too_few = want["header"][1] == R.TOO_FEW
    for k in R.OUTPUTS:
        g = np.ascontiguousarray(got[k][b])
        if too_few and k != "header" and prior_byte is not None:
            assert np.all(g.view(np.uint8) == prior_byte), (k, "written by a TOO_FEW call")
            continue
        w = np.ascontiguousarray(np.asarray(want[k], OUT_DTYPES[k]).reshape(g.shape))
        bad = np.argwhere(g.view(np.uint8 if g.dtype.itemsize == 1 else np.uint32) != w.view(np.uint8 if w.dtype.itemsize == 1 else np.uint32))
        assert len(bad) == 0, (k, bad[:8].tolist(), g.ravel()[:8], w.ravel()[:8])


class TwoViewRig:
    """guarded runs of xfh_two_view_device: every output sits between guard bytes that must come back untouched"""

    def __init__(self, L):
        from xfeatslam_amd.extractor import Context
        self.L, self.ctx = L, Context(nfeatures=1, max_height=32, max_width=32)

    def close(self):
        self.ctx.close()

    def run(self, xy1, xy2, m12, draws, sigma=1.0, min_parallax_cos=None, min_tri=50, cam=None):
        """arrays with a leading B (draws [iters][8] = shared, stride 0) -> (parsed outputs, raw bytes)"""
        import guarded
        from xfeatslam_amd import capi
        from xfeatslam_amd.extractor import Context
        xy1, xy2, m12 = np.ascontiguousarray(xy1, F), np.ascontiguousarray(xy2, F), np.ascontiguousarray(m12, np.int32)
        draws = np.ascontiguousarray(draws, np.int32)
        B, n1, n2, iters = m12.shape[0], m12.shape[1], xy2.shape[1], draws.shape[-2]
        stride = 0 if draws.ndim == 2 else iters * 8
        lay = Context.two_view_layout(B, n1, GUARD)
        bufs = [capi.DeviceBuffer(max(a.nbytes, 16)).upload(a) for a in (xy1, xy2, m12, draws)]
        wsb = self.L.xfh_two_view_workspace_bytes(n1, n2, iters, B)
        assert wsb > 0
        ws, out = guarded.Guarded(wsb, GUARD), guarded.outputs(lay)
        try:
            self.ctx.two_view_device(B, n1, n2, camera(cam), bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, stride, iters, RAND_MAX, ws.ptr, out.ptr,
                                     sigma=sigma, min_parallax_cos=min_parallax_cos, min_triangulated=min_tri, guard=GUARD)
            self.ctx.synchronize()
            raw = guarded.download(out, lay)
            ws.download()
        finally:
            for b in bufs + [ws, out]:
                b.free()
        return lay.parse(raw), raw
