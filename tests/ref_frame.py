"""numpy restatement of what the reference's RGB-D Frame constructor does between extraction and the first search (test
infrastructure, no GPU):

  Frame::UndistortKeyPoints     src/Frame.cc:940-973  -- cv::undistortPoints(src, dst, K, dist, Mat(), P = K), from OpenCV's documented
                                algorithm: float64, five fixed-point iterations (TermCriteria COUNT 5, no epsilon exit), one rounding
                                to fp32 per coordinate
  Frame::ComputeImageBounds     src/Frame.cc:975-1002
  Frame::ComputeStereoFromRGBD  src/Frame.cc:1177-1198, the depth conversion of Tracking.cc:577-581 / :1548
  and the grid of the result:   ref_window.build on the undistorted coordinates

Every float64 expression is written out operation by operation in the documented order (numpy never contracts a multiply and an
add); the fp32 depth arithmetic goes through np.float32.  `corrupt` switches in ONE deliberate mistake, for the tests that show the
checks would catch it.
"""
import numpy as np

import ref_window as RW

F = np.float32
D = np.float64

TUM1 = dict(fx=517.306408, fy=516.469215, cx=318.643040, cy=255.313989, k1=0.262383, k2=-0.953104, p1=-0.005358, p2=0.002628,
            k3=1.163314, bf=40.0, width=640, height=480)          # the reference's examples/RGB-D/TUM1.yaml
TUM1_DEPTH_FACTOR = 5000.0


def camera(**kw):
    """a camera dict with fp32-rounded parameters (what xfh_camera holds)"""
    c = dict(TUM1)
    c.update(kw)
    return {k: (int(v) if k in ("width", "height") else F(v)) for k, v in c.items()}


def undistort(cam, xy, iterations=5, corrupt=None, with_branch=False):
    """[n][2] fp32 -> [n][2] fp32.  with_branch: also the mask of points whose icdist went negative"""
    xy = np.asarray(xy, F).reshape(-1, 2)
    neg = np.zeros(len(xy), bool)
    if cam["k1"] == F(0):
        return (xy.copy(), neg) if with_branch else xy.copy()
    fx, fy, cx, cy = D(cam["fx"]), D(cam["fy"]), D(cam["cx"]), D(cam["cy"])
    k1, k2, p1, p2, k3 = D(cam["k1"]), D(cam["k2"]), D(cam["p1"]), D(cam["p2"]), D(cam["k3"])
    if corrupt == "swap_p":
        p1, p2 = p2, p1
    with np.errstate(all="ignore"):
        x0 = (xy[:, 0].astype(D) - cx) / fx
        y0 = (xy[:, 1].astype(D) - cy) / fy
        x, y = x0.copy(), y0.copy()
        live = np.ones(len(xy), bool)                       # points that have not taken the icdist < 0 exit
        for _ in range(iterations):
            r2 = x * x if corrupt == "r2_no_y" else x * x + y * y
            icdist = D(1) / (D(1) + ((k3 * r2 + k2) * r2 + k1) * r2)
            bad = live & (icdist < 0)
            dx = D(2) * p1 * x * y + p2 * (r2 + D(2) * x * x)
            dy = p1 * (r2 + D(2) * y * y) + D(2) * p2 * x * y
            nx = (x0 - dx) * icdist
            ny = (y0 - dy) * icdist
            go = live & ~bad
            x = np.where(go, nx, np.where(bad, x0, x))
            y = np.where(go, ny, np.where(bad, y0, y))
            live = go
            neg |= bad
        out = np.stack([(x * fx + cx).astype(F), (y * fy + cy).astype(F)], 1)
    return (out, neg) if with_branch else out


def distort(cam, xy):
    """the FORWARD radial-tangential model in float64 (pixel of the ideal point xy): shares no iteration with undistort"""
    xy = np.asarray(xy, D).reshape(-1, 2)
    fx, fy, cx, cy = D(cam["fx"]), D(cam["fy"]), D(cam["cx"]), D(cam["cy"])
    k1, k2, p1, p2, k3 = D(cam["k1"]), D(cam["k2"]), D(cam["p1"]), D(cam["p2"]), D(cam["k3"])
    x = (xy[:, 0] - cx) / fx; y = (xy[:, 1] - cy) / fy
    r2 = x * x + y * y
    cd = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
    xd = x * cd + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * cd + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return np.stack([xd * fx + cx, yd * fy + cy], 1)


def bounds(cam, **kw):
    """ComputeImageBounds -> (min_x, min_y, max_x, max_y) as fp32; std::min(a, b) = b < a ? b : a, std::max(a, b) = a < b ? b : a"""
    w, h = F(cam["width"]), F(cam["height"])
    if cam["k1"] == F(0):
        return (F(0), F(0), w, h)
    p = undistort(cam, np.array([[0, 0], [w, 0], [0, h], [w, h]], F), **kw)
    mn = lambda a, b: b if b < a else a
    mx = lambda a, b: b if a < b else a
    return (mn(p[0, 0], p[2, 0]), mn(p[0, 1], p[1, 1]), mx(p[1, 0], p[3, 0]), mx(p[2, 1], p[3, 1]))


def sample_depth(cam, img, xy, scale=1.0, corrupt=None):
    """imDepth(v, u) at [n][2] fp32 positions: fp32 image as it is, uint16 as (float)raw * scale with one fp32 rounding; 0 where the
    pixel ((int)v, (int)u) is outside the image (truncation: (-1, 0) is pixel 0)"""
    xy = np.asarray(xy, F).reshape(-1, 2)
    W, H = int(cam["width"]), int(cam["height"])
    u, v = xy[:, 0], xy[:, 1]
    with np.errstate(all="ignore"):
        ok = (u > F(-1)) & (u < F(W)) & (v > F(-1)) & (v < F(H))
    iu = np.where(ok, np.trunc(np.where(ok, u, 0)), 0).astype(np.int64); iv = np.where(ok, np.trunc(np.where(ok, v, 0)), 0).astype(np.int64)
    raw = np.asarray(img)[iv, iu]
    with np.errstate(all="ignore"):
        if raw.dtype == np.uint16:
            if corrupt == "scale_f64":
                d = (raw.astype(D) * (D(1) / D(TUM1_DEPTH_FACTOR))).astype(F)   # scaled in float64, rounded twice
            else:
                d = raw.astype(F) * F(scale)
        else:
            d = raw.astype(F)
    return np.where(ok, d, F(0)).astype(F)


def stereo(cam, xy_raw, xy_un, img, scale=1.0, corrupt=None):
    """ComputeStereoFromRGBD -> (depth[n], uright[n]) fp32; img None: the monocular constructor, -1 everywhere"""
    xy_raw = np.asarray(xy_raw, F).reshape(-1, 2); xy_un = np.asarray(xy_un, F).reshape(-1, 2)
    n = len(xy_raw)
    if img is None:
        return np.full(n, -1, F), np.full(n, -1, F)
    d = sample_depth(cam, img, xy_un if corrupt == "depth_at_undistorted" else xy_raw, scale, corrupt)
    with np.errstate(all="ignore"):
        pos = (d >= 0) if corrupt == "d_ge_0" else (d > 0)
        u = xy_raw[:, 0] if corrupt == "uright_from_raw" else xy_un[:, 0]
        ur = (u - F(cam["bf"]) / d).astype(F)
    return np.where(pos, d, F(-1)).astype(F), np.where(pos, ur, F(-1)).astype(F)


def grid(xy_un, b, use=None):
    """AssignFeaturesToGrid on mvKeysUn -> (cell_start, items)"""
    return RW.build(xy_un[:, 0], xy_un[:, 1], b, use)


def same_bits(a, b):
    """fp32 arrays equal bit for bit (NaN payloads aside: any NaN equals any NaN)"""
    a = np.asarray(a, F); b = np.asarray(b, F)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
