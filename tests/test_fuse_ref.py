"""The Fuse restatement (tests/ref_fuse.py) on hand-made cases whose answers are written out (tests/ref_fuse.py::handmade),
xfh_scale_level_thresholds against the expression it replaces, xfh_fuse_project against the restatement by equality of bits on points
that sit ON every boundary, and the conditions of the seeded scenes the GPU test uses (the frames come from the CPU oracle's
extraction here: this is where the seeds are chosen).  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import ref_frame as RF
import ref_fuse as RU
import ref_projection as RP
import ref_window as RW
from xfeatslam_amd import capi, synth
from xfeatslam_amd.extractor import Context

F = np.float32
SF, NL = 1.2, 8


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    import __graft_entry__ as g
    if not os.path.exists(capi.LIB_PATH):
        g.build()


def cam_struct(c):
    return capi.Camera(*[float(c[k]) for k in "fx fy cx cy k1 k2 p1 p2 k3 bf".split()], int(c["width"]), int(c["height"]))


def table_level(rmax, ratio):
    """the contract's level = #{ l : ratio > ratio_max[l] }"""
    with np.errstate(all="ignore"):
        return int((F(ratio) > rmax).sum())


@pytest.mark.parametrize("sf,nl", [(1.2, 8), (1.2, 1), (1.2, 2), (2.0, 16), (1.0001, 16), (1.5, 5)])
def test_level_thresholds_against_the_direct_expression(sf, nl):
    rmax = Context.scale_level_thresholds(sf, nl)
    assert len(rmax) == nl - 1 and np.all(np.isfinite(rmax)) and np.all(np.diff(rmax) > 0)
    ratios = [np.exp(x) for x in np.linspace(-3, 8, 4001)] + [1.0, float(F(sf)), 1e-45, 1e-38, 3.4e38, 0.5, 2.0]
    for t in rmax:                                                       # every threshold and +-1, +-2 ulp
        dn1 = np.nextafter(t, F(0)); up1 = np.nextafter(t, F(np.inf))
        ratios += [t, dn1, np.nextafter(dn1, F(0)), up1, np.nextafter(up1, F(np.inf))]
    for r in ratios:
        assert table_level(rmax, r) == RU.predict_level(F(r), sf, nl), (sf, nl, float(r))
    for t, l in zip(rmax, range(nl - 1)):                                # the definition: the LARGEST float whose expression is <= l
        assert RU.predict_level(t, sf, 64) <= l < RU.predict_level(np.nextafter(t, F(np.inf)), sf, 64)
    # where the reference's (int) conversion is undefined: NaN -> 0, +Inf -> nlevels - 1, <= 0 -> 0
    assert table_level(rmax, np.nan) == 0 and table_level(rmax, np.inf) == nl - 1
    assert table_level(rmax, 0.0) == 0 and table_level(rmax, -0.0) == 0 and table_level(rmax, -3.0) == 0 and table_level(rmax, -np.inf) == 0
    L = capi.lib()
    buf = np.zeros(16, F)
    for bad in ((1.2, 0), (1.2, 17), (1.0, 8), (0.9, 8), (float("nan"), 8), (float("inf"), 8), (-1.2, 8)):
        assert L.xfh_scale_level_thresholds(bad[0], bad[1], buf.ctypes.data) == 1, bad
    assert L.xfh_scale_level_thresholds(1.2, 8, None) == 1 and L.xfh_scale_level_thresholds(1.2, 1, None) == 0


def both(T, Ow, cam, b, th, xyz, nr, dist, sf=SF, nl=NL):
    """xfh_fuse_project and the restatement on the same points: every output by equality of bits"""
    rmax = Context.scale_level_thresholds(sf, nl)
    uvr, ur, lv, st = Context.fuse_project(T, Ow, cam_struct(cam), b, th, RU.scale_factors(sf, nl), rmax, xyz, nr, dist)
    mu, mv, mur, mr, mlv, mst = RU.project(T, Ow, cam, b, th, sf, nl, xyz, nr, dist)
    assert np.array_equal(st, mst), np.nonzero(st != mst)[0][:8]
    assert np.array_equal(lv, mlv), np.nonzero(lv != mlv)[0][:8]
    assert RF.same_bits(uvr[:, 0], mu) and RF.same_bits(uvr[:, 1], mv) and RF.same_bits(ur, mur) and RF.same_bits(uvr[:, 2], mr)
    return mu, mv, mur, mr, mlv, mst


def test_fuse_project_on_every_boundary():
    cam = RU.UNIT_CAM
    b = (10.0, 20.0, 600.0, 400.0)
    O0 = np.zeros(3, F)
    wide = lambda n: np.tile(np.array([0, np.inf, 1], F), (n, 1))
    # zc = -1, -0.0, +0.0, NaN, 1: only zc < 0 is behind; -0.0 and +0.0 go on (u = -100 / -0.0 = +Inf and 0 / 0 = NaN: out of the image), NaN is out of the image
    z = np.array([-1.0, -0.0, 0.0, np.nan, 1.0], F)
    xyz = np.stack([np.full(5, 100, F) * np.where(np.isfinite(z), z, 1), np.full(5, 100, F) * np.where(np.isfinite(z), z, 1), z], 1).astype(F)
    xyz[1, :2] = -100
    T0 = RU.I34.copy(); T0[11] = -0.0
    u, v, ur, r, lv, st = both(T0, O0, cam, b, 3.0, xyz, xyz.copy(), wide(5))
    assert st.tolist() == [RU.BEHIND, RU.OUT_OF_IMAGE, RU.OUT_OF_IMAGE, RU.OUT_OF_IMAGE, RU.VISIBLE]
    assert u[0] == 0 and ur[0] == 0 and np.isinf(u[1]) and np.isnan(u[2]) and np.isnan(u[3]) and u[4] == 100 and ur[4] == 60 and lv.tolist() == [-1, -1, -1, -1, 0]
    # u on min_x is in, on max_x is out (half-open); the same for v; one ulp inside max is in, one ulp below min is out
    on = np.array([[10, 100, 1], [600, 100, 1], [100, 20, 1], [100, 400, 1]], F)
    off = on.copy()
    off[0, 0] = np.nextafter(F(10), F(0)); off[1, 0] = np.nextafter(F(600), F(0)); off[2, 1] = np.nextafter(F(20), F(0)); off[3, 1] = np.nextafter(F(400), F(0))
    assert both(RU.I34, O0, cam, b, 3.0, on, on.copy(), wide(4))[5].tolist() == [RU.VISIBLE, RU.OUT_OF_IMAGE, RU.VISIBLE, RU.OUT_OF_IMAGE]
    assert both(RU.I34, O0, cam, b, 3.0, off, off.copy(), wide(4))[5].tolist() == [RU.OUT_OF_IMAGE, RU.VISIBLE, RU.OUT_OF_IMAGE, RU.VISIBLE]
    # dist3D = 2 exactly (Ow = (100, 100, -1), the point at (100, 100, 1)): equal to min and to max is inside, one ulp past either is out
    p = np.tile(np.array([100, 100, 1], F), (5, 1)); Ow = np.array([100, 100, -1], F)
    nr = np.tile(np.array([0, 0, 1], F), (5, 1))
    up, dn = np.nextafter(F(2), F(3)), np.nextafter(F(2), F(0))
    dist = np.array([[2, 2, 2], [up, 9, 2], [0, dn, 2], [2, np.nan, 2], [np.nan, np.nan, 2]], F)
    assert both(RU.I34, Ow, cam, b, 3.0, p, nr, dist)[5].tolist() == [RU.VISIBLE, RU.OUT_OF_RANGE, RU.OUT_OF_RANGE, RU.VISIBLE, RU.VISIBLE]
    # dot = 0.5 * dist3D exactly passes (the compare is '<'), one ulp less is past 60 degrees, a NaN normal passes
    nr = np.array([[0, 0, 0.5], [0, 0, np.nextafter(F(0.5), F(0))], [0, 0, np.nan], [0, 0, -1], [7, -7, 0.5]], F)
    assert both(RU.I34, Ow, cam, b, 3.0, p, nr, np.tile(np.array([0, 9, 2], F), (5, 1)))[5].tolist() == [RU.VISIBLE, RU.BAD_ANGLE, RU.VISIBLE, RU.BAD_ANGLE, RU.VISIBLE]
    # ratio = predict_distance / 2: 1.0, ratio_max[0], ratio_max[1], their successors, and the undefined cases
    rmax = Context.scale_level_thresholds(SF, NL)
    rat = np.array([1.0, rmax[0], np.nextafter(rmax[0], F(9)), rmax[1], np.nextafter(rmax[1], F(9)), np.nan, np.inf, 0.0, -1.0, 0.9], F)
    dist = np.stack([np.zeros(len(rat), F), np.full(len(rat), 9, F), (rat * F(2)).astype(F)], 1)
    n = len(rat)
    u, v, ur, r, lv, st = both(RU.I34, Ow, cam, b, 3.0, np.tile(p[0], (n, 1)), np.tile(np.array([0, 0, 1], F), (n, 1)), dist)
    assert np.all(st == RU.VISIBLE) and lv.tolist() == [0, 0, 1, 1, 2, 0, 7, 0, 0, 0]
    assert r.tolist() == [F(3) * RU.scale_factors(SF, NL)[l] for l in lv] and r[2] == F(3) * F(1.2)


def test_fuse_project_equals_the_restatement_bit_for_bit():
    rng = np.random.RandomState(12)
    n = 6000
    cam = RF.camera()
    b = tuple(float(x) for x in RF.bounds(cam))
    xyz = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(-1, 6, n)], 1).astype(F)
    nr = rng.randn(n, 3).astype(F); nr[:, 2] += 1
    dist = np.stack([rng.uniform(0, 3, n), rng.uniform(2, 9, n), rng.uniform(1, 9, n)], 1).astype(F)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e38, -1e38, 1e-40, 3.4e38], F)
    for j in range(600):
        (xyz, nr, dist)[j % 3][7 * j, (j // 3) % 3] = special[(j // 9) % len(special)]
    for s in (1, 2, 3):
        T = RP.pose(s, cam=cam, angle=0.3)
        st = both(T, RU.camera_centre(T), cam, b, 7.0, xyz, nr, dist)[5]
        assert set(range(RU.BEHIND, RU.VISIBLE + 1)) <= set(st.tolist())
    T = RP.pose(1, cam=cam); T[5] = np.nan; T[11] = np.inf
    both(T, np.array([np.nan, 1e38, 0], F), cam, b, 7.0, xyz, nr, dist)
    L = capi.lib()
    p = xyz.ctypes.data
    args = lambda **kw: [kw.get("T", p), kw.get("O", p), kw.get("cam", C.byref(cam_struct(cam))), C.byref(capi.GridBounds(*b)), 3.0, p, p, kw.get("nl", 8), p, p, p,
                         kw.get("n", 1), p, p, p, p]
    for kw in (dict(T=None), dict(O=None), dict(cam=None), dict(nl=0), dict(nl=17), dict(n=-1)):
        assert L.xfh_fuse_project(*args(**kw)) == 1, kw
    assert L.xfh_kernel_name(capi.K["FUSE_SEARCH"]) == b"k_fuse_search"
    assert L.xfh_fuse_search_device(None, 1, 1, 0, p, p, p, p, p, p, p, C.byref(cam_struct(cam)), C.byref(capi.GridBounds(*b)), 3.0, p, p, 8, p, p, 0, 1, None, 1, 256,
                                    100, p, p, p, p, p, p, None, p) == 1


def test_hand_made_candidate_sets(oracle_mod):
    cases = RU.handmade()
    assert len(cases) == 11
    for name, k, want in cases:
        m = RU.run_case(oracle_mod, k)
        for key, val in want.items():
            assert m[key].tolist() == val, (name, key, m[key].tolist(), val)
        assert m["n_fused"] == want["status"].count(RU.FUSED), name


SCENES = [(900, 4096), (901, 1000)]                                   # (image seed, nfeatures) of the GPU test
SHIFT = (0, 0)                                                        # problem 0: the keyframe is the frame the map points were made from


@pytest.mark.parametrize("seed,nf", SCENES)
def test_seeded_scenes_exercise_every_path(oracle_mod, weights_dense, seed, nf):
    """what tests/fuse_rig.py builds on the device, from the CPU oracle's extraction: problem 0 of the GPU test"""
    cam = RF.camera()
    img = synth.image(480, 640, seed)
    orc = oracle_mod.Oracle(weights_dense[1])
    k0, d0, _, _ = orc.extract(img, nf, (0, 0))
    k1, d1 = k0, d0                                                   # (few keypoints are detected again in a shifted frame: at 1000 features a quarter)
    raw1 = np.stack([k1["x"], k1["y"]], 1)
    xy0 = RF.undistort(cam, np.stack([k0["x"], k0["y"]], 1)); xy1 = RF.undistort(cam, raw1)
    rng = np.random.RandomState(seed + 7)                             # the depth images of projection_rig.Rig; frame 0 is the keyframe
    depth = rng.randint(1, 65536, (5, 480, 640)).astype(np.uint16)
    depth[rng.rand(5, 480, 640) < 1 / 3] = 0
    _, uright = RF.stereo(cam, raw1, xy1, depth[0], scale=F(1) / F(RF.TUM1_DEPTH_FACTOR))
    b = tuple(float(x) for x in RF.bounds(cam))
    T = RP.pose(seed, SHIFT, cam=cam)
    Ow = RU.camera_centre(T)
    rmax = Context.scale_level_thresholds(SF, NL)
    x, y = xy1[:, 0].copy(), xy1[:, 1].copy()
    xyz, nr, dist, flags = RU.scene(seed, xy0, cam, T, rmax, kf=(x, y, uright))
    grid = RW.build(x, y, b)
    u, v, _, _, _, _ = RU.project(T, Ow, cam, b, 3.0, SF, NL, xyz, nr, dist)
    near = oracle_mod.distance_i32(d0[:256], d1).min(axis=1)
    print(f"seed {seed} nf {nf}: nearest DescriptorDistance of a last-frame row over the whole keyframe: median {int(np.median(near))}, under 100: {np.mean(near <= 100):.2f}")
    d0 = RU.query_descriptors(seed, u, v, x, y, d1, d0)
    for th in (3.0, 7.0):
        u, v, ur, r, lv, st = RU.project(T, Ow, cam, b, th, SF, NL, xyz, nr, dist)
        st = np.where(flags & 1, st, RU.INACTIVE).astype(np.uint8)
        on = RU.search(oracle_mod, st, lv, u, v, r, ur, d0, grid, x, y, b, d1, uright=uright, chi2=True, init_dist=256)
        off = RU.search(oracle_mod, st, lv, u, v, r, ur, d0, grid, x, y, b, d1, uright=uright, chi2=False, init_dist=RU.INT_MAX)
        counts = np.bincount(on["status"], minlength=8)
        reach = st == RU.VISIBLE
        fused = on["status"] == RU.FUSED
        moved = int((fused & (on["best_idx"] != off["best_idx"])).sum())
        # the chi-square branches: candidates of the queries at level <= 1, by branch, skipped and kept
        sk = {True: [0, 0], False: [0, 0]}
        for q in np.nonzero(reach & (lv <= 1))[0]:
            c = RW.features_in_area(grid, x, y, u[q], v[q], r[q], b)
            if len(c):
                s = RU.chi2_skips(u[q], v[q], ur[q], x[c], y[c], uright[c])
                for stereo in (True, False):
                    m = (uright[c] >= 0) == stereo
                    sk[stereo][0] += int((s & m).sum()); sk[stereo][1] += int((~s & m).sum())
        print(f"seed {seed} nf {nf} th {th}: statuses {counts.tolist()}, levels of the searched {np.bincount(lv[reach], minlength=NL).tolist()}, "
              f"chi2 stereo skipped/kept {sk[True]}, mono {sk[False]}, fused {int(fused.sum())} (chi2 off: {off['n_fused']}), best_idx moves without chi2 for {moved} fused queries")
        assert np.all(counts >= 16), counts
        lvr = lv[reach]
        assert (lvr == 0).sum() >= 16 and (lvr == 1).sum() >= 16 and (lvr >= 2).sum() >= 16
        assert min(sk[True]) >= 1 and min(sk[False]) >= 1
        assert int(fused.sum()) >= nf // 8
        assert moved >= 1
        assert on["n_fused"] == int(fused.sum())
