"""The SearchByProjection restatement (tests/ref_projection.py) on hand-made cases whose answers are written out here,
xfh_project_points against it by equality of bits, and the order dependence of the seeded scenes the GPU test uses (the frames
come from the CPU oracle's extraction here).  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import ref_frame as RF
import ref_projection as RP
import ref_window as RW
from xfeatslam_amd import capi, synth
from xfeatslam_amd.extractor import Context

F = np.float32
B640 = (0.0, 0.0, 640.0, 480.0)
I34 = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F)


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    import __graft_entry__ as g
    if not os.path.exists(capi.LIB_PATH):
        g.build()


def cam_struct(c):
    return capi.Camera(*[float(c[k]) for k in "fx fy cx cy k1 k2 p1 p2 k3 bf".split()], int(c["width"]), int(c["height"]))


def line_descriptors(values):
    """descriptors on one axis: DescriptorDistance(a, b) = (int)(512 * (a - b)^2) in fp32"""
    d = np.zeros((len(values), 64), F)
    d[:, 0] = values
    return d


def tiny(oracle_mod, tvals, qvals, claims, nn_ratio=0.0, th_high=1000, skip=None, txy=None):
    """targets on a line of descriptor space, all inside one window around (100, 100); every query sits on that spot"""
    nt, nq = len(tvals), len(qvals)
    x = np.full(nt, 100, F) + np.arange(nt, dtype=F); y = np.full(nt, 100, F)
    if txy is not None:
        x, y = (np.asarray(a, F) for a in txy)
    grid = RW.build(x, y, B640)
    st = np.full(nq, RP.VISIBLE, np.uint8)
    u = np.full(nq, 101, F); v = np.full(nq, 100, F)
    return RP.search(oracle_mod, st, np.asarray(claims, bool), u, v, F(15), np.zeros(nq, F), line_descriptors(qvals), grid, x, y, B640,
                     line_descriptors(tvals), skip=skip, init_dist=256, th_high=th_high, nn_ratio=nn_ratio)


def test_two_claiming_queries_share_a_best_keypoint(oracle_mod):
    # distances of both queries: keypoint 0 -> 0, keypoint 1 -> (int)(512 * 0.01) = 5, keypoint 2 -> (int)(512 * 0.09) = 46
    r = tiny(oracle_mod, [0.0, 0.1, 0.3], [0.0, 0.0], [True, True])
    assert r["match_idx"].tolist() == [0, 1] and r["status"].tolist() == [RP.MATCHED, RP.MATCHED]
    assert r["best_dist"].tolist() == [0, 5] and r["second_dist"].tolist() == [5, 46] and r["n_candidates"].tolist() == [3, 2]
    assert r["assigned"].tolist() == [0, 1, -1] and r["n_matches"] == 2


def test_a_non_claiming_query_is_overwritten(oracle_mod):
    r = tiny(oracle_mod, [0.0, 0.1, 0.3], [0.0, 0.0], [False, True])
    assert r["match_idx"].tolist() == [0, 0] and r["status"].tolist() == [RP.MATCHED, RP.MATCHED]
    assert r["assigned"].tolist() == [1, -1, -1] and r["n_matches"] == 2 and r["n_candidates"].tolist() == [3, 3]
    # a third query behind the claiming one must skip keypoint 0
    r = tiny(oracle_mod, [0.0, 0.1, 0.3], [0.0, 0.0, 0.0], [False, True, False])
    assert r["match_idx"].tolist() == [0, 0, 1] and r["assigned"].tolist() == [1, 2, -1] and r["n_matches"] == 3
    # a static skip mask is a claim made before the loop
    r = tiny(oracle_mod, [0.0, 0.1, 0.3], [0.0], [True], skip=np.array([1, 0, 0], np.uint8))
    assert r["match_idx"].tolist() == [1] and r["n_candidates"].tolist() == [2]


def test_ratio_rule_with_and_without_a_second(oracle_mod):
    # best 5, second 8: 5 > 0.6 * 8 -> rejected; 5 <= 0.9 * 8 -> matched
    t, q = [0.1, 0.126], [0.0]
    r = tiny(oracle_mod, t, q, [True], nn_ratio=0.6)
    assert r["best_dist"].tolist() == [5] and r["second_dist"].tolist() == [8]
    assert r["status"].tolist() == [RP.REJECTED] and r["match_idx"].tolist() == [-1] and r["n_matches"] == 0 and r["assigned"].tolist() == [-1, -1]
    assert tiny(oracle_mod, t, q, [True], nn_ratio=0.9)["match_idx"].tolist() == [0]
    assert tiny(oracle_mod, t, q, [True], nn_ratio=0.0)["match_idx"].tolist() == [0]           # the Frame-Frame form has no ratio
    # no second candidate (bestLevel2 == -1): accepted without the ratio
    r = tiny(oracle_mod, [0.1], q, [True], nn_ratio=0.6)
    assert r["match_idx"].tolist() == [0] and r["second_dist"].tolist() == [256]
    # a second above init_dist is no second either; th_high rejects on its own; no survivor under init_dist is rejected, not matched
    assert tiny(oracle_mod, [0.1, 0.9], q, [True], nn_ratio=0.6)["match_idx"].tolist() == [0]
    r = tiny(oracle_mod, [0.1], q, [True], th_high=4)
    assert r["status"].tolist() == [RP.REJECTED]
    r = tiny(oracle_mod, [0.9], q, [True])
    assert r["status"].tolist() == [RP.REJECTED] and r["best_dist"].tolist() == [256] and r["n_candidates"].tolist() == [1]
    # nothing in the window
    r = tiny(oracle_mod, [0.1], q, [True], txy=([400.0], [400.0]))
    assert r["status"].tolist() == [RP.NO_CANDIDATES] and r["n_candidates"].tolist() == [0]


def test_projection_special_values():
    cam = RF.camera(fx=1.0, fy=1.0, cx=0.0, cy=0.0, bf=40.0)
    b = (10.0, 20.0, 600.0, 400.0)
    z = np.array([-1.0, -0.0, 0.0, np.nan, 1.0], F)
    xyz = np.stack([np.full(5, 100, F) * np.where(np.isfinite(z), z, 1), np.full(5, 100, F) * np.where(np.isfinite(z), z, 1), z], 1).astype(F)
    xyz[1, :2] = -100                                       # every term of zc is -0.0 (with t_z = -0.0 below): the sum keeps the sign
    T0 = I34.copy(); T0[11] = -0.0
    u, v, ur, st = RP.project(T0, cam, b, xyz)
    # zc = -1 and -0.0: invz < 0 (-1 and -inf); +0.0: invz = +inf, u = 0 / 0 = NaN passes the cull; NaN: passes everything
    assert st.tolist() == [RP.BEHIND, RP.BEHIND, RP.VISIBLE, RP.VISIBLE, RP.VISIBLE]
    assert u[0] == 0 and u[1] == 0 and np.isnan(u[2]) and np.isnan(u[3]) and u[4] == 100 and ur[4] == 60
    # u exactly on min_x and on max_x is kept (the compare is strict), one ulp outside is culled; the same for v
    on = np.array([[10, 100, 1], [600, 100, 1], [100, 20, 1], [100, 400, 1]], F)
    off = on.copy()
    off[0, 0] = np.nextafter(F(10), F(0)); off[1, 0] = np.nextafter(F(600), F(1e9)); off[2, 1] = np.nextafter(F(20), F(0)); off[3, 1] = np.nextafter(F(400), F(1e9))
    assert RP.project(I34, cam, b, on)[3].tolist() == [RP.VISIBLE] * 4
    assert RP.project(I34, cam, b, off)[3].tolist() == [RP.OUT_OF_BOUNDS] * 4
    for pts in (xyz, on, off):
        uvr, lur, lst = Context.project_points(T0, cam_struct(cam), b, pts, 7.0)
        mu, mv, mur, mst = RP.project(T0, cam, b, pts)
        assert RF.same_bits(uvr[:, 0], mu) and RF.same_bits(uvr[:, 1], mv) and RF.same_bits(lur, mur) and np.array_equal(lst, mst) and np.all(uvr[:, 2] == 7)


def test_project_points_equals_the_restatement_bit_for_bit():
    rng = np.random.RandomState(12)
    n = 10000
    cam = RF.camera()
    b = tuple(float(x) for x in RF.bounds(cam))
    xyz = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(-1, 6, n)], 1).astype(F)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e38, -1e38, 1e-40, 3.4e38], F)
    for j in range(900):
        xyz[7 * j, j % 3] = special[(j // 3) % len(special)]
    for s in (1, 2, 3):
        T = RP.pose(s, cam=cam, angle=0.3)
        uvr, ur, st = Context.project_points(T, cam_struct(cam), b, xyz, 15.0)
        mu, mv, mur, mst = RP.project(T, cam, b, xyz)
        assert np.array_equal(st, mst)
        assert RF.same_bits(uvr[:, 0], mu) and RF.same_bits(uvr[:, 1], mv) and RF.same_bits(ur, mur) and np.all(uvr[:, 2] == 15)
        assert {RP.BEHIND, RP.OUT_OF_BOUNDS, RP.VISIBLE} <= set(st.tolist())
    T = RP.pose(1, cam=cam)
    T[5] = np.nan; T[11] = np.inf
    uvr, ur, st = Context.project_points(T, cam_struct(cam), b, xyz, 15.0)
    mu, mv, mur, mst = RP.project(T, cam, b, xyz)
    assert np.array_equal(st, mst) and RF.same_bits(uvr[:, 0], mu) and RF.same_bits(uvr[:, 1], mv) and RF.same_bits(ur, mur)
    L = capi.lib()
    p = xyz.ctypes.data
    assert L.xfh_project_points(None, C.byref(cam_struct(cam)), C.byref(capi.GridBounds(*b)), p, 1, 1.0, p, p, p) == 1
    assert L.xfh_project_points(p, None, C.byref(capi.GridBounds(*b)), p, 1, 1.0, p, p, p) == 1
    assert L.xfh_project_points(p, C.byref(cam_struct(cam)), C.byref(capi.GridBounds(*b)), p, -1, 1.0, p, p, p) == 1
    assert L.xfh_search_projection_workspace_bytes(4096, 4096, 2) == 2 * L.xfh_search_projection_workspace_bytes(4096, 4096, 1) > 0
    assert L.xfh_search_projection_device(None, 0, 1, 1, p, None, p, None, None, 1.0, p, p, p, p, 0, 1, None, None, 256, 1000, 0.0, p, p, p, p, p, p, None, p, p) == 1
    assert L.xfh_kernel_name(capi.K["PROJ_RESOLVE"]) == b"k_proj_resolve" and L.xfh_kernel_name(15) == b"k_frame_finish"


SCENES = [(900, 4096), (901, 1000)]                                   # (image seed, nfeatures) of the GPU test
SHIFT = (2, 1)                                                        # the current frame is the last one moved by (2, 1) pixels


def seeded_problem(oracle_mod, blob, seed, nf):
    """what tests/test_gpu_projection.py builds on the device, from the CPU oracle's extraction: (last, current) keypoints and
    descriptors, world points, flags, pose"""
    cam = RF.camera()
    img = synth.image(480, 640, seed)
    orc = oracle_mod.Oracle(blob)
    k0, d0, _, _ = orc.extract(img, nf, (0, 0))
    k1, d1, _, _ = orc.extract(np.roll(img, (SHIFT[1], SHIFT[0]), (0, 1)), nf, (0, 0))
    xy0 = RF.undistort(cam, np.stack([k0["x"], k0["y"]], 1)); xy1 = RF.undistort(cam, np.stack([k1["x"], k1["y"]], 1))
    xyz, flags = RP.scene(seed, xy0, cam)
    return cam, xy1, d0, d1, xyz, flags, RP.pose(seed, SHIFT, cam=cam)


@pytest.mark.parametrize("seed,nf", SCENES)
def test_seeded_scenes_are_order_dependent(oracle_mod, weights_dense, seed, nf):
    cam, xy1, d0, d1, xyz, flags, T = seeded_problem(oracle_mod, weights_dense[1], seed, nf)
    b = tuple(float(x) for x in RF.bounds(cam))
    x, y = xy1[:, 0].copy(), xy1[:, 1].copy()
    grid = RW.build(x, y, b)
    u, v, ur, st = RP.project(T, cam, b, xyz)
    st = np.where(flags & 1, st, RP.INACTIVE).astype(np.uint8)
    near = oracle_mod.distance_i32(d0[:256], d1).min(axis=1)
    print(f"seed {seed} nf {nf}: nearest DescriptorDistance of a query over the whole current frame: median {int(np.median(near))}, under 256: {np.mean(near < 256):.2f}")
    for r in (7.0, 15.0, 30.0):
        for init in (1 << 30, 256):
            with_claims = RP.search(oracle_mod, st, (flags & 2) != 0, u, v, F(r), ur, d0, grid, x, y, b, d1, init_dist=init)
            without = RP.search(oracle_mod, st, np.zeros(len(flags), bool), u, v, F(r), ur, d0, grid, x, y, b, d1, init_dist=init)
            active = st == RP.VISIBLE
            share = float(np.mean(with_claims["match_idx"][active] != without["match_idx"][active]))
            print(f"seed {seed} nf {nf} r {r} init_dist {init}: active {int(active.sum())}, matched {with_claims['n_matches']} / {without['n_matches']}, "
                  f"match_idx differs for {share:.3f} of the active queries")
            # the scenes as the GPU test searches them (init_dist = 1 << 30, th_high = 1000).  With the reference's 256 the synthetic weights'
            # descriptors admit few matches at all (printed above), and the share is printed, not asserted.
            if init != 256:
                assert share >= 0.05
