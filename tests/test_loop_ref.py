"""The restatements of the loop-closing and relocalisation matchers (tests/ref_loop.py) on hand-made cases whose answers are written out,
xfh_map_project and xfh_sim3_project against the restatements by equality of bits on points that sit ON every boundary and on random
points with specials, the argument checks of the stateless functions, kernel names and ids, and the conditions of the seeded scenes
the GPU test uses (the frames come from the CPU oracle's extraction here: this is where the seeds are chosen).  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ref_frame as RF
import ref_fuse as RU
import ref_loop as RL
import ref_projection as RP
import ref_window as RW
from xfeatslam_amd import capi, synth
from xfeatslam_amd.extractor import Context

F = np.float32
SF, NL = 1.2, 8
FORMS = sorted(RL.FORMS.items())
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    import __graft_entry__ as g
    if not os.path.exists(capi.LIB_PATH):
        g.build()


def cam_struct(c):
    return capi.Camera(*[float(c[k]) for k in "fx fy cx cy k1 k2 p1 p2 k3 bf".split()], int(c["width"]), int(c["height"]))


def both_map(T, Ow, cam, b, th, form, xyz, nr, dist, sf=SF, nl=NL):
    """xfh_map_project and the restatement on the same points: every output by equality of bits"""
    rmax = Context.scale_level_thresholds(sf, nl)
    uvr, lv, st = Context.map_project(T, Ow, cam_struct(cam), b, th, RU.scale_factors(sf, nl), rmax, form, xyz, nr, dist)
    mu, mv, mr, mlv, mst = RL.map_project(T, Ow, cam, b, th, sf, nl, form, xyz, nr, dist)
    assert np.array_equal(st, mst), (form, np.nonzero(st != mst)[0][:8])
    assert np.array_equal(lv, mlv), (form, np.nonzero(lv != mlv)[0][:8])
    assert RF.same_bits(uvr[:, 0], mu) and RF.same_bits(uvr[:, 1], mv) and RF.same_bits(uvr[:, 2], mr), form
    return mu, mv, mr, mlv, mst


def both_sim3(T, M, cam, b, th, xyz, dist, sf=SF, nl=NL):
    rmax = Context.scale_level_thresholds(sf, nl)
    uvr, lv, st = Context.sim3_project(T, M, cam_struct(cam), b, th, RU.scale_factors(sf, nl), rmax, xyz, dist)
    mu, mv, mr, mlv, mst = RL.sim3_project(T, M, cam, b, th, sf, nl, xyz, dist)
    assert np.array_equal(st, mst), np.nonzero(st != mst)[0][:8]
    assert np.array_equal(lv, mlv), np.nonzero(lv != mlv)[0][:8]
    assert RF.same_bits(uvr[:, 0], mu) and RF.same_bits(uvr[:, 1], mv) and RF.same_bits(uvr[:, 2], mr)
    return mu, mv, mr, mlv, mst


def test_map_project_on_every_boundary():
    cam = RU.UNIT_CAM
    b = (10.0, 20.0, 600.0, 400.0)
    O0 = np.zeros(3, F)
    wide = lambda n: np.tile(np.array([0, np.inf, 1], F), (n, 1))
    S3, KF, RE = RL.FORM_SIM3, RL.FORM_SIM3_KF, RL.FORM_RELOC
    # zc = -1, -0.0, +0.0, NaN, 1
    z = np.array([-1.0, -0.0, 0.0, np.nan, 1.0], F)
    xyz = np.stack([np.full(5, 100, F) * np.where(np.isfinite(z), z, 1), np.full(5, 100, F) * np.where(np.isfinite(z), z, 1), z], 1).astype(F)
    xyz[1, :2] = -100
    T0 = RU.I34.copy(); T0[11] = -0.0
    for form in (S3, KF):
        u, v, r, lv, st = both_map(T0, O0, cam, b, 3.0, form, xyz, xyz.copy(), wide(5))
        assert st.tolist() == [RL.BEHIND, RL.OUT_OF_IMAGE, RL.OUT_OF_IMAGE, RL.OUT_OF_IMAGE, RL.VISIBLE]
        assert u[0] == 0 and np.isinf(u[1]) and np.isnan(u[2]) and np.isnan(u[3]) and u[4] == 100 and lv.tolist() == [-1, -1, -1, -1, 0]
    # the relocalisation form has no depth test (zc = -1 projects to (100, 100)) and its bounds let a NaN pass
    u, v, r, lv, st = both_map(T0, O0, cam, b, 3.0, RE, xyz, xyz.copy(), wide(5))
    assert st.tolist() == [RL.VISIBLE, RL.OUT_OF_IMAGE, RL.VISIBLE, RL.VISIBLE, RL.VISIBLE] and u[0] == 100 and np.isnan(u[2]) and np.isnan(u[3])
    # half-open against closed: on min is in for both, on max only for the closed bounds; one ulp outside is out for both
    on = np.array([[10, 100, 1], [600, 100, 1], [100, 20, 1], [100, 400, 1]], F)
    past = on.copy()
    past[0, 0] = np.nextafter(F(10), F(0)); past[1, 0] = np.nextafter(F(600), F(700)); past[2, 1] = np.nextafter(F(20), F(0)); past[3, 1] = np.nextafter(F(400), F(500))
    V, O = RL.VISIBLE, RL.OUT_OF_IMAGE
    for form in (S3, KF):
        assert both_map(RU.I34, O0, cam, b, 3.0, form, on, on.copy(), wide(4))[4].tolist() == [V, O, V, O]
        assert both_map(RU.I34, O0, cam, b, 3.0, form, past, past.copy(), wide(4))[4].tolist() == [O, O, O, O]
    assert both_map(RU.I34, O0, cam, b, 3.0, RE, on, on.copy(), wide(4))[4].tolist() == [V, V, V, V]
    assert both_map(RU.I34, O0, cam, b, 3.0, RE, past, past.copy(), wide(4))[4].tolist() == [O, O, O, O]
    # the two projections differ in the last bit on (5, 300, 3)
    p = np.array([[5, 300, 3]], F)
    assert both_map(RU.I34, O0, cam, b, 3.0, S3, p, p.copy(), wide(1))[0][0] == RL.bits(0x3fd55555)
    assert both_map(RU.I34, O0, cam, b, 3.0, KF, p, p.copy(), wide(1))[0][0] == RL.bits(0x3fd55556)
    # dist3D = 2 exactly: equal to min and to max is inside, one ulp past either is out, a NaN bound never excludes
    p = np.tile(np.array([100, 100, 1], F), (5, 1)); Ow = np.array([100, 100, -1], F)
    nr = np.tile(np.array([0, 0, 1], F), (5, 1))
    up, dn = np.nextafter(F(2), F(3)), np.nextafter(F(2), F(0))
    dist = np.array([[2, 2, 2], [up, 9, 2], [0, dn, 2], [2, np.nan, 2], [np.nan, np.nan, 2]], F)
    for form in (S3, KF, RE):
        assert both_map(RU.I34, Ow, cam, b, 3.0, form, p, nr, dist)[4].tolist() == [V, RL.OUT_OF_RANGE, RL.OUT_OF_RANGE, V, V]
    # dot = 0.5 * dist3D exactly passes, one ulp less is past 60 degrees, a NaN normal passes; the relocalisation form does not look
    nr = np.array([[0, 0, 0.5], [0, 0, np.nextafter(F(0.5), F(0))], [0, 0, np.nan], [0, 0, -1], [7, -7, 0.5]], F)
    d9 = np.tile(np.array([0, 9, 2], F), (5, 1))
    for form in (S3, KF):
        assert both_map(RU.I34, Ow, cam, b, 3.0, form, p, nr, d9)[4].tolist() == [V, RL.BAD_ANGLE, V, RL.BAD_ANGLE, V]
    assert both_map(RU.I34, Ow, cam, b, 3.0, RE, p, nr, d9)[4].tolist() == [V] * 5
    # the level thresholds and the undefined ratios
    rmax = Context.scale_level_thresholds(SF, NL)
    rat = np.array([1.0, rmax[0], np.nextafter(rmax[0], F(9)), rmax[1], np.nextafter(rmax[1], F(9)), np.nan, np.inf, 0.0, -1.0, 0.9], F)
    dist = np.stack([np.zeros(len(rat), F), np.full(len(rat), 9, F), (rat * F(2)).astype(F)], 1)
    n = len(rat)
    for form in (S3, KF, RE):
        u, v, r, lv, st = both_map(RU.I34, Ow, cam, b, 3.0, form, np.tile(p[0], (n, 1)), np.tile(np.array([0, 0, 1], F), (n, 1)), dist)
        assert np.all(st == V) and lv.tolist() == [0, 0, 1, 1, 2, 0, 7, 0, 0, 0]
        assert r.tolist() == [F(3) * RU.scale_factors(SF, NL)[l] for l in lv]


def specials(n, rng, arrays):
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e38, -1e38, 1e-40, 3.4e38], F)
    for j in range(600):
        a = arrays[j % len(arrays)]
        a[7 * j, (j // len(arrays)) % 3] = special[(j // 9) % len(special)]


def test_map_project_equals_the_restatement_bit_for_bit():
    rng = np.random.RandomState(12)
    n = 6000
    cam = RF.camera()
    b = tuple(float(x) for x in RF.bounds(cam))
    xyz = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(-1, 6, n)], 1).astype(F)
    nr = rng.randn(n, 3).astype(F); nr[:, 2] += 1
    dist = np.stack([rng.uniform(0, 3, n), rng.uniform(2, 9, n), rng.uniform(1, 9, n)], 1).astype(F)
    specials(n, rng, (xyz, nr, dist))
    for form in list(RL.FORMS.values()) + [0, 15, RL.PROJECT_INVZ | RL.BOUNDS_CLOSED]:
        for s in (1, 2):
            T = RP.pose(s, cam=cam, angle=0.3)
            st = both_map(T, RU.camera_centre(T), cam, b, 7.0, form, xyz, nr, dist)[4]
            want = {RL.OUT_OF_IMAGE, RL.OUT_OF_RANGE, RL.VISIBLE} | ({RL.BEHIND} if form & RL.CULL_BEHIND else set()) | ({RL.BAD_ANGLE} if form & RL.CHECK_ANGLE else set())
            assert want == set(st.tolist()), (form, set(st.tolist()))
        T = RP.pose(1, cam=cam); T[5] = np.nan; T[11] = np.inf
        both_map(T, np.array([np.nan, 1e38, 0], F), cam, b, 7.0, form, xyz, nr, dist)


def test_sim3_project_equals_the_restatement_bit_for_bit():
    rng = np.random.RandomState(13)
    n = 6000
    cam = RF.camera()
    b = tuple(float(x) for x in RF.bounds(cam))
    xyz = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(-1, 6, n)], 1).astype(F)
    dist = np.stack([rng.uniform(0, 3, n), rng.uniform(2, 9, n), rng.uniform(1, 9, n)], 1).astype(F)
    specials(n, rng, (xyz, dist))
    for s in (1, 2, 3):
        T1, T2, M21, M12 = RL.sim3_pair(s, cam)
        T1 = RP.pose(s, cam=cam, angle=0.3)
        for T, M in ((T1, M21), (T2, M12)):
            st = both_sim3(T, M, cam, b, 7.0, xyz, dist)[4]
            assert {RL.BEHIND, RL.OUT_OF_IMAGE, RL.OUT_OF_RANGE, RL.VISIBLE} == set(st.tolist())
    M = M21.copy(); M[5] = np.nan; M[11] = np.inf
    both_sim3(T1, M, cam, b, 7.0, xyz, dist)
    M = M21.copy(); M[8:11] = 0; M[11] = -0.0                                      # p2.z = +-0: not behind, u = +-Inf or NaN: out of the image
    st = both_sim3(T1, M, cam, b, 7.0, xyz, dist)[4]
    assert set(st.tolist()) <= {RL.OUT_OF_IMAGE, RL.BEHIND}
    # on the boundaries: unit camera, identity pose, M = 2 I: (100, 100, 1) -> p2 = (200, 200, 2), |p2| = sqrtf(80004)
    ucam, ub = RU.UNIT_CAM, (10.0, 20.0, 600.0, 400.0)
    M2 = np.array([2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 0], F)
    d3 = np.sqrt(F(80004), dtype=F)
    up, dn = np.nextafter(d3, F(1e9)), np.nextafter(d3, F(0))
    p = np.tile(np.array([100, 100, 1], F), (4, 1))
    dist = np.array([[d3, d3, 1], [up, 1e9, 1], [0, dn, 1], [0, 200, 1]], F)
    u, v, r, lv, st = both_sim3(RU.I34, M2, ucam, ub, 3.0, p, dist)
    assert st.tolist() == [RL.VISIBLE, RL.OUT_OF_RANGE, RL.OUT_OF_RANGE, RL.OUT_OF_RANGE] and u[0] == 100 and v[0] == 100
    on = np.array([[10, 100, 1], [600, 100, 1], [100, 20, 1], [100, 400, 1], [-100, -100, -1]], F)
    wide = np.tile(np.array([0, np.inf, 1], F), (5, 1))
    assert both_sim3(RU.I34, RU.I34, ucam, ub, 3.0, on, wide)[4].tolist() == [RL.VISIBLE, RL.OUT_OF_IMAGE, RL.VISIBLE, RL.OUT_OF_IMAGE, RL.BEHIND]


def test_stateless_functions_refuse_bad_arguments_and_kernel_ids():
    L = capi.lib()
    cam = RF.camera()
    b = tuple(float(x) for x in RF.bounds(cam))
    buf = np.zeros(64, F); p = buf.ctypes.data
    margs = lambda **kw: [kw.get("T", p), kw.get("O", p), kw.get("cam", C.byref(cam_struct(cam))), kw.get("b", C.byref(capi.GridBounds(*b))), 3.0, kw.get("sf", p), p,
                          kw.get("nl", 8), kw.get("form", 3), kw.get("xyz", p), p, p, kw.get("n", 1), kw.get("uvr", p), p, p]
    assert L.xfh_map_project(*margs()) == 0
    for kw in (dict(T=None), dict(O=None), dict(cam=None), dict(b=None), dict(sf=None), dict(nl=0), dict(nl=17), dict(n=-1), dict(form=16), dict(form=-1), dict(xyz=None),
               dict(uvr=None)):
        assert L.xfh_map_project(*margs(**kw)) == 1, kw
    assert L.xfh_map_project(*margs(n=0, xyz=None, uvr=None)) == 0
    sargs = lambda **kw: [kw.get("T", p), kw.get("M", p), kw.get("cam", C.byref(cam_struct(cam))), kw.get("b", C.byref(capi.GridBounds(*b))), 3.0, kw.get("sf", p), p,
                          kw.get("nl", 8), kw.get("xyz", p), p, kw.get("n", 1), kw.get("uvr", p), p, p]
    assert L.xfh_sim3_project(*sargs()) == 0
    for kw in (dict(T=None), dict(M=None), dict(cam=None), dict(b=None), dict(sf=None), dict(nl=0), dict(nl=17), dict(n=-1), dict(xyz=None), dict(uvr=None)):
        assert L.xfh_sim3_project(*sargs(**kw)) == 1, kw
    assert Context.map_projection_search_workspace_bytes(0, 8, 1) == 0 and Context.map_projection_search_workspace_bytes(8, 8, 0) == 0
    assert Context.map_projection_search_workspace_bytes(8, capi.GRID_MAX_N + 1, 1) == 0
    w1, w4 = Context.map_projection_search_workspace_bytes(1000, 1000, 1), Context.map_projection_search_workspace_bytes(1000, 1000, 4)
    assert w1 % 256 == 0 and w4 % 256 == 0 and w1 >= Context.search_projection_workspace_bytes(1000, 1000, 1) + 4000 and w4 >= 4 * (w1 - 4096)
    # without a ctx the searches refuse before they touch anything
    side = capi.Sim3Side(8, p, p, p, 0, p, p, p, p, p, p, p, p, p, p, p, None)
    cs, bs = cam_struct(cam), capi.GridBounds(*b)
    assert L.xfh_sim3_search_device(None, 1, 0, C.byref(side), C.byref(side), p, p, C.byref(cs), C.byref(bs), 3.0, p, p, 8, 1000, p, p) == 1
    assert L.xfh_sim3_search(None, C.byref(side), C.byref(side), p, p, C.byref(cs), C.byref(bs), 3.0, p, p, 8, 1000, p, p) == 1
    assert L.xfh_map_projection_search_device(None, 3, 1, 8, p, p, p, p, p, p, p, C.byref(cs), C.byref(bs), 3.0, p, p, 8, p, p, 0, 0, 8, None, 256, 100.0, p, p, p, p,
                                              p, p, p, None, p, p) == 1
    assert L.xfh_map_projection_search(None, 3, 8, p, p, p, p, p, p, p, C.byref(cs), C.byref(bs), 3.0, p, p, 8, p, p, 8, None, 256, 100.0, p, p, p, p, p, p, None, p,
                                       p) == 1
    K = capi.K
    assert (K["MAPPROJ_CANDIDATES"], K["SIM3_SEARCH"], K["SIM3_AGREE"]) == (23, 24, 25)
    assert [L.xfh_kernel_name(i) for i in (23, 24, 25, 26)] == [b"k_mapproj_candidates", b"k_sim3_search", b"k_sim3_agree", b"?"]
    assert L.xfh_kernel_name(22) == b"k_bow_resolve" and L.xfh_kernel_name(17) == b"k_proj_resolve"       # existing ids keep their values
    assert (capi.MAPPROJ_FORM_SIM3, capi.MAPPROJ_FORM_SIM3_KF, capi.MAPPROJ_FORM_RELOC) == (RL.FORM_SIM3, RL.FORM_SIM3_KF, RL.FORM_RELOC)
    assert (capi.MAPPROJ_MATCHED, capi.MAPPROJ_VISIBLE, capi.SIM3_FOUND, capi.SIM3_VISIBLE) == (7, 5, 7, 5)


def test_project_functions_and_argument_checks_under_sanitizers(tmp_path):
    """xfh_map_project / xfh_sim3_project on heap buffers of exactly the documented sizes, against mapproj_math.h / sim3_math.h compiled into
    the program, and the argument checks of the search calls with a NULL ctx: a stand-alone program built with AddressSanitizer + UBSan
    against the sanitizer build of the HOST code (make -C xfeatslam_amd/csrc asan; device code is not instrumented, nothing runs on a GPU)"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "xfeatslam_amd", "csrc"), "asan", "-s", "-j8"])
    exe = str(tmp_path / "asan_loop_test")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "xfeatslam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "asan_loop_test.cpp"),
                           "-L" + os.path.join(ROOT, "xfeatslam_amd"), "-lxfeat_hip_asan", "-Wl,-rpath," + os.path.join(ROOT, "xfeatslam_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "asan_loop_test ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


def test_hand_made_map_projection_cases(oracle_mod):
    cases = RL.handmade_map()
    assert len(cases) == 15 and all(len(k["x"]) <= 16 for _, k, _ in cases)
    for name, k, want in cases:
        m = RL.run_map_case(oracle_mod, k)
        for key, val in want.items():
            got = m[key] if np.isscalar(m[key]) else m[key].tolist()
            assert got == val, (name, key, got, val)


def test_hand_made_sim3_cases(oracle_mod):
    cases = RL.handmade_sim3()
    assert len(cases) == 5
    for name, k, want in cases:
        m = RL.run_sim3_case(oracle_mod, k)
        for key, val in want.items():
            got = m[key] if np.isscalar(m[key]) else m[key].tolist()
            assert got == val, (name, key, got, val)


SCENES = [(900, 4096), (901, 1000)]                                   # (image seed, nfeatures) of the GPU test
ACCEPT_SIM3 = float(F(RL.TH_LOW) * F(1.5))                            # LoopClosing's ratioHamming = 1.5
ACCEPT_RELOC = 100.0                                                  # Tracking::Relocalization's ORBdist
ACCEPT = dict(sim3=ACCEPT_SIM3, sim3_kf=ACCEPT_SIM3, reloc=ACCEPT_RELOC)


@pytest.fixture(scope="module")
def frames(oracle_mod, weights_dense):
    """frame 0 of projection_rig.Rig from the CPU oracle's extraction: undistorted keypoints, descriptors, bounds"""
    out = {}
    cam = RF.camera()
    orc = oracle_mod.Oracle(weights_dense[1])
    for seed, nf in SCENES:
        k0, d0, _, _ = orc.extract(synth.image(480, 640, seed), nf, (0, 0))
        out[seed] = (RF.undistort(cam, np.stack([k0["x"], k0["y"]], 1)), d0)
    return cam, tuple(float(x) for x in RF.bounds(cam)), out


@pytest.mark.parametrize("seed,nf", SCENES)
def test_map_projection_scenes_exercise_every_path(oracle_mod, frames, seed, nf):
    """what tests/loop_rig.py builds on the device, from the CPU oracle's extraction: problem 0 of the GPU test.  Per form and per th: every
    status the form has at least 16 times, levels 0, 1 and >= 2 among the searched, at least nf / 16 answers that the claim changes, at least
    nf / 8 matches, and at least 16 queries whose four best candidates are all taken when their turn comes -- that last one wherever a window
    CAN hold more than four keypoints: at th = 4 the largest searched window is 9.6 pixels wide (level 1), and with 1000 features no such
    window of these frames holds five keypoints (none in the image seeds 901 .. 924; the densest holds four), so there no candidate list is
    ever truncated and the condition cannot be met by any seed; the test asserts that this is the reason."""
    cam, b, fr = frames
    xy, desc = fr[seed]
    x, y = xy[:, 0].copy(), xy[:, 1].copy()
    T = RP.pose(seed, (0, 0), cam=cam)
    Ow = RU.camera_centre(T)
    rmax = Context.scale_level_thresholds(SF, NL)
    sc = RL.map_scene(oracle_mod, seed, xy, desc, cam, T, b, rmax)
    grid = RW.build(x, y, b)
    for fname, form in FORMS:
        for th in (4.0, 15.0):
            u, v, r, lv, st = RL.map_project(T, Ow, cam, b, th, SF, NL, form, sc["xyz"], sc["normals"], sc["dist"])
            st = np.where(sc["flags"] & 1, st, RL.INACTIVE).astype(np.uint8)
            seq = RL.map_search(oracle_mod, st, lv, u, v, r, sc["qdesc"], grid, x, y, b, desc, taken=sc["taken"], accept_max=ACCEPT[fname])
            free = RL.map_search(oracle_mod, st, lv, u, v, r, sc["qdesc"], grid, x, y, b, desc, taken=sc["taken"], accept_max=ACCEPT[fname], claim=False)
            counts = np.bincount(seq["status"], minlength=8)
            reach = st == RL.VISIBLE
            lvr = lv[reach]
            differs = int(((seq["status"] != free["status"]) | (seq["match_idx"] != free["match_idx"]) | (seq["best_dist"] != free["best_dist"]) |
                           (seq["n_tested"] != free["n_tested"])).sum())
            print(f"seed {seed} nf {nf} {fname} th {th}: statuses {counts.tolist()}, levels of the searched {np.bincount(lvr, minlength=NL).tolist()}, "
                  f"matches {seq['n_matches']} (claim-free {free['n_matches']}), answers that differ {differs}, four best taken {int(seq['redo'].sum())}")
            must = [s for s in range(8) if (s != RL.BEHIND or form & RL.CULL_BEHIND) and (s != RL.BAD_ANGLE or form & RL.CHECK_ANGLE)]
            assert np.all(counts[must] >= 16), counts
            assert (lvr == 0).sum() >= 16 and (lvr == 1).sum() >= 16 and (lvr >= 2).sum() >= 16
            assert differs >= nf // 16
            if nf == 4096 or th == 15.0:
                assert int(seq["redo"].sum()) >= 16
            else:
                assert max(len(m) for _, _, m, _ in sc["spots"]) <= 4 and seq["n_window"].max() <= 4          # (see the docstring)
            assert seq["n_matches"] >= nf // 8
            a = seq["assigned"]
            assert np.array_equal(np.sort(a[a >= 0]), np.nonzero(seq["status"] == RL.MATCHED)[0]) and not np.any(sc["taken"][a >= 0])


@pytest.mark.parametrize("seed,nf", SCENES)
def test_sim3_scenes_exercise_every_path(oracle_mod, frames, seed, nf):
    cam, b, fr = frames
    xy, desc = fr[seed]
    x, y = xy[:, 0].copy(), xy[:, 1].copy()
    grid = RW.build(x, y, b)
    rmax = Context.scale_level_thresholds(SF, NL)
    T1, T2, M21, M12 = RL.sim3_pair(seed, cam)
    s1 = RL.sim3_side(seed, xy, desc, xy, desc, cam, T1, M21, b, rmax)
    s2 = RL.sim3_side(seed + 1, xy, desc, xy, desc, cam, T2, M12, b, rmax)
    for th in (4.0, 15.0):
        res = []
        for q, T, M in ((s1, T1, M21), (s2, T2, M12)):
            u, v, r, lv, st = RL.sim3_project(T, M, cam, b, th, SF, NL, q["points"], q["dist"])
            st = np.where(q["flags"] & 1, st, RL.INACTIVE).astype(np.uint8)
            m = RL.sim3_search(oracle_mod, st, lv, u, v, r, q["mp_desc"], grid, x, y, b, desc)
            counts = np.bincount(m["status"], minlength=8)
            print(f"seed {seed} nf {nf} th {th}: statuses {counts.tolist()}, levels of the searched {np.bincount(lv[st == RL.VISIBLE], minlength=NL).tolist()}")
            # (at th = 15 hardly a window of these frames is empty: NO_CANDIDATES is asked for at th = 4, the radius the GPU test's counts rest on)
            assert np.all(counts[[0, 1, 2, 3, 6, 7] + ([5] if th == 4.0 else [])] >= 16) and counts[4] == 0, counts
            res.append(m)
        m12, nfound = RL.sim3_agree(res[0]["match"], res[1]["match"])
        dropped = int(((res[0]["match"] >= 0) & (m12 < 0)).sum())
        print(f"seed {seed} nf {nf} th {th}: agreed {nfound}, one-sided matches of side 1 dropped {dropped}")
        assert nfound >= nf // 8 and dropped >= 16
