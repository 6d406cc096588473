"""The triangulation call without a GPU: the two forms of tests/ref_triangulate.py against each other, the host entry point xfh_triangulate_pair and
the stand-alone sanitizer program (both compile xfeatslam_amd/csrc/triangulate_math.h, the kernels' own lines) against the rule by bits, the two
stated deviations measured against their derived bounds, the conditions the scenes of tests/triangulate_rig.py are chosen for, hand-made pairs with
written-out answers and every class of refusal that needs no device."""
import collections
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_triangulate as RG
import triangulate_rig as R
from conftest import ROOT
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context

F, D = np.float32, np.float64


@pytest.fixture(scope="module")
def main(oracle_mod):
    s = R.main_scene()
    P = R.main_params()
    d = s.dists(oracle_mod)
    m = RG.snapshot_matches(d, s.k1, s.k2, s.F12, s.ep)
    return s, P, d, m, RG.rule_from_matches(P, s.k1, s.k2, m), RG.literal(P, d, s.k1, s.k2, s.F12, s.ep)


@pytest.fixture(scope="module")
def plant():
    o, m = R.planted()
    return o, m, R.planted_params(), RG.rule_from_matches(R.planted_params(), o.k1, o.k2, m, claim=False)


def forms_agree(w, l):
    """statuses (a SUPERSEDED pair of the rule was never searched by the literal form), kinds, winners and the creation order"""
    sup = w["status"] == RG.SUPERSEDED
    assert np.array_equal(w["status"][~sup], l["status"][~sup]) and not l["status"][sup].any()
    assert np.array_equal(w["kind"][~sup], l["kind"][~sup])
    lst = [(int(w["new_idx1"][j]), int(w["new_b"][j]), int(w["new_idx2"][j])) for j in range(w["n_new"])]
    assert lst == [(c[0], c[1], c[2]) for c in l["created"]]
    win = np.full(len(w["winner"]), -1)
    for i, b, *_ in l["created"]:
        win[i] = b
    assert np.array_equal(win, w["winner"]) and np.all(w["new_idx1"][w["n_new"]:] == -1)
    assert lst == sorted(lst, key=lambda e: (e[1], e[0]))                                               # b ascending, then idx1 ascending


def test_the_two_forms_agree_on_the_scene(main):
    s, P, d, m, w, l = main
    forms_agree(w, l)
    # floats: the two forms differ only by LAPACK's float32 SVD and libm's cosine -- a few float steps of the point, never a decision
    worst = max(float(np.abs(c[3] - w["new_xyz"][j]).max()) for j, c in enumerate(l["created"]))
    print(f"main scene: {w['n_new']} new points, headers {w['header'].tolist()}, largest |x3D(rule) - x3D(literal)| = {worst:.3g} m")


def test_the_two_forms_agree_on_200_random_scenes():
    tot = collections.Counter()
    for seed in range(200):
        s = R.small_scene(1000 + seed)
        P = R.main_params(far_th=20.0, inertial=bool(seed % 2))
        d = s.dists()
        w = RG.rule(P, d, s.k1, s.k2, s.F12, s.ep)
        forms_agree(w, RG.literal(P, d, s.k1, s.k2, s.F12, s.ep))
        tot.update(RG.NAMES[x] for x in w["status"].ravel())
    print(dict(tot))
    assert tot["ACCEPTED"] > 1000 and tot["SUPERSEDED"] > 1000 and tot["FAR"] > 100 and tot["LOW_PARALLAX"] > 100


def c_pair(cam, P, o1, o2):
    kf = lambda o: dict(xy=(o["x"], o["y"]), xy_raw=(o["xr"], o["yr"]), ur=o["ur"], depth=o["depth"], Tcw=o["T"], Ow=o["Ow"])
    return Context.triangulate_pair(cam, kf(o1), kf(o2), sigma2=P["sigma2"], ratio_factor=P["ratio_factor"], scale_last=P["scale_last"], far_th=P["far_th"],
                                    inertial=P["inertial"])


def same_pair(c, r, o1, o2, P, tag):
    assert c["status"] == r["status"] and c["kind"] == r["kind"], (tag, c["status"], r["status"])
    assert c["x3D"].tobytes() == r["x3D"].tobytes() and c["x3Dh"].tobytes() == r["x3Dh"].tobytes(), (tag, c["x3D"], r["x3D"])
    nrm, dst = RG.normal_depth(r["x3D"], o1["Ow"], o2["Ow"], P["scale_last"]) if r["status"] == RG.ACCEPTED else (np.zeros(3, F), np.zeros(3, F))
    assert c["normal"].tobytes() == nrm.tobytes() and c["dist"].tobytes() == dst.tobytes(), tag


def test_host_pair_equals_the_rule_by_bits(main, plant):
    s, P, d, m, w, _ = main
    cam = R.cam_struct()
    n = 0
    for (b, i), r in w["info"].items():
        o1, o2 = RG.obs(s.k1, i), RG.obs(s.k2[b], int(m[b][i]))
        same_pair(c_pair(cam, P, o1, o2), r, o1, o2, P, (b, i)); n += 1
    o, mp, Pp, wp = plant
    for (b, i), r in wp["info"].items():
        o1, o2 = RG.obs(o.k1, i), RG.obs(o.k2[b], int(mp[b][i]))
        same_pair(c_pair(cam, Pp, o1, o2), r, o1, o2, Pp, ("planted", b, i)); n += 1
    print(f"{n} pairs equal by bits")


def test_handmade_pairs():
    cam = R.cam_struct(R.HCAM)
    for name, o1, o2, kw, want in R.handmade():
        P = RG.params(R.HCAM, **dict(dict(ratio_factor=R.RATIO_FACTOR, scale_last=R.SCALE_LAST), **kw))
        r = RG.pair_rule(P, o1, o2)
        assert r["status"] == want["status"] and r["kind"] == want["kind"], (name, RG.NAMES[r["status"]], r["kind"])
        if "x3D" in want:
            assert RG.ulps(r["x3D"], np.array(want["x3D"], F)).max() <= want["tol"], (name, r["x3D"])
        same_pair(c_pair(cam, P, o1, o2), r, o1, o2, P, name)
        lit = RG.pair_rule(P, o1, o2, form="literal")
        assert lit["status"] == r["status"] or name == "w == 0", name       # (LAPACK's float32 w is tiny, not zero: its point is far behind the cameras)
    name, o1, o2, kw, _ = [c for c in R.handmade() if c[0] == "w == 0"][0]
    r = RG.pair_rule(RG.params(R.HCAM), o1, o2)
    assert np.array_equal(r["x3Dh"], [0, 0, 1, 0]) and np.all(r["A"][:, 2] == 0)


def test_null_vector_against_float64_svd(main, plant):
    """the rule's x3Dh against numpy's float64 SVD of the same float32 A.  Derived bound: the fp64 iteration's error (a few 1e-16) times the condition
    of the null vector (1 / gap, at most about 1e6 at the lowest parallax the branch lets through) stays orders below half a float step, so only a
    rounding boundary can differ: at most ONE float step of the largest component, in every component"""
    s, P, d, m, w, _ = main
    worst, n, worst64 = 0.0, 0, 0.0
    infos = list(w["info"].values()) + list(plant[3]["info"].values())
    for seed in range(40):
        sc = R.small_scene(3000 + seed)
        infos += list(RG.rule(R.main_params(far_th=0.0), sc.dists(), sc.k1, sc.k2, sc.F12, sc.ep)["info"].values())
    for r in infos:
        if r["A"] is None or not np.all(np.isfinite(r["A"])):
            continue
        ref = RG.lapack_null_vector(r["A"], D)
        x = r["x3Dh"]
        if np.dot(ref, x) < 0:
            ref = -ref
        step = np.spacing(F(np.abs(ref).max()))
        diff = np.abs(x.astype(F).astype(D) - ref.astype(F).astype(D)).max() / step
        worst, worst64, n = max(worst, diff), max(worst64, np.abs(x - ref).max()), n + 1
    print(f"{n} null vectors: largest difference to the float64 SVD after rounding to float = {worst:.2f} float steps of the largest component; before rounding {worst64:.3g}")
    assert n > 1000 and worst <= 1.0


def test_cosine_identity():
    """(z^2 - h^2) / (z^2 + h^2) in double, rounded once, against float32 cos(2 * arctan2(h, z)) over a dense depth grid, 0.1 .. 40 m at the rig's mb.
    Derived bound: two float32 libm calls of under one ulp each (atan2 near 0: the ulp of an angle <= 0.37; cos near 1: 6e-8) and one doubling give at
    most about 2e-7; 1e-6 leaves a factor of five"""
    P = R.main_params()
    z = np.concatenate([np.linspace(0.1, 40.0, 400001), np.geomspace(0.1, 40.0, 100001)]).astype(F)
    h = D(F(P["mb"] / F(2)))
    ident = ((z.astype(D) ** 2 - h * h) / (z.astype(D) ** 2 + h * h)).astype(F)
    libm = np.cos(F(2) * np.arctan2(np.full_like(z, F(P["mb"] / F(2))), z)).astype(F)
    worst = float(np.abs(ident.astype(D) - libm.astype(D)).max())
    print(f"cosine identity against float32 libm over {len(z)} depths: largest difference {worst:.3g}")
    assert worst < 1e-6
    assert all(RG.cos_identity(P["mb"], zz).tobytes() == ident[k].tobytes() for k, zz in list(enumerate(z))[::5000])


PROBES = [np.array(v, D) for v in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))] + \
         [np.array((a, b, c), D) for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)]


def conditions(P, k1, k2s, m, w):
    """per scene: the largest difference between the fp64 and the LAPACK-float32 point, the decisions under both, and the margins"""
    delta, pairs = 0.0, []
    for (b, i), r in w["info"].items():
        o1, o2 = RG.obs(k1, i), RG.obs(k2s[b], int(m[b][i]))
        lit = RG.pair_rule(P, o1, o2, form="literal")
        assert lit["status"] == r["status"] and lit["kind"] == r["kind"], (b, i)
        if r["A"] is not None and np.all(np.isfinite(r["x3D"])) and np.all(np.isfinite(lit["x3D"])) and r["status"] != RG.DEGENERATE:
            delta = max(delta, float(np.abs(r["x3D"].astype(D) - lit["x3D"].astype(D)).max()))
        pairs.append((b, i, o1, o2, r))
    cos_margin = 1.0
    for b, i, o1, o2, r in pairs:
        if np.isnan(r["cosRays"]):
            continue
        if r["st1"] or r["st2"]:                                           # the decisions a stereo cosine takes part in
            cs = min(r["cos1"], r["cos2"])
            cos_margin = min(cos_margin, abs(float(r["cosRays"]) - float(cs)), abs(float(r["cos1"]) - float(r["cos2"])))
        else:                                                              # and the ones the rays' summation order could move
            cos_margin = min(cos_margin, abs(float(r["cosRays"]) - (0.9996 if P["inertial"] else 0.9998)))
        if np.all(np.isfinite(r["x3D"])) and r["status"] >= RG.BEHIND1 and r["status"] != RG.ZERO_DIST:
            for v in PROBES:
                Xp = (r["x3D"].astype(D) + 8.0 * delta * v).astype(F)
                assert RG.gates(P, o1, o2, r["st1"], r["st2"], Xp) == r["status"], (b, i, RG.NAMES[r["status"]], delta)
    return delta, cos_margin


def test_conditions_of_the_scenes(main, plant):
    """asserted where the seeds are chosen: what the scenes are in the rig for, and that no decision sits near its boundary"""
    s, P, d, m, w, l = main
    o, mp, Pp, wp = plant
    snap = collections.Counter(RG.NAMES[x] for x in w["snapshot"].ravel()) + collections.Counter(RG.NAMES[x] for x in wp["snapshot"].ravel())
    print(dict(snap))
    assert set(snap) == set(RG.NAMES) - {"SUPERSEDED", "DEGENERATE"}       # (w == 0 needs a pose no keyframe has: the hand-made pair, on the GPU as n1 = n2 = 1)
    assert (w["status"] == RG.SUPERSEDED).sum() > 50
    kinds = {int(k) for k in w["kind"].ravel()} | {int(k) for k in wp["kind"].ravel()}
    assert kinds == {0, 1, 2}
    both = [(b, i) for (b, i), r in w["info"].items() if r["st1"] and r["st2"]]
    assert len(both) >= 5, "both-stereo pairs exercise the else-if"
    acc = w["snapshot"] == RG.ACCEPTED
    assert (acc.sum(0) >= 2).sum() >= 20, "an idx1 accepted at two neighbours: the claim decides"
    rej0 = (w["snapshot"][0] != RG.NO_MATCH) & ~acc[0] & ~acc[1] & acc[2]
    assert rej0.any() and np.all(w["winner"][rej0] == 2), "rejected at neighbour 0, accepted at neighbour 2"
    assert mp[0, 4] == mp[0, 5] and wp["snapshot"][0, 4] != RG.NO_MATCH, "an idx2 shared by two idx1"
    nanp = wp["info"][(0, 1)]
    assert np.isnan(nanp["cosRays"]) and nanp["status"] == RG.LOW_PARALLAX
    for name, sc, PP, mm, ww in (("main", s, P, m, w), ("planted", o, Pp, mp, wp)):
        delta, cm = conditions(PP, sc.k1, sc.k2, mm, ww)
        print(f"{name}: largest |x3D(fp64) - x3D(LAPACK float32)| = {delta:.3g} m; every gate holds at 8x that; nearest cosine decision {cm:.3g} from its boundary")
        assert cm > 1e-6


def test_refusals_that_need_no_device():
    L = capi.lib()
    cam = R.cam_struct()
    a = np.zeros(12, F); i2 = (C.c_int * 2)(); o = np.zeros(16, F)
    ok = lambda **kw: L.xfh_triangulate_pair(*[kw.get(k, v) for k, v in (("cam", C.byref(cam)), ("flags", 0), ("s", 1.0), ("rf", 1.8), ("sl", 1.0), ("far", 0.0),
                                              ("xy1", a.ctypes.data), ("raw1", None), ("ur1", -1.0), ("z1", -1.0), ("T1", a.ctypes.data), ("O1", a.ctypes.data),
                                              ("xy2", a.ctypes.data), ("raw2", None), ("ur2", -1.0), ("z2", -1.0), ("T2", a.ctypes.data), ("O2", a.ctypes.data),
                                              ("st", C.addressof(i2)), ("kd", C.addressof(i2) + 4), ("X", o.ctypes.data), ("n", o.ctypes.data + 16),
                                              ("d", o.ctypes.data + 32), ("xh", None))])
    assert ok() == 0 and ok(flags=capi.TRIANG_INERTIAL) == 0
    bad = [ok(cam=None), ok(flags=capi.TRIANG_CLAIM), ok(flags=4), ok(s=float("nan")), ok(rf=float("inf")), ok(sl=float("nan")), ok(far=float("inf"))]
    bad += [ok(**{k: None}) for k in ("xy1", "T1", "O1", "xy2", "T2", "O2", "st", "kd", "X", "n", "d")]
    assert all(rc == 1 for rc in bad), bad
    p = a.ctypes.data
    assert L.xfh_triangulate_device(None, 1, 1, 1, 1, 0, C.byref(cam), 1.0, 1.8, 1.0, 0.0, *([p] * 25)) == 1
    assert L.xfh_triangulate(None, 1, 1, 1, 0, C.byref(cam), 1.0, 1.8, 1.0, 0.0, *([p] * 25)) == 1
    assert L.xfh_kernel_name(capi.K["TRIANGULATE_PAIRS"]) == b"k_triangulate_pairs" and L.xfh_kernel_name(capi.K["TRIANGULATE_FINISH"]) == b"k_triangulate_finish"
    assert capi.K["TRIANGULATE_PAIRS"] == 36 and L.xfh_kernel_name(35) == b"k_pose_optimize"            # existing ids keep their values


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("triangulate") / "asan_triangulate_test")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "xfeatslam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "asan_triangulate_test.cpp"), "-o", exe])
    return exe


def test_rule_under_sanitizers_on_hostile_inputs(asan_exe):
    """a stand-alone program built from this repository's header alone with AddressSanitizer + UBSan: nothing of the library is linked, nothing
    runs on a GPU, nothing is loaded into Python"""
    r = subprocess.run([asan_exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "asan_triangulate_test ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


def test_rule_under_sanitizers_equals_the_python_rule(asan_exe, tmp_path, main, plant):
    s, P, d, m, w, _ = main
    o, mp, Pp, wp = plant
    rec = lambda ob: np.concatenate([[ob["x"], ob["y"], ob["xr"], ob["yr"], ob["ur"], ob["depth"]], ob["T"], ob["Ow"]]).astype(F).tobytes()
    sets = [(R.CAM, P, [(RG.obs(s.k1, i), RG.obs(s.k2[b], int(m[b][i])), r) for (b, i), r in w["info"].items()]),
            (R.CAM, Pp, [(RG.obs(o.k1, i), RG.obs(o.k2[b], int(mp[b][i])), r) for (b, i), r in wp["info"].items()])]
    for name, o1, o2, kw, _ in R.handmade():                                # good, NaN and hostile pairs alike
        Ph = RG.params(R.HCAM, **dict(dict(ratio_factor=R.RATIO_FACTOR, scale_last=R.SCALE_LAST), **kw))
        sets.append((R.HCAM, Ph, [(o1, o2, RG.pair_rule(Ph, o1, o2))]))
    for k, (cam, PP, pairs) in enumerate(sets):
        with open(tmp_path / "in.bin", "wb") as f:
            f.write(struct.pack("<i9fi", len(pairs), *[float(cam[c]) for c in ("fx", "fy", "cx", "cy", "bf")], float(PP["sigma2"]), float(PP["ratio_factor"]),
                                float(PP["scale_last"]), float(PP["far_th"]), int(PP["inertial"])))
            for o1, o2, _ in pairs:
                f.write(rec(o1) + rec(o2))
        r = subprocess.run([asan_exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
        want = b""
        for o1, o2, rr in pairs:
            nrm, dst = RG.normal_depth(rr["x3D"], o1["Ow"], o2["Ow"], PP["scale_last"]) if rr["status"] == RG.ACCEPTED else (np.zeros(3, F), np.zeros(3, F))
            want += struct.pack("<2i", int(rr["status"]), int(rr["kind"])) + rr["x3D"].astype(F).tobytes() + nrm.tobytes() + dst.tobytes() + rr["x3Dh"].astype(D).tobytes()
        assert open(tmp_path / "out.bin", "rb").read() == want, k
