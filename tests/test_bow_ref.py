"""CPU side of SearchByBoW: the literal transcription of the reference's loop and the per-node form of the contract (tests/ref_bow.py)
agree -- the equivalence the device design rests on --, the scene of tests/bow_rig.py holds every case the GPU tests are meant to meet
(asserted here, where the seeds are chosen), xfh_bow_accept agrees with the restatement on every boundary, and the blob-clamping header
and xfh_bow_accept run under AddressSanitizer + UBSan in a stand-alone program.  The searches themselves need a GPU: tests/test_gpu_bow.py."""
import os
import subprocess

import numpy as np
import pytest

import bow_rig as BR
import ref_bow as RB
from conftest import ROOT
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context

F = np.float32
RATIOS = (0.6, 0.9, 1.5)


@pytest.fixture(scope="module")
def scene():
    return BR.Scene()


def agree(dist, no1, a1, no2, e2, flags, **kw):
    lit = RB.literal(dist, no1, a1, no2, e2, flags, **kw)
    for order in (None, 1, 2):
        m = RB.per_node(dist, no1, a1, no2, e2, flags, order=order, **kw)
        for key, val in lit.items():
            assert np.array_equal(val, m[key]), (key, flags, order, kw)
    assert np.all((m["status"] == RB.MATCHED) == (m["match12"] >= 0)) and m["n_matches"] == int((m["match12"] >= 0).sum()) == int((m["assigned2"] >= 0).sum())
    hit = np.nonzero(m["match12"] >= 0)[0]
    assert np.array_equal(m["assigned2"][m["match12"][hit]], hit)                            # a target is claimed once
    return m


def test_hand_made_cases_both_forms():
    cases = RB.handmade()
    assert len(cases) == 9
    for name, dist, no1, a1, no2, e2, flags, ratio, want in cases:
        m = agree(dist, no1, a1, no2, e2, flags, nn_ratio=ratio)
        for key, val in want.items():
            assert m[key].tolist() == val, (name, key, m[key].tolist(), val)
        assert m["n_matches"] == want["status"].count(RB.MATCHED), name


def test_the_two_forms_agree_on_the_scene(oracle_mod, scene):
    s = scene
    for p, b in ((0, 0), (0, 1), (0, 2), (1, 0), (2, 0), (1, 1), (2, 2)):
        for keyframe in (False, True):
            for ratio in RATIOS:
                s1, s2 = s.blocks[p], s.s2[b]
                agree(s.dist(oracle_mod, p, b), s1["node_of"], s1["active"], s2["node_of"], s2["has"] if keyframe else None, RB.STRICT_LOW if keyframe else 0, nn_ratio=ratio)
    agree(s.dist(oracle_mod, 0, 0), s.s1["node_of"], s.s1["active"], s.s2[0]["node_of"], None, 0, nn_ratio=0.75, th_low=40, init_dist=120)
    agree(s.dist(oracle_mod, 0, 0), s.s1["node_of"], s.s1["active"], s.s2[0]["node_of"], s.s2[0]["has"], 1, nn_ratio=1.5, th_low=300, init_dist=0x7fffffff)


def test_scene_holds_every_case(oracle_mod, scene):
    """the conditions the GPU tests rely on, so that they cannot pass vacuously"""
    s = scene
    assert (len(s.s1["node_of"]), len(s.s2[0]["node_of"])) == (BR.N1, BR.N2) == (390, 515)
    fv1, fv2 = RB.feature_vector(s.s1["node_of"]), RB.feature_vector(s.s2[0]["node_of"])
    sz1, sz2 = {len(v) for v in fv1.values()}, {len(v) for v in fv2.values()}
    assert {1, 64, 65} <= sz1 and max(sz1) >= 130 and {1, 63, 64, 65, 150} <= sz2
    assert set(fv1) - set(fv2) and set(fv2) - set(fv1) and {0, 1, 0xFFFFFFFE} <= set(fv1) & set(fv2) and any((1 << 31) < k < 0xFFFFFFFE for k in fv1)
    assert (s.s1["node_of"] == RB.NONE).sum() >= 8 and (s.s2[0]["node_of"] == RB.NONE).sum() >= 8
    for keyframe in (False, True):
        st = {r: RB.new_stats() for r in RATIOS}
        m = {r: s.want(oracle_mod, 0, 0, keyframe, nn_ratio=r, stats=st[r]) for r in RATIOS}
        free = {r: s.want(oracle_mod, 0, 0, keyframe, nn_ratio=r, claims=False) for r in RATIOS}
        a, f, t = m[0.6], free[0.6], st[0.6]
        counts = np.bincount(a["status"], minlength=5)
        moved = np.nonzero((a["match12"] != f["match12"]) | (a["best_dist"] != f["best_dist"]) | (a["second_dist"] != f["second_dist"]))[0]
        ratio_passes = int(((f["status"] == RB.REJECTED) & (a["status"] == RB.MATCHED) & (a["best_dist"] == f["best_dist"])).sum())
        ratio_fails = int(((f["status"] == RB.MATCHED) & (a["status"] == RB.REJECTED)).sum())
        print(f"keyframe form {keyframe}: statuses {counts.tolist()}, moved by a claim {len(moved)}, chain depth {int(t['depth'].max())}, accepted after a claim {ratio_passes}, "
              f"rejected after a claim {ratio_fails}, single {t['single']}, none eligible {t['none_eligible']}, none after claims {t['none_after_claims']}, "
              f"lists run out {[st[r]['runs_out'] for r in RATIOS]}, matches {[m[r]['n_matches'] for r in RATIOS]}")
        assert np.all(counts >= 2), counts                                                   # every status occurs
        assert len(moved) >= 8 and t["depth"].max() >= 3                                     # an earlier query took their nearest; a chain of depth >= 3
        assert ratio_passes >= 1 and ratio_fails >= 1
        assert t["single"] >= 1 and t["none_after_claims"] >= 1 and (t["none_eligible"] >= 1) == keyframe
        # the pile-up: with every candidate accepted the i-th query of the spot finds about i claimed entries ahead, and the lists run out
        pile = st[1.5]["ahead"][np.nonzero(s.s1["node_of"] == BR.TR.BIG)[0]]
        assert (pile >= RB.K_LIST).sum() >= 30 and pile.max() >= 30 and st[1.5]["runs_out"] >= 30
        assert len({m[r]["n_matches"] for r in RATIOS}) == 3
        # duplicates: rejected while nn_ratio <= 1 (best == second), the FIRST member wins at 1.5
        dup = np.nonzero((a["best_dist"] == a["second_dist"]) & (a["best_dist"] < RB.TH_LOW) & (a["status"] == RB.REJECTED))[0]
        assert len(dup) >= 3 and np.all(m[0.9]["status"][dup] == RB.REJECTED) and st[1.5]["tie_first_wins"] >= 3
        # a query whose best distance IS the th_low passed: matched in the frame form, rejected under XFH_BOW_STRICT_LOW
        th = s.th_low(oracle_mod)
        lo = s.want(oracle_mod, 0, 0, False, th_low=th); hi = s.want(oracle_mod, 0, 0, True, th_low=th)
        on = np.nonzero((lo["status"] == RB.MATCHED) & (lo["best_dist"] == th))[0]
        assert len(on) >= 1 and np.any((hi["best_dist"][on] == th) & (hi["status"][on] == RB.REJECTED))
    nm = [[s.want(oracle_mod, p, b)["n_matches"] for p, b in pairs] for pairs in (((0, 0), (0, 1), (0, 2)), ((0, 0), (1, 0), (2, 0)), ((0, 0), (1, 1), (2, 2)))]
    assert all(len(set(x)) == 3 and min(x) >= 8 for x in nm), nm                            # the three problems of every batch differ


def test_bow_accept_boundaries():
    L = capi.lib()
    n = 0
    both = lambda bi, b, sec, th, r, fl: (Context.bow_accept(bi, b, sec, th, r, fl), RB.accept(bi, b, sec, th, r, fl))
    for fl in (0, 1):
        for th in (0, 1, 100, 256, 1000):
            for b in (th - 1, th, th + 1):
                if b < 0:
                    continue
                for sec in (b, b + 1, 2 * b + 1, 256, 0x7fffffff):
                    for bi in (-1, 0, 5):
                        g, w = both(bi, b, sec, th, 0.6, fl)
                        assert g == w, (bi, b, sec, th, fl); n += 1
                        assert g == (bi >= 0 and (b < th if fl else b <= th) and b < np.float32(0.6) * np.float32(sec)), (bi, b, sec, th, fl)
        assert both(0, 100, 256, 100, 0.6, fl) == ((not fl),) * 2 and both(0, 99, 256, 100, 0.6, fl) == (True, True) and both(-1, 0, 256, 100, 0.6, fl) == (False, False)
    # (float)best exactly equal to, one ulp below and one ulp above nn_ratio * (float)second
    for r in (0.6, 0.7, 0.75, 0.9, 1.5):
        hits = 0
        for sec in list(range(1, 700)) + [256, 1 << 20, (1 << 24) + 1, 0x7fffffff]:
            prod = F(F(r) * F(sec))
            for b in {int(np.floor(float(prod))) + k for k in (-1, 0, 1, 2)}:
                if b < 0 or b > 0x7fffffff:
                    continue
                g, w = both(0, b, sec, 0x7fffffff, r, 0)
                assert g == w == bool(F(b) < prod), (r, b, sec); n += 1
                hits += int(F(b) == prod)
        assert hits >= 1, r                                                                  # the equality case occurred
        # the product itself one ulp apart: a ratio whose product with `second` lands on each side of an integer best
        for sec, b in ((10, 6), (100, 60), (256, 153), (40, 30), (200, 150), (1000, 900), (64, 96)):
            for rr in (np.nextafter(F(b) / F(sec), F(0)), F(b) / F(sec), np.nextafter(F(b) / F(sec), F(9))):
                g, w = both(0, b, sec, 0x7fffffff, float(rr), 0)
                assert g == w, (rr, b, sec); n += 1
    rng = np.random.RandomState(11)
    for _ in range(4000):
        bi = int(rng.randint(-1, 3)); b = int(rng.randint(0, 300)); sec = int(rng.choice([b, b + int(rng.randint(0, 300)), 256])); th = int(rng.randint(0, 300))
        r = float(rng.choice([0.6, 0.7, 0.75, 0.9, 1.5, rng.rand() * 2])); fl = int(rng.randint(0, 2))
        g, w = both(bi, b, sec, th, r, fl)
        assert g == w, (bi, b, sec, th, r, fl); n += 1
    assert n > 6000
    assert L.xfh_kernel_name(capi.K["BOW_CANDIDATES"]) == b"k_bow_candidates" and L.xfh_kernel_name(capi.K["BOW_RESOLVE"]) == b"k_bow_resolve"
    assert (capi.K["BOW_CANDIDATES"], capi.K["BOW_RESOLVE"]) == (21, 22) and L.xfh_kernel_name(20) == b"k_triangulation_search"
    # the workspace size: 0 for sizes the call refuses, a multiple of 256 that grows with B and n1 otherwise
    W = Context.bow_search_workspace_bytes
    assert W(0, 5, 1) == 0 and W(5, 0, 1) == 0 and W(5, 5, 0) == 0 and W(capi.GRID_MAX_N + 1, 5, 1) == 0 and W(5, 5, 65536) == 0
    assert W(390, 515, 1) % 256 == 0 and W(390, 515, 3) > 2 * W(390, 515, 1) > 0 and W(391, 515, 1) >= W(390, 515, 1) >= 390 * 11 * 4
    p = np.zeros(64, np.uint8).ctypes.data
    assert L.xfh_bow_search_device(None, 1, 1, 1, 0, 0, 256, 100, 0.6, p, p, p, 0, p, None, p, 0, p, p, p, p, p, p, p, p) == 1
    assert L.xfh_bow_search(None, 1, 1, 0, 256, 100, 0.6, p, p, p, p, None, p, p, p, p, p, p, p, p) == 1


def test_clamping_header_and_accept_under_sanitizers(tmp_path):
    """nodes_clamp.h -- the lines the kernels read blobs through -- over well-formed and hostile blobs in heap buffers of exactly
    xfh_nodes_bytes(n) bytes, and xfh_bow_accept, in a stand-alone program built with AddressSanitizer + UBSan against the sanitizer build
    of the HOST code (make -C xfeatslam_amd/csrc asan; device code is not instrumented and nothing here runs on a GPU)"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "xfeatslam_amd", "csrc"), "asan", "-s", "-j8"])
    exe = str(tmp_path / "asan_bow_test")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "xfeatslam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "asan_bow_test.cpp"),
                           "-L" + os.path.join(ROOT, "xfeatslam_amd"), "-lxfeat_hip_asan", "-Wl,-rpath," + os.path.join(ROOT, "xfeatslam_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "asan_bow_test ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
