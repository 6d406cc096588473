"""The two restatements of the keyframe database query (tests/ref_bowdb.py) against each other, on random databases and on every database of
tests/bowdb_rig.py (whose builders assert the condition each one is chosen for); xfh_bow_score -- the kernel's own source lines on the host --
against both by the bits of the double; hand-made cases with written-out answers; every class of refusal; the same lines under
AddressSanitizer.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bowdb_rig as R
import ref_bowdb as RB
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
bits = lambda x: np.float64(x).view(np.uint64)


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    if not os.path.exists(capi.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "xfeatslam_amd", "csrc"), "-s", "-j8"])


def _same(lit, rul, tag):
    """what the literal walk defines, against the rule: the sharing list in order, the word counts of the listed, the thresholds, the scored
    list with acc and pBestKF by bits, best_acc, the candidates"""
    k, m = rul["n_scored"], rul["n_candidates"]
    assert lit["listed"] == rul["listed"] and len(lit["listed"]) == rul["n_listed"], (tag, "listed")
    assert all(rul["common"][s] == w for s, w in lit["words"].items()), (tag, "words")
    assert (lit["max_common"], lit["min_common"]) == (rul["max_common"], rul["min_common"]), tag
    assert lit["list_slot"] == rul["list_slot"][:k].tolist() and lit["list_best"] == rul["list_best"][:k].tolist(), (tag, "list")
    assert np.array_equal(np.array(lit["list_acc"], F).view(np.uint32), rul["list_acc"][:k].view(np.uint32)), (tag, "acc")
    assert F(lit["best_acc"]).view(np.uint32) == F(rul["best_acc"]).view(np.uint32), (tag, "best_acc")
    assert lit["cand_slot"] == rul["cand_slot"][:m].tolist(), (tag, "candidates")
    assert np.array_equal(np.array(lit["cand_acc"], F).view(np.uint32), rul["cand_acc"][:m].view(np.uint32)), (tag, "cand_acc")
    assert np.all(rul["list_slot"][k:] == -1) and np.all(rul["list_best"][k:] == -1) and np.all(rul["cand_slot"][m:] == -1)
    assert set(np.nonzero(rul["status"] == RB.SCORED)[0].tolist()) == set(lit["list_slot"])


@pytest.mark.parametrize("name", R.NAMES)
def test_literal_and_rule_agree(name):
    c = R.case(name)                                                                           # (asserts the case's own conditions)
    for form in R.FORMS:
        s1, s2 = c["state0"].copy(), c["state0"].copy()
        for i, q in enumerate(c["queries"]):
            lit = RB.literal(c["db"], q["q"], form, s1, q["exclude"])
            rul = RB.rule(c["db"], q["q"], form, s2, q["exclude"])
            _same(lit, rul, (name, form, i))
            assert np.array_equal(s1.view(np.uint32), s2.view(np.uint32)), (name, form, i, "state")


def test_literal_and_rule_agree_on_more_random_databases():
    seen = 0
    for seed in range(40):
        c = R.random_db(5 + 3 * seed, 8 if seed % 2 else 40, 900 + seed, nn=seed % 12)
        for form in R.FORMS:
            s1, s2 = c["state0"].copy(), c["state0"].copy()
            for i, q in enumerate(c["queries"]):
                lit = RB.literal(c["db"], q["q"], form, s1, q["exclude"])
                rul = RB.rule(c["db"], q["q"], form, s2, q["exclude"])
                _same(lit, rul, (seed, form, i))
                seen += rul["n_candidates"] < rul["n_scored"]
    assert seen > 10                                                                           # the dedupe and the 0.75 test drop entries


def test_bow_score_by_bits():
    """xfh_bow_score against both restatements on every (query, slot) pair of the rig, and on the edge vectors"""
    pairs = 0
    for name in R.NAMES:
        c = R.case(name)
        for q in c["queries"]:
            for v in c["db"]["vecs"][:40]:
                if v is None:
                    continue
                s, nc, fc = Context.bow_score(q["q"][0], q["q"][1], v[0], v[1])
                ws, wn, wf = RB.rule_score(q["q"], v)
                assert bits(s) == bits(ws) == bits(RB.literal_score(q["q"], v)) and (nc, fc) == (wn, wf), (name, nc, wn)
                pairs += nc > 0
    assert pairs > 200
    a = R.mk({3: 0.25, 9: 0.5, 11: 0.25}); b = R.mk({4: 0.5, 10: 0.5}); e = (np.zeros(0, np.uint32), np.zeros(0))
    assert Context.bow_score(*a, *b) == (0.0, 0, capi.BOWDB_NO_WORD) and bits(Context.bow_score(*a, *b)[0]) == bits(-0.0)      # disjoint: -0.0
    assert Context.bow_score(*a, *a) == (1.0, 3, 3)                                            # identical, L1-normalised: 1
    for x, y in ((a, e), (e, a), (e, e)):
        s, nc, fc = Context.bow_score(*x, *y)
        assert bits(s) == bits(-0.0) and nc == 0 and fc == capi.BOWDB_NO_WORD
    lo = R.mk({0: 0.5, 7: 0.5}); hi = R.mk({0: 0.25, 0xFFFFFFFE: 0.75}); hi2 = R.mk({5: 0.5, 0xFFFFFFFE: 0.5})
    assert Context.bow_score(*lo, *hi) == (0.25, 1, 0) and Context.bow_score(*hi, *hi2) == (0.5, 1, 0xFFFFFFFE)
    # padding past n_words is not read: the transform's 0xFFFFFFFF / 0.0 entries behind the count change nothing
    L = capi.lib()
    pi, pv = np.array([3, 9, 0xFFFFFFFF, 0xFFFFFFFF], np.uint32), np.array([0.5, 0.5, 0.0, 0.0])
    qi, qv = np.array([9, 0xFFFFFFFF], np.uint32), np.array([1.0, 1.0])
    sc, nc, fc = C.c_double(), C.c_int(), C.c_uint32()
    assert L.xfh_bow_score(pi.ctypes.data, pv.ctypes.data, 2, qi.ctypes.data, qv.ctypes.data, 1, C.byref(sc), C.byref(nc), C.byref(fc)) == 0
    assert (sc.value, nc.value, fc.value) == (0.5, 1, 9)
    assert L.xfh_bow_score(pi.ctypes.data, pv.ctypes.data, 4, qi.ctypes.data, qv.ctypes.data, 2, C.byref(sc), C.byref(nc), C.byref(fc)) == 0 and nc.value == 2


def test_hand_made_answers():
    """written out by hand.  Query {1, 2, 3, 4, 5} at 0.25 (every value is dyadic, so every sum below is exact); for positive values score = sum of min(vi, wi) over the shared words"""
    q = R.mk({w: 0.25 for w in (1, 2, 3, 4, 5)})
    vecs = [R.mk({1: 0.5, 2: 0.125, 3: 0.125, 4: 0.125, 9: 0.125}),        # 0: 4 shared, first 1, score 0.25 + 3 * 0.125 = 0.625
            R.mk({2: 0.25, 3: 0.25, 4: 0.25, 5: 0.25}),                     # 1: 4 shared, first 2, score 1.0
            R.mk({5: 1.0}),                                                 # 2: 1 shared: listed, below min_common = 3
            R.mk({7: 1.0}),                                                 # 3: shares nothing
            None,                                                           # 4: empty
            R.mk({3: 0.0625, 4: 0.0625, 5: 0.0625, 6: 0.8125})]             # 5: 3 shared = min_common exactly: not scored
    db = R.make_db(vecs, {0: [2, 1, 3, 4], 1: [5, 0]}, nn=4)
    state = np.array([0, 0, 0.5, 9, 9, 0.25], F)                             # slot 2 and 5 carry a value from an earlier query
    r = RB.rule(db, q, RB.RELOC, state)
    assert r["common"].tolist() == [4, 4, 1, 0, 0, 3] and r["status"].tolist() == [RB.SCORED, RB.SCORED, RB.BELOW_MIN, RB.NOT_SHARING, RB.EMPTY, RB.BELOW_MIN]
    assert (r["n_listed"], r["max_common"], r["min_common"], r["n_scored"]) == (4, 4, 3, 2)
    assert r["score"].tolist()[:3] == [0.625, 1.0, 0.25] and bits(r["score"][3]) == bits(-0.0) and bits(r["score"][4]) == bits(-0.0)
    assert state.tolist() == [0.625, 1.0, 0.5, 9, 9, 0.25]
    # entry 0 = slot 0: 0.625 + 0.5 (slot 2, stale) + 1.0 (slot 1) = 2.125; slots 3 and 4 are not listed.  pBestKF = slot 1 (1.0 > 0.625; 0.5 is not)
    # entry 1 = slot 1: 1.0 + 0.25 (slot 5, stale) + 0.625 (slot 0) = 1.875; pBestKF stays slot 1
    a0, a1 = F(2.125), F(1.875)
    assert r["list_slot"].tolist()[:3] == [0, 1, -1] and r["list_best"].tolist()[:2] == [1, 1] and r["list_acc"].tolist()[:2] == [a0, a1]
    assert r["best_acc"] == a0 and r["n_candidates"] == 1 and r["cand_slot"].tolist()[:2] == [1, -1] and r["cand_acc"][0] == a0       # both name slot 1: the first wins
    r2 = RB.rule(db, q, RB.NBEST, np.array([0, 0, 0.5, 9, 9, 0.25], F), exclude=(1,))
    assert r2["status"][1] == RB.EXCLUDED and r2["n_scored"] == 1 and r2["cand_slot"][0] == 0 and r2["cand_acc"][0] == F(1.125)
    lit = RB.literal(db, q, RB.RELOC, np.array([0, 0, 0.5, 9, 9, 0.25], F))
    assert lit["listed"] == [0, 1, 5, 2] and lit["cand_slot"] == [1]
    assert [RB.min_common(k) for k in (1, 4, 5, 6, 10)] == [0, 3, 4, 4, 8]


def test_refusals_and_layout():
    L = capi.lib()
    p = np.zeros(64, np.uint8).ctypes.data
    sc, nc, fc = C.c_double(), C.c_int(), C.c_uint32()
    ok = (p, p, 2, p, p, 2, C.byref(sc), C.byref(nc), C.byref(fc))
    assert L.xfh_bow_score(*ok) == 0
    for i, v in ((2, -1), (5, -1), (0, None), (1, None), (3, None), (4, None), (6, None), (7, None), (8, None)):
        a = list(ok); a[i] = v
        assert L.xfh_bow_score(*a) == 1, (i, v)
    assert L.xfh_bow_score(None, None, 0, None, None, 0, C.byref(sc), C.byref(nc), C.byref(fc)) == 0                # a NULL array with a count of 0
    W = Context.bowdb_query_workspace_bytes
    assert W(0, 1) == 0 and W(-1, 1) == 0 and W(capi.BOWDB_MAX_SLOTS + 1, 1) == 0 and W(5, 0) == 0 and W(5, 65536) == 0
    assert W(300, 3) % 256 == 0 and W(300, 3) >= 3 * 300 * 4 and W(capi.BOWDB_MAX_SLOTS, 1) > 0
    # the device and host forms refuse before any HIP call (no ctx here); every other class needs a ctx: tests/test_gpu_bowdb.py
    assert L.xfh_bowdb_query_device(None, 1, 1, 0, p, p, p, 1, p, p, p, 1, None, None, 0, None, p, p, p, p, p, p, p, p, p, p, p, p) == 1
    assert L.xfh_bowdb_query(None, 1, 0, p, p, 1, p, p, p, 1, None, None, 0, None, p, p, p, p, p, p, p, p, p, p, p) == 1
    assert (capi.BOWDB_MAX_SLOTS, capi.BOWDB_MAX_NEIGHBOURS, capi.BOWDB_HEADER_INTS, capi.BOWDB_FORM_RELOC, capi.BOWDB_FORM_NBEST) == (8192, 16, 8, 0, 1)
    assert (capi.BOWDB_EMPTY, capi.BOWDB_NOT_SHARING, capi.BOWDB_EXCLUDED, capi.BOWDB_BELOW_MIN, capi.BOWDB_SCORED) == (RB.EMPTY, RB.NOT_SHARING, RB.EXCLUDED, RB.BELOW_MIN, RB.SCORED)
    hdr = open(os.path.join(ROOT, "include", "xfeat_hip.h")).read()
    for k, v in (("MAX_SLOTS", 8192), ("MAX_NEIGHBOURS", 16), ("HEADER_INTS", 8), ("FORM_RELOC", 0), ("FORM_NBEST", 1), ("EMPTY", 0), ("NOT_SHARING", 1), ("EXCLUDED", 2),
                 ("BELOW_MIN", 3), ("SCORED", 4)):
        assert f"#define XFH_BOWDB_{k} {v}" in hdr, k
    assert L.xfh_kernel_name(capi.K["BOWDB_SCORE"]) == b"k_bowdb_score" and L.xfh_kernel_name(capi.K["BOWDB_SELECT"]) == b"k_bowdb_select"
    assert (capi.K["BOWDB_SCORE"], capi.K["BOWDB_SELECT"]) == (33, 34) and L.xfh_kernel_name(32) == b"k_vocab_finish"    # existing ids keep their values
    lay = Context.bowdb_query_layout(3, 300, 256)
    offs = sorted(v for k, v in lay.items() if k != "bytes")
    assert all(o % 256 == 0 for o in offs) and offs[0] == 256 and len(set(offs)) == 10 and lay["bytes"] > offs[-1]


def test_score_header_under_sanitizers(tmp_path):
    """bowdb_math.h -- the lines k_bowdb_score and k_bowdb_select run per lane -- over well-formed and hostile vectors (n_words beyond the stride,
    descending ids) in heap buffers of exactly their size, xfh_bow_score and the argument checks, in a stand-alone program built with
    AddressSanitizer + UBSan against the sanitizer build of the HOST code (make -C xfeatslam_amd/csrc asan; device code is not instrumented
    and nothing here runs on a GPU)"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "xfeatslam_amd", "csrc"), "asan", "-s", "-j8"])
    exe = str(tmp_path / "asan_bowdb_test")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "xfeatslam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "asan_bowdb_test.cpp"),
                           "-L" + os.path.join(ROOT, "xfeatslam_amd"), "-lxfeat_hip_asan", "-Wl,-rpath," + os.path.join(ROOT, "xfeatslam_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "asan_bowdb_test: ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
