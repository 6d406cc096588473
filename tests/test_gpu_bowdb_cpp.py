"""The C++ layer of the keyframe database: ORB_SLAM3::XFkeyframeDatabase (include/xfeat/ORBmatcher_xfeat.h), compiled with g++ like the other
drop-in classes, on databases of tests/bowdb_rig.py: add() in insertion order, the queries of the case in both forms on the database's own two
persistent score arrays, and the two candidate functions with a map per slot.  Every dumped output equals the rule's answer
(tests/ref_bowdb.py) by integers and bits."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bowdb_rig as R
import ref_bowdb as RB
from conftest import ROOT

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def exe(gpu_lib, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("bowdb") / "bowdb_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "bowdb_test.cpp"),
                           "-L" + os.path.join(ROOT, "xfeatslam_amd"), "-lxfeat_hip", "-Wl,-rpath," + os.path.join(ROOT, "xfeatslam_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", path])
    return path


def _bow(v):
    return struct.pack("<i", len(v[0])) + np.ascontiguousarray(v[0], np.uint32).tobytes() + np.ascontiguousarray(v[1], np.float64).tobytes()


@pytest.mark.parametrize("name", ("samebest", "exclusion", "stale", "random_63_8"))
def test_cpp_keyframe_database(tmp_path, exe, name):
    c = R.case(name)
    db = c["db"]
    n, nn = len(db["vecs"]), db["neigh"].shape[1]
    seq = np.arange(n) if db["seq"] is None else db["seq"]
    order = sorted((s for s in range(n) if db["vecs"][s] is not None), key=lambda s: (int(seq[s]), s))          # `add` in insertion order
    queries = [(form, q) for form in R.FORMS for q in c["queries"]]
    stride = max([c["stride"]] + [len(q["q"][0]) for _, q in queries])                        # the class has one stride for the slots and the query
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<5i", n, stride, nn, len(order), len(queries)))
        for s in order:
            f.write(struct.pack("<i", s) + _bow(db["vecs"][s]) + np.ascontiguousarray(db["neigh"][s], np.int32).tobytes())
        for form, q in queries:
            f.write(struct.pack("<i", form) + _bow(q["q"]) + struct.pack("<i", len(q["exclude"])) + np.array(q["exclude"], np.int32).tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = np.fromfile(tmp_path / "out.bin", np.uint8)
    want = []
    state = {form: np.zeros(n, F) for form in R.FORMS}                                         # the database's own arrays start at zero
    for form, q in queries:
        w = RB.rule(db, q["q"], form, state[form], q["exclude"])
        want += [np.array([w[k] for k in ("n_listed", "max_common", "min_common", "n_scored", "n_candidates")], np.int32), np.array([w["best_acc"]], F),
                 w["common"], w["score"], w["status"], w["list_slot"], w["list_acc"], w["list_best"], w["cand_slot"], w["cand_acc"]]
    # the candidate functions on the last query (NBEST state after the chain; RELOC state likewise): map of slot s = s % 2, the query's map 0
    form, q = queries[-1]
    rel = RB.rule(db, q["q"], RB.RELOC, state[RB.RELOC])
    want.append(np.array([len(x) for x in [[s for s in R.cands(rel) if s % 2 == 0]]] + [s for s in R.cands(rel) if s % 2 == 0], np.int32))
    nb = RB.rule(db, q["q"], RB.NBEST, state[RB.NBEST])
    loop, merge = [], []
    for s in R.cands(nb):
        if not (len(loop) < 2 or len(merge) < 2):
            break
        if s % 2 == 0 and len(loop) < 2:
            loop.append(s)
        elif s % 2 == 1 and len(merge) < 2:
            merge.append(s)
    want += [np.array([len(loop)] + loop, np.int32), np.array([len(merge)] + merge, np.int32)]
    wraw = np.concatenate([np.ascontiguousarray(a).view(np.uint8).ravel() for a in want])
    assert len(raw) == len(wraw) and np.array_equal(raw, wraw), (len(raw), len(wraw), np.nonzero(raw[:min(len(raw), len(wraw))] != wraw[:min(len(raw), len(wraw))])[0][:8])
    print(f"{name}: {len(queries)} queries, last NBEST {R.cands(nb)} -> loop {loop}, merge {merge}")
