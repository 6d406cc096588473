"""The C++ layer of the vocabulary transform: ORB_SLAM3::XFvocabulary (include/xfeat/ORBmatcher_xfeat.h), the Mat overload and the form on
rows that sit in a record in device memory, compiled with g++ like the other drop-in classes: both produce the dump of the C ABI
(xfh_vocab_pack + xfh_bow_transform), and that dump is the restatement's answer (tests/ref_vocab.py): n_words, node_of, the BowVector bit
for bit and the node blob byte for byte."""
import os
import struct
import subprocess

import numpy as np
import pytest

import vocab_rig as VR
from conftest import ROOT
from xfeatslam_amd.extractor import Context

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(gpu_lib, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("vocab") / "vocab_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "vocab_test.cpp"),
                           "-L" + os.path.join(ROOT, "xfeatslam_amd"), "-lxfeat_hip", "-Wl,-rpath," + os.path.join(ROOT, "xfeatslam_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", path])
    return path


@pytest.mark.parametrize("name,kind,n,lu", [("irregular", "mixed", 257, 1), ("dfs", "mixed", 4096, 4), ("irregular", "stopped", 257, 2)])
def test_cpp_vocabulary(tmp_path, exe, name, kind, n, lu):
    voc = VR.vocabulary(name)
    rows = VR.features(name, kind, n)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<4i", len(voc["parent"]), voc["L"], n, lu))
        for a in (voc["parent"].astype(np.uint32), voc["word_id"].astype(np.uint32), voc["weight"].astype(np.float64), voc["desc"].astype(np.uint8), rows.astype(np.float32)):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = np.fromfile(tmp_path / "out.bin", np.uint8)
    w = VR.want(name, kind, n, lu)
    nw, nb = w["n_words"], Context.nodes_bytes(n)
    ids = np.full(n, 0xFFFFFFFF, np.uint32); ids[:nw] = w["bow_ids"]
    vals = np.zeros(n, np.float64); vals[:nw] = w["bow_vals"]
    want = np.concatenate([np.array([nw], np.int32).view(np.uint8), w["node_of"].view(np.uint8), ids.view(np.uint8), vals.view(np.uint8),
                           Context.nodes_pack(w["node_of"])[:nb]])
    assert len(raw) == 3 * len(want), (len(raw), len(want))
    for j, form in enumerate(("C ABI", "Mat", "device rows")):
        got = raw[j * len(want):(j + 1) * len(want)]
        assert np.array_equal(got, want), (form, np.nonzero(got != want)[0][:8])
    print(f"{name} {kind} n {n} levelsup {lu}: {nw} words, {int((w['node_of'] != 0xFFFFFFFF).sum())} features in nodes")
