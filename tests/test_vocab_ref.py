"""CPU tests of the vocabulary transform: the two forms of the restatement (tests/ref_vocab.py) against each other on every feature set of
every vocabulary of tests/vocab_rig.py, xfh_vocab_descend (vocab_math.h, the kernel's own lines) against them on every feature, the
xfh_vocab_pack / xfh_vocab_unpack round trip, every class of refusal of xfh_vocab_pack, and vocab_math.h over good, truncated and hostile
blobs under AddressSanitizer + UBSan in a stand-alone program (tests/cpp/asan_vocab_test.cpp).  Every comparison is equality of integers or
of the bits of doubles.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import ref_vocab as RV
import vocab_rig as VR
from conftest import ROOT
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context

bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("name", VR.NAMES)
def test_two_forms_and_host_descent(name):
    voc = VR.vocabulary(name)
    blob = VR.blob(name)
    for kind, n in VR.cases(name):
        rows = VR.features(name, kind, n)
        for lu in VR.levelsups(voc["L"]):
            lit = RV.literal(voc, rows, lu)
            vec = VR.want(name, kind, n, lu)
            tag = (name, kind, n, lu)
            for k in ("word", "node_of", "bow_ids"):
                assert np.array_equal(lit[k], vec[k]), (tag, k)
            assert np.array_equal(bits(lit["weight"]), bits(vec["weight"])) and np.array_equal(bits(lit["bow_vals"]), bits(vec["bow_vals"])), tag
            assert lit["n_words"] == vec["n_words"] and lit["fv"] == RV.feature_vector(vec["node_of"]), tag
            # the node blob of node_of is the feature vector
            ids, ns, items = Context.nodes_unpack(Context.nodes_pack(vec["node_of"])[:Context.nodes_bytes(n)], n)
            assert ids.tolist() == list(lit["fv"]) and all(items[ns[j]:ns[j + 1]].tolist() == f for j, f in enumerate(lit["fv"].values())), tag
            word, node, wt = Context.vocab_descend(blob, rows, lu)
            go = wt > 0
            assert np.array_equal(word, vec["word"]) and np.array_equal(bits(wt), bits(vec["weight"])), tag
            assert np.array_equal(node[go], vec["node_of"][go]) and np.all(vec["node_of"][~go] == RV.NONE), tag
        if kind == "stopped":
            assert vec["n_words"] == 0 and np.all(vec["node_of"] == RV.NONE)
        if kind == "oneword":
            w = float(vec["weight"][0])
            assert vec["n_words"] == 1 and vec["bow_vals"][0] == 1.0 and len(set(vec["word"].tolist())) == 1 and n == 4096
            acc = 0.0
            for _ in range(n):
                acc += w
            assert acc != n * w                                        # the iterated sum is not count * w
        if kind == "mixed" and n >= 257:
            assert 3 < vec["n_words"] < n and (vec["bow_vals"] > 0).all() and abs(vec["bow_vals"].sum() - 1.0) < 1e-9
            assert not rows.view(np.uint32)[::8, :8].any() and np.isnan(rows[:, :8]).any() and np.isinf(rows[:, :8]).any()


def test_node_levels_and_the_special_leaves():
    """where the node id comes from: level L - levelsup of the path, the root at and above L, the leaf where the path is shorter; and the
    planted leaves of the irregular vocabulary"""
    voc = VR.vocabulary("irregular")
    sp, L = voc["special"], voc["L"]
    blob = VR.blob("irregular")
    row = lambda first: VR._rows(np.random.RandomState(1), np.asarray(first, np.uint8)[None])
    anc = lambda k: VR._ancestors(voc["parent"], sp[k])
    for key in ("leaf1", "wide_late", "chain_end", "dup_first", "tie_first"):
        r = row(sp["planted"] if key == "tie_first" else voc["desc"][sp[key]])
        path = anc(key)
        for lu in range(0, L + 3):
            word, node, wt = Context.vocab_descend(blob, r, lu)
            lvl = L - lu
            want = 0 if lvl <= 0 else (path[lvl] if lvl < len(path) else sp[key])
            assert (int(word[0]), int(node[0])) == (int(voc["word_id"][sp[key]]), want), (key, lu)
            assert int(RV.literal(voc, r, lu)["node_of"][0]) == want
    word, node, wt = Context.vocab_descend(blob, row(voc["desc"][sp["dup_second"]]), 0)
    assert int(word[0]) == int(voc["word_id"][sp["dup_first"]])                            # of two identical siblings the first wins
    for key in ("w_zero", "w_neg", "w_nan", "phantom"):
        r = row(voc["desc"][sp[key]])
        word, node, wt = Context.vocab_descend(blob, r, 1)
        assert int(word[0]) == int(voc["word_id"][sp[key]]) and not wt[0] > 0 and bits(wt)[0] == bits(voc["weight"][sp[key]:sp[key] + 1])[0]
        lit = RV.literal(voc, r, 1)
        assert lit["n_words"] == 0 and lit["node_of"][0] == RV.NONE
    assert int(Context.vocab_descend(blob, np.zeros((1, 64), np.float32), 1)[0][0]) == 0   # a zero row lands on the phantom: word 0, stopped


@pytest.mark.parametrize("name", VR.NAMES)
def test_pack_unpack_round_trip(name):
    voc = VR.vocabulary(name)
    n = len(voc["parent"])
    blob, mc, dp = Context.vocab_pack(voc["parent"], voc["word_id"], voc["weight"], voc["desc"], voc["L"])
    nb = Context.vocab_bytes(n)
    assert nb % 32 == 0 and len(blob) == nb and np.array_equal(blob, VR.blob(name))        # two packs: identical bytes
    counts = np.bincount(voc["parent"][1:], minlength=n)
    assert mc == counts.max() and dp == {"bfs": 3, "dfs": 3, "irregular": 10}[name]
    u = Context.vocab_unpack(blob, n)
    assert (u["L"], u["max_children"], u["depth"]) == (voc["L"], mc, dp)
    assert np.array_equal(u["parent"], voc["parent"]) and np.array_equal(u["word_id"], voc["word_id"])
    assert np.array_equal(bits(u["weight"][1:]), bits(voc["weight"][1:])) and np.array_equal(u["desc"][1:], voc["desc"][1:]) and not u["desc"][0].any()
    # the layout the header documents: the children of a slot are consecutive slots, their rows one contiguous 32-byte aligned run
    w = blob[64:64 + 16 * n].view(np.uint32).reshape(n, 4)
    rows = blob[nb - 32 * n:].reshape(n, 32)
    ch = RV.children(voc)
    slot_of = np.zeros(n, np.int64); slot_of[w[:, 2]] = np.arange(n)
    assert sorted(w[:, 2].tolist()) == list(range(n)) and (nb - 32 * n) % 32 == 0 and w[0, 2] == 0
    for node in range(n):
        first, nch = w[slot_of[node], :2]
        assert nch == len(ch[node]) and w[first:first + nch, 2].tolist() == ch[node] if nch else first == 0
        assert node == 0 or np.array_equal(rows[slot_of[node]], voc["desc"][node])
    # truncated and damaged blobs are refused, never read past
    with pytest.raises(capi.XfhError):
        Context.vocab_unpack(blob[:nb - 1], n)
    for off, val in ((0, 0), (4, n - 1), (8, 0), (8, 11), (64, 2), (64 + 4, 0), (64 + 16 + 8, 0), (64 + 16 * (n - 1), 1)):
        bad = blob.copy(); bad[off:off + 4].view(np.uint32)[0] = val
        with pytest.raises(capi.XfhError):
            Context.vocab_unpack(bad, n)


def test_pack_refuses_every_class():
    L = capi.lib()
    voc = VR.vocabulary("bfs")
    n = len(voc["parent"])
    out = np.zeros(Context.vocab_bytes(n), np.uint8)
    arr = dict(parent=voc["parent"].copy(), word=voc["word_id"], weight=voc["weight"], desc=voc["desc"])

    def pack(nn=n, Lv=3, **kw):
        a = dict(arr); a.update(kw)
        p = lambda x: None if x is None else x.ctypes.data
        return L.xfh_vocab_pack(nn, Lv, p(a["parent"]), p(a["word"]), p(a["weight"]), p(a["desc"]), None if kw.get("blob", 1) is None else out.ctypes.data, None, None)

    assert pack() == 0
    assert [pack(nn=k) for k in (1, 0, -1)] == [1, 1, 1] and pack(nn=2) == 0               # n_nodes < 2
    assert [pack(Lv=k) for k in (0, -1, 11, 1 << 20)] == [1, 1, 1, 1] and pack(Lv=1) == 0 and pack(Lv=10) == 0   # L outside 1 .. 10
    for i, v in ((1, 1), (7, 7), (7, 8), (n - 1, n - 1), (500, 0xFFFFFFFF), (1, 5)):       # parent[i] >= i (with i = 1: the root is left without children)
        bad = voc["parent"].copy(); bad[i] = v
        assert pack(parent=bad) == 1, (i, v)
    flat = np.zeros(n, np.uint32)                                                          # every node under the root
    assert pack(nn=34, parent=flat) == 1 and pack(nn=33, parent=flat) == 0                 # 33 children resp. XFH_VOCAB_MAX_CHILDREN
    chain = np.maximum(np.arange(n, dtype=np.int64) - 1, 0).astype(np.uint32)
    assert pack(nn=34, parent=chain) == 1 and pack(nn=33, parent=chain) == 0               # depth 33 resp. XFH_VOCAB_MAX_DEPTH
    for k in ("parent", "word", "weight", "desc"):
        assert pack(**{k: None}) == 1, k
    assert pack(blob=None) == 1
    assert (capi.VOCAB_MAX_CHILDREN, capi.VOCAB_MAX_DEPTH, capi.BOWT_TF_IDF_L1) == (32, 32, 0)
    assert Context.vocab_bytes(0) == 0 and Context.vocab_bytes(-3) == 0 and Context.vocab_bytes(2) > 64 + 2 * 56 - 1
    # the entry points that need no GPU refuse before any HIP call; the kernels have names
    W = Context.bow_transform_workspace_bytes
    assert W(0, 1) == 0 and W(5, 0) == 0 and W(capi.GRID_MAX_N + 1, 1) == 0 and W(5, 65536) == 0 and W(257, 3) % 256 == 0 and W(257, 3) >= 3 * 257 * 8
    p = np.zeros(64, np.uint8).ctypes.data
    assert L.xfh_bow_transform_device(None, 1, 1, 4, 0, p, 4096, p, 0, p, p, p, p, p, p, p, p) == 1
    assert L.xfh_bow_transform(None, 1, 4, 0, p, 4096, p, p, p, p, p, p, p, p) == 1
    assert L.xfh_vocab_descend(p, 64, -1, p, p, p, p) == 1 and L.xfh_vocab_descend(p, 63, 4, p, p, p, p) == 1 and L.xfh_vocab_descend(None, 64, 4, p, p, p, p) == 1
    assert L.xfh_kernel_name(capi.K["VOCAB_DESCEND"]) == b"k_vocab_descend" and L.xfh_kernel_name(capi.K["VOCAB_FINISH"]) == b"k_vocab_finish"
    assert (capi.K["VOCAB_DESCEND"], capi.K["VOCAB_FINISH"]) == (31, 32) and L.xfh_kernel_name(29) == b"k_init_final"    # existing ids keep their values


def test_descent_header_under_sanitizers(tmp_path):
    """vocab_math.h -- the lines k_vocab_descend goes down a blob through -- over well-formed, truncated and hostile blobs in heap buffers of
    exactly their byte count, xfh_vocab_pack / _unpack and the argument checks, in a stand-alone program built with AddressSanitizer + UBSan
    against the sanitizer build of the HOST code (make -C xfeatslam_amd/csrc asan; device code is not instrumented and nothing here runs on
    a GPU)"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "xfeatslam_amd", "csrc"), "asan", "-s", "-j8"])
    exe = str(tmp_path / "asan_vocab_test")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "xfeatslam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "asan_vocab_test.cpp"),
                           "-L" + os.path.join(ROOT, "xfeatslam_amd"), "-lxfeat_hip_asan", "-Wl,-rpath," + os.path.join(ROOT, "xfeatslam_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "asan_vocab_test ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
