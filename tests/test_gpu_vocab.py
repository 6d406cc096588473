"""xfh_bow_transform_device (k_vocab_descend, k_vocab_finish) against the restatement tests/ref_vocab.py on the vocabularies and feature sets of
tests/vocab_rig.py.  Every comparison is equality of integers or of the bits of doubles: word, node_of, weight, n_words, bow_ids, bow_vals, and
the node blob against the bytes of Context.nodes_pack(node_of).  The conditions the vocabularies and sets are chosen for are asserted where
the seeds are chosen, on the CPU (tests/vocab_rig.py, tests/test_vocab_ref.py)."""
import numpy as np
import pytest

import bow_rig as BR
import ref_vocab as RV
import vocab_rig as VR
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context, ORBmatcher

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def rig(gpu_lib):
    r = VR.VocabRig(gpu_lib)
    yield r
    r.close()


@pytest.mark.parametrize("name", VR.NAMES)
def test_every_set_and_levelsup(rig, name):
    voc = VR.vocabulary(name)
    for kind, n in VR.cases(name):
        rows = VR.features(name, kind, n)
        for lu in VR.levelsups(voc["L"]):
            res, raw, out, _ = rig.run(name, [rows], lu)
            out.free()
            w = VR.want(name, kind, n, lu)
            VR.check(res[0], w, (name, kind, n, lu))
        print(f"{name} {kind} n {n}: {w['n_words']} words, {int((w['node_of'] != RV.NONE).sum())} features in {len(set(w['node_of'].tolist()) - {RV.NONE})} nodes")
        _, again, out, _ = rig.run(name, [rows], lu)                                       # two runs: identical bytes
        out.free()
        assert np.array_equal(again, raw), (name, kind, n)


def test_three_frames_in_records(rig):
    """B = 3 on descriptor blocks that sit inside record-sized buffers, xfh_record_bytes(n) apart, guard bytes round every output (VocabRig.run
    checks them): every frame equals its own B = 1 answer, and two runs give identical bytes"""
    name = "irregular"
    voc = VR.vocabulary(name)
    for n, kinds in ((257, ("mixed", "stopped")), (4096, ("mixed", "oneword", "stopped"))):
        frames = [VR.features(name, k, n) for k in kinds]
        if len(frames) < 3:
            frames.append(np.ascontiguousarray(np.roll(frames[0], 11, 0)))
        for lu in (1, 4):
            res, raw, out, _ = rig.run(name, frames, lu, records=True)
            out.free()
            for b, k in enumerate(kinds):
                VR.check(res[b], VR.want(name, k, n, lu), (n, k, lu))
            if len(kinds) < 3:
                VR.check(res[2], RV.vectorised(voc, frames[2], lu), (n, "rolled", lu))
            assert len({r["n_words"] for r in res}) >= 2
            _, again, out, _ = rig.run(name, frames, lu, records=True)
            out.free()
            assert np.array_equal(again, raw), (n, lu)


def test_largest_frame(rig):
    """n = XFH_GRID_MAX_N: 16384 keys are 128 KB of LDS, the size at which k_vocab_finish needs the large-LDS opt-in; two frames in one call"""
    n, lu = capi.GRID_MAX_N, 1
    rows = VR.features("dfs", "mixed", n)
    frames = [rows, np.ascontiguousarray(rows[::-1])]
    res, raw, out, _ = rig.run("dfs", frames, lu)
    out.free()
    VR.check(res[0], VR.want("dfs", "mixed", n, lu), ("largest", 0))
    VR.check(res[1], RV.vectorised(VR.vocabulary("dfs"), frames[1], lu), ("largest", 1))
    assert res[0]["n_words"] == res[1]["n_words"] > 900 and not np.array_equal(res[0]["nodes"], res[1]["nodes"])
    _, again, out, _ = rig.run("dfs", frames, lu)
    out.free()
    assert np.array_equal(again, raw)


def test_device_blob_feeds_bow_search(rig, oracle_mod):
    """the chain the call exists for: the node blobs the transform wrote on the device go straight into xfh_bow_search_device, and the answer
    is that of the same search on blobs packed on the host from the restatement's node_of"""
    s = BR.Scene()
    name, lu = "bfs", 2                                                                    # L = 3: the nodes of level 1, ten of them
    ctx = rig.ctx
    n1, n2 = BR.N1, BR.N2
    sides = []
    for rows in (s.s1["desc"], s.s2[0]["desc"]):
        res, _, out, lay = rig.run(name, [rows], lu)
        want = RV.vectorised(VR.vocabulary(name), rows, lu)
        VR.check(res[0], want, ("scene", len(rows)))
        sides.append((out, lay, want))
    assert len(set(sides[0][2]["node_of"].tolist()) & set(sides[1][2]["node_of"].tolist())) >= 5
    stride1, stride2 = (n1 + 1) * 256, (n2 + 1) * 256
    d1 = capi.DeviceBuffer(stride1).upload(np.ascontiguousarray(s.s1["desc"], F))
    d2 = capi.DeviceBuffer(stride2).upload(np.ascontiguousarray(s.s2[0]["desc"], F))
    act = capi.DeviceBuffer(n1 + 16).upload(s.s1["active"])
    ws = capi.DeviceBuffer(Context.bow_search_workspace_bytes(n1, n2, 1))
    lay = Context.bow_search_layout(1, n1, n2)
    raws = []
    for form in ("device", "host"):
        if form == "device":
            b1, b2 = sides[0][0].ptr + sides[0][1]["nodes"], sides[1][0].ptr + sides[1][1]["nodes"]
            keep = []
        else:
            keep = [capi.DeviceBuffer(Context.nodes_bytes(n)).upload(Context.nodes_pack(w["node_of"])[:Context.nodes_bytes(n)]) for n, (_, _, w) in zip((n1, n2), sides)]
            b1, b2 = keep[0].ptr, keep[1].ptr
        out = capi.DeviceBuffer(lay["bytes"]).upload(np.full(lay["bytes"], 0xA5, np.uint8))
        ctx.bow_search_device(1, n1, n2, 0, b1, act.ptr, d1.ptr, stride1, b2, None, d2.ptr, stride2, ws.ptr, out.ptr, nn_ratio=0.9)
        ctx.synchronize()
        raws.append(out.download(np.uint8, lay["bytes"]))
        out.free()
        for k in keep:
            k.free()
    assert np.array_equal(raws[0], raws[1])
    status = raws[0][lay["status"]:lay["status"] + n1]
    nm = int(raws[0][lay["n_matches"]:lay["n_matches"] + 4].view(np.int32)[0])
    # ... and it is the search the restatement describes for that node_of
    m = BR.RB.per_node(s.dist(oracle_mod, 0, 0), sides[0][2]["node_of"], s.s1["active"], sides[1][2]["node_of"], None, 0, nn_ratio=0.9)
    assert np.array_equal(status, m["status"]) and nm == m["n_matches"] > 0
    assert np.array_equal(raws[0][lay["match12"]:lay["match12"] + 4 * n1].view(np.int32), m["match12"])
    for x in (d1, d2, act, ws, sides[0][0], sides[1][0]):
        x.free()


def test_host_form_and_matcher(rig):
    for name, kind, n, lu in (("irregular", "mixed", 257, 1), ("dfs", "mixed", 4096, 4), ("irregular", "stopped", 257, 0), ("bfs", "mixed", 1, 1)):
        rows = VR.features(name, kind, n)
        h = rig.ctx.bow_transform(VR.blob(name), rows, lu)
        res, _, out, _ = rig.run(name, [rows], lu)
        out.free()
        d = res[0]
        k = d["n_words"]
        assert h["n_words"] == k and np.array_equal(h["bow_ids"], d["bow_ids"][:k]) and np.array_equal(h["bow_vals"].view(np.uint64), d["bow_vals"][:k].view(np.uint64))
        for key in ("word", "node_of", "nodes"):
            assert np.array_equal(h[key], d[key]), (name, key)
        assert np.array_equal(h["weight"].view(np.uint64), d["weight"].view(np.uint64))
    m = ORBmatcher(ctx=rig.ctx)
    rows = VR.features("irregular", "mixed", 257)
    bow, node_of, r = m.ComputeBoW(VR.blob("irregular"), rows)                             # levelsup = 4, as Frame::ComputeBoW
    w = VR.want("irregular", "mixed", 257, 4)
    assert [b[0] for b in bow] == w["bow_ids"].tolist() and np.array_equal(np.array([b[1] for b in bow]).view(np.uint64), w["bow_vals"].view(np.uint64))
    assert np.array_equal(node_of, w["node_of"])


def test_invalid_arguments_launch_nothing(rig):
    L, ctx = rig.L, rig.ctx
    name, n = "bfs", 257
    dv, nb = rig.vocab(name)
    rows = VR.features(name, "mixed", n)
    lay = Context.bow_transform_layout(1, n)
    sent = np.full(lay["bytes"], 0xA5, np.uint8)
    out = capi.DeviceBuffer(lay["bytes"]).upload(sent)
    dd = capi.DeviceBuffer(n * 256 + 32).upload(rows)
    ws = capi.DeviceBuffer(Context.bow_transform_workspace_bytes(n, 1) + 32)
    base = dict(ctx=ctx.h, B=1, n=n, lu=4, flags=0, voc=dv.ptr, vb=nb, desc=dd.ptr, st=n * 256, ws=ws.ptr, word=out.ptr + lay["word"], no=out.ptr + lay["node_of"],
                wt=out.ptr + lay["weight"], nodes=out.ptr + lay["nodes"], ids=out.ptr + lay["bow_ids"], vals=out.ptr + lay["bow_vals"], nw=out.ptr + lay["n_words"])

    def call(**kw):
        a = dict(base); a.update(kw)
        return L.xfh_bow_transform_device(*[a[k] for k in base])

    bad = [dict(B=0), dict(B=-1), dict(B=65536), dict(n=0), dict(n=-1), dict(n=capi.GRID_MAX_N + 1), dict(lu=-1), dict(flags=1), dict(flags=2), dict(flags=-1),
           dict(vb=0), dict(vb=63), dict(vb=Context.vocab_bytes(2) - 1), dict(voc=base["voc"] + 8), dict(desc=base["desc"] + 4), dict(st=n * 256 + 8),
           dict(ws=base["ws"] + 8), dict(nodes=base["nodes"] + 8), dict(wt=base["wt"] + 4), dict(vals=base["vals"] + 4), dict(word=base["word"] + 2),
           dict(no=base["no"] + 1), dict(ids=base["ids"] + 2), dict(nw=base["nw"] + 2)] + [{k: None} for k in ("ctx", "voc", "desc", "ws", "word", "no", "wt", "nodes", "ids", "vals", "nw")]
    ctx.synchronize()
    for kid in ("VOCAB_DESCEND", "VOCAB_FINISH"):
        ctx.timing_enable(capi.K[kid])
        for kw in bad:
            assert call(**kw) == 1, kw
        ctx.synchronize()
        assert ctx.timing_read()[0] == 0 and np.array_equal(out.download(np.uint8, lay["bytes"]), sent)
        assert call() == 0 and call(lu=0) == 0 and call(lu=100) == 0 and call(vb=nb - 32) == 0     # the valid calls still work afterwards (a short blob is clamped)
        ctx.synchronize()
        assert ctx.timing_read()[0] == 4 and not np.array_equal(out.download(np.uint8, lay["bytes"]), sent)
        ctx.timing_enable(capi.K["NONE"])
        out.upload(sent)
    # the host form refuses the same classes before it stages anything
    blob = VR.blob(name)
    houts = dict(word=np.full(4 * n, 0xA5, np.uint8), no=np.full(4 * n, 0xA5, np.uint8), wt=np.full(8 * n, 0xA5, np.uint8), nodes=np.full(Context.nodes_bytes(n), 0xA5, np.uint8),
                 ids=np.full(4 * n, 0xA5, np.uint8), vals=np.full(8 * n, 0xA5, np.uint8), nw=np.full(4, 0xA5, np.uint8))
    r32 = np.ascontiguousarray(rows, F)
    hb = dict(ctx=ctx.h, n=n, lu=4, flags=0, voc=blob.ctypes.data, vb=nb, desc=r32.ctypes.data, **{k: a.ctypes.data for k, a in houts.items()})

    def hcall(**kw):
        a = dict(hb); a.update(kw)
        return L.xfh_bow_transform(*[a[k] for k in hb])

    hbad = [dict(ctx=None), dict(n=0), dict(n=capi.GRID_MAX_N + 1), dict(lu=-2), dict(flags=1), dict(vb=10), dict(voc=None), dict(desc=None)] + [{k: None} for k in houts]
    ctx.timing_enable(capi.K["VOCAB_FINISH"])
    for kw in hbad:
        assert hcall(**kw) == 1, kw
    assert ctx.timing_read()[0] == 0 and all(np.all(a == 0xA5) for a in houts.values())
    assert hcall() == 0
    assert ctx.timing_read()[0] == 1 and not any(np.all(a == 0xA5) for a in houts.values())
    ctx.timing_enable(capi.K["NONE"])
    for x in (out, dd, ws):
        x.free()
