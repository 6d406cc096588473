"""xfh_bowdb_query_device (k_bowdb_score, k_bowdb_select) against the order-free rule of tests/ref_bowdb.py on the databases of
tests/bowdb_rig.py.  Every comparison is equality of integers or of the bits of doubles and floats: common, score, status, the header, best_acc,
the scored list with acc and pBestKF, the candidate sequence, and the state array after the call.  The conditions the databases are chosen for
are asserted where they are built, on the CPU (tests/bowdb_rig.py, tests/test_bowdb_ref.py)."""
import numpy as np
import pytest

import bowdb_rig as R
import ref_bowdb as RB
import ref_vocab as RV
import vocab_rig as VR
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context, KeyFrameDatabase

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def rig(gpu_lib):
    r = R.DeviceRig(gpu_lib)
    yield r
    r.close()


@pytest.mark.parametrize("name", R.NAMES)
def test_every_database_both_forms(rig, name):
    """the case's queries as a chain on one state array per form (the stale-state chain among them); n_slots 1, 63, 65, 300 and strides 8 and
    257 are the random databases; two runs give identical bytes"""
    for form in R.FORMS:
        raws = rig.chain(name, form)
        again = rig.chain(name, form)
        assert all(np.array_equal(a, b) for a, b in zip(raws, again)), (name, form)
    w = R.want(name, RB.NBEST)
    print(f"{name}: " + ", ".join(f"{r['n_listed']} listed / {r['n_scored']} scored / {r['n_candidates']} candidates" for r in w))


@pytest.mark.parametrize("name", ("random_65_8", "random_300_257"))
def test_three_queries_in_one_call(rig, name):
    """B = 3 queries against one database, each with its own exclusion and state: every problem equals its own B = 1 answer"""
    c = R.case(name)
    n = len(c["db"]["vecs"])
    rng = np.random.RandomState(3)
    states = (rng.rand(3, n) * 0.3).astype(F)
    for form in R.FORMS:
        res, raw, after = rig.run(name, c, form, c["queries"], states)
        for b, q in enumerate(c["queries"]):
            st = states[b].copy()
            w = RB.rule(c["db"], q["q"], form, st, q["exclude"])
            R.check(res[b], w, (name, form, b))
            assert np.array_equal(after[b].view(np.uint32), st.view(np.uint32))
            one, _, after1 = rig.run(name, c, form, [q], states[b][None])
            R.check(one[0], w, (name, form, b, "B = 1"))
            assert np.array_equal(after1[0].view(np.uint32), st.view(np.uint32))
        assert len({r["n_scored"] for r in res}) >= 2
        _, again, _ = rig.run(name, c, form, c["queries"], states)
        assert np.array_equal(again, raw)


def test_stale_state_chain(rig):
    """two successive queries on one state array differ from two fresh ones, on the device as in the rule"""
    c = R.case("stale")
    for form in R.FORMS:
        z = c["state0"][None]
        r1, _, s1 = rig.run("stale", c, form, [c["queries"][0]], z)
        chained, _, _ = rig.run("stale", c, form, [c["queries"][1]], s1)
        fresh, _, _ = rig.run("stale", c, form, [c["queries"][1]], z)
        wc, wf = R.run_chain(c, form)[1], R.run_chain(c, form, fresh=True)[1]
        R.check(chained[0], wc, ("chained", form)); R.check(fresh[0], wf, ("fresh", form))
        assert R.cands(chained[0]) != R.cands(fresh[0]) and chained[0]["list_acc"][0] != fresh[0]["list_acc"][0]


def test_most_slots(rig):
    """n_slots = XFH_BOWDB_MAX_SLOTS with vectors of at most 8 words: the select kernel's sorts and LDS at their largest, a list of more than a
    thousand entries, d_seq a permutation"""
    assert len(R.case("many_slots")["db"]["vecs"]) == capi.BOWDB_MAX_SLOTS and R.case("many_slots")["db"]["seq"] is not None
    for form in R.FORMS:
        rig.chain("many_slots", form)


def test_widest_vectors(rig):
    """4 slots at stride XFH_GRID_MAX_N with 16384-word vectors: the score kernel's largest LDS staging and an ordered sum of thousands of terms"""
    assert R.case("widest")["stride"] == capi.GRID_MAX_N
    for form in R.FORMS:
        rig.chain("widest", form)


def test_hostile_word_counts_are_clamped(rig):
    """n_words beyond the stride on slots that are filled to it, and below zero on empty ones: clamped to [0, stride] before use, so the answer is
    that of the honest counts"""
    c = R.case("random_63_8")
    full = [s for s, v in enumerate(c["db"]["vecs"]) if v is not None and len(v[0]) == c["stride"]]
    empty = [s for s, v in enumerate(c["db"]["vecs"]) if v is None]
    assert len(full) >= 3 and len(empty) >= 3
    claims = {full[0]: c["stride"] + 1, full[1]: 1 << 30, full[2]: 0x7fffffff, empty[0]: -1, empty[1]: -(1 << 31), empty[2]: -5}
    hostile = dict(c, claims=claims)
    for form in R.FORMS:
        state = c["state0"].copy()
        for i, q in enumerate(c["queries"]):
            res, _, after = rig.run("random_63_8_hostile", hostile, form, [q], state[None])
            R.check(res[0], R.want("random_63_8", form)[i], ("hostile", form, i))
            state = after[0]


def test_transform_writes_the_slots(rig):
    """the chain the call exists for: xfh_bow_transform_device writes three frames straight into database slots (db_stride == n), a fourth
    frame is the query, and the answer is the rule's on vectors built on the host"""
    name, n, lu = "irregular", 257, 4
    ctx = rig.ctx
    frames = [VR.features(name, "mixed", n), np.ascontiguousarray(np.roll(VR.features(name, "mixed", n), 5, 0)[::-1]), VR.features(name, "stopped", n),
              np.ascontiguousarray(np.roll(VR.features(name, "mixed", n), 11, 0))]
    blob = VR.blob(name)
    nb = Context.vocab_bytes(len(VR.vocabulary(name)["parent"]))
    dv = capi.DeviceBuffer(nb).upload(blob[:nb])
    n_slots = 5                                                                                # slots 0, 2, 3 are written; 1 and 4 stay empty
    ids = capi.DeviceBuffer(4 * n_slots * n).upload(np.zeros(4 * n_slots * n, np.uint8))
    vals = capi.DeviceBuffer(8 * n_slots * n).upload(np.zeros(8 * n_slots * n, np.uint8))
    nw = capi.DeviceBuffer(4 * n_slots).upload(np.zeros(n_slots, np.int32))
    qbuf = dict(ids=capi.DeviceBuffer(4 * n), vals=capi.DeviceBuffer(8 * n), nw=capi.DeviceBuffer(4))
    ws = capi.DeviceBuffer(Context.bow_transform_workspace_bytes(n, 1))
    lay = Context.bow_transform_layout(1, n)
    scratch = capi.DeviceBuffer(lay["bytes"])
    L = capi.lib()
    vecs = [None] * n_slots
    keep = [dv, ids, vals, nw, ws, scratch, *qbuf.values()]
    for f, slot in zip(frames, (0, 2, 3, None)):
        rows = capi.DeviceBuffer(n * 256 + 16).upload(np.ascontiguousarray(f, F))
        keep.append(rows)
        bi, bv, bn = (qbuf["ids"].ptr, qbuf["vals"].ptr, qbuf["nw"].ptr) if slot is None else (ids.ptr + 4 * slot * n, vals.ptr + 8 * slot * n, nw.ptr + 4 * slot)
        capi.check(L.xfh_bow_transform_device(ctx.h, 1, n, lu, capi.BOWT_TF_IDF_L1, dv.ptr, nb, rows.ptr, 0, ws.ptr, scratch.ptr + lay["word"],
                                              scratch.ptr + lay["node_of"], scratch.ptr + lay["weight"], scratch.ptr + lay["nodes"], bi, bv, bn), ctx.h)
        w = RV.vectorised(VR.vocabulary(name), f, lu)
        v = (w["bow_ids"], w["bow_vals"])
        if slot is None:
            query = v
        else:
            vecs[slot] = v if w["n_words"] else None
    assert vecs[3] is None and len(vecs[0][0]) > 20                                           # the stopped frame leaves an empty slot
    db = R.make_db(vecs, {0: [2, 3], 2: [0]}, nn=2)
    neigh = capi.DeviceBuffer(db["neigh"].nbytes).upload(db["neigh"])
    keep.append(neigh)
    qlay = Context.bowdb_query_layout(1, n_slots)
    for form in R.FORMS:
        state = capi.DeviceBuffer(4 * n_slots).upload(np.zeros(n_slots, F))
        qws = capi.DeviceBuffer(Context.bowdb_query_workspace_bytes(n_slots, 1))
        out = capi.DeviceBuffer(qlay["bytes"])
        ctx.bowdb_query_device(1, n_slots, form, qbuf["ids"].ptr, qbuf["vals"].ptr, qbuf["nw"].ptr, n, ids.ptr, vals.ptr, nw.ptr, n, None, neigh.ptr, 2, None,
                               state.ptr, qws.ptr, out.ptr)
        ctx.synchronize()
        res = Context.bowdb_query_parse(out.download(np.uint8, qlay["bytes"]), qlay, 1, n_slots)[0]
        st = np.zeros(n_slots, F)
        w = RB.rule(db, query, form, st)
        R.check(res, w, ("transform", form))
        assert w["n_scored"] >= 1 and w["status"].tolist()[1] == RB.EMPTY and w["status"].tolist()[3] == RB.EMPTY
        assert np.array_equal(state.download(F, n_slots).view(np.uint32), st.view(np.uint32))
        for x in (state, qws, out):
            x.free()
    for x in keep:
        x.free()


def test_host_form_and_database_class(rig):
    """xfh_bowdb_query (host pointers) and the KeyFrameDatabase class give the device form's answers; the map split and the caps are the caller's"""
    for name in ("samebest", "exclusion", "random_63_8"):
        c = R.case(name)
        ids, vals, nw = R.pack(c["db"], c["stride"])
        for form in R.FORMS:
            state, ref_state = c["state0"].copy(), c["state0"].copy()
            for i, q in enumerate(c["queries"]):
                ex = np.zeros(len(nw), np.uint8); ex[list(q["exclude"])] = 1
                r = rig.ctx.bowdb_query(form, q["q"][0], q["q"][1], ids, vals, nw, c["db"]["neigh"], state, seq=c["db"]["seq"], exclude=ex if ex.any() else None)
                R.check(r, RB.rule(c["db"], q["q"], form, ref_state, q["exclude"]), (name, form, i, "host form"))
                assert np.array_equal(state.view(np.uint32), ref_state.view(np.uint32))
    c = R.case("samebest")
    db = KeyFrameDatabase(rig.ctx, 5, 8, nn=3)                                                  # (the query has six words: the stride is the database's and the query's)
    order = sorted((s for s in range(5) if c["db"]["vecs"][s] is not None), key=lambda s: int(c["db"]["seq"][s]))     # `add` in insertion order
    for s in order:
        db.add(s, *c["db"]["vecs"][s], neighbours=[int(t) for t in c["db"]["neigh"][s] if 0 <= t < 5])
    q = c["queries"][0]["q"]
    assert db.DetectRelocalizationCandidates(*q) == [1] and db.DetectRelocalizationCandidates(*q, map_of_slot=[0, 7, 0, 0, 0], pMap=0) == []
    maps = [0, 0, 1, 0, 1]
    assert db.DetectNBestCandidates(*q, connected=(), nNumCandidates=3, map_of_slot=maps, query_map=0) == ([1], [4, 2])
    assert db.DetectNBestCandidates(*q, connected=(), nNumCandidates=1, map_of_slot=maps, query_map=0) == ([1], [4])
    assert db.DetectNBestCandidates(*q, connected=(1,), nNumCandidates=3, map_of_slot=maps, query_map=0)[1] == [4, 2]
    db.erase(4)
    assert db.DetectNBestCandidates(*q, connected=(), nNumCandidates=3, map_of_slot=maps, query_map=0) == ([1], [2])
    db.close()


def test_invalid_arguments_launch_nothing(rig):
    L, ctx = rig.L, rig.ctx
    name = "random_63_8"
    c = R.case(name)
    n, stride = 63, 8
    d = rig.database(name, c)
    lay = Context.bowdb_query_layout(1, n)
    sent = np.full(lay["bytes"], 0xA5, np.uint8)
    out = capi.DeviceBuffer(lay["bytes"]).upload(sent)
    q = c["queries"][0]["q"]
    qi = capi.DeviceBuffer(64).upload(np.ascontiguousarray(q[0], np.uint32)); qv = capi.DeviceBuffer(128).upload(np.ascontiguousarray(q[1], np.float64))
    qn = capi.DeviceBuffer(16).upload(np.array([len(q[0])], np.int32))
    st = capi.DeviceBuffer(4 * n + 16).upload(np.zeros(n, F))
    ex = capi.DeviceBuffer(n + 16).upload(np.zeros(n, np.uint8))
    ws = capi.DeviceBuffer(Context.bowdb_query_workspace_bytes(n, 1) + 32)
    base = dict(ctx=ctx.h, B=1, n=n, form=0, qi=qi.ptr, qv=qv.ptr, qn=qn.ptr, qs=8, di=d["ids"].ptr, dv=d["vals"].ptr, dn=d["nw"].ptr, ds=stride, seq=d["seq"].ptr,
                neigh=d["neigh"].ptr, nn=10, ex=ex.ptr, st=st.ptr, ws=ws.ptr, common=out.ptr + lay["common"], score=out.ptr + lay["score"],
                status=out.ptr + lay["status"], header=out.ptr + lay["header"], best=out.ptr + lay["best_acc"], ls=out.ptr + lay["list_slot"],
                la=out.ptr + lay["list_acc"], lb=out.ptr + lay["list_best"], cs=out.ptr + lay["cand_slot"], ca=out.ptr + lay["cand_acc"])

    def call(**kw):
        a = dict(base); a.update(kw)
        return L.xfh_bowdb_query_device(*[a[k] for k in base])

    outs = ("common", "score", "status", "header", "best", "ls", "la", "lb", "cs", "ca")
    bad = [dict(B=0), dict(B=-1), dict(B=65536), dict(n=0), dict(n=-1), dict(n=capi.BOWDB_MAX_SLOTS + 1), dict(form=2), dict(form=-1), dict(qs=0),
           dict(qs=capi.GRID_MAX_N + 1), dict(ds=0), dict(ds=-8), dict(ds=capi.GRID_MAX_N + 1), dict(nn=-1), dict(nn=capi.BOWDB_MAX_NEIGHBOURS + 1),
           dict(ws=base["ws"] + 8), dict(qv=base["qv"] + 4), dict(dv=base["dv"] + 4), dict(score=base["score"] + 4), dict(qi=base["qi"] + 2), dict(qn=base["qn"] + 2),
           dict(di=base["di"] + 1), dict(dn=base["dn"] + 2), dict(seq=base["seq"] + 2), dict(neigh=base["neigh"] + 2), dict(st=base["st"] + 2)]
    bad += [{k: base[k] + 2} for k in outs if k not in ("score", "status")]
    bad += [{k: None} for k in ("ctx", "qi", "qv", "qn", "di", "dv", "dn", "neigh", "st", "ws") + outs]
    ctx.synchronize()
    for kid in ("BOWDB_SCORE", "BOWDB_SELECT"):
        ctx.timing_enable(capi.K[kid])
        for kw in bad:
            assert call(**kw) == 1, kw
        ctx.synchronize()
        assert ctx.timing_read()[0] == 0 and np.array_equal(out.download(np.uint8, lay["bytes"]), sent)
        assert call() == 0 and call(seq=None, ex=None) == 0 and call(nn=0, neigh=None) == 0 and call(form=1) == 0      # the valid calls still work afterwards
        ctx.synchronize()
        assert ctx.timing_read()[0] == 4 and not np.array_equal(out.download(np.uint8, lay["bytes"]), sent)
        ctx.timing_enable(capi.K["NONE"])
        out.upload(sent)
    assert L.xfh_kernel_name(capi.K["BOWDB_SCORE"]) == b"k_bowdb_score" and L.xfh_kernel_name(capi.K["BOWDB_SELECT"]) == b"k_bowdb_select"
    for x in (out, qi, qv, qn, st, ex, ws):
        x.free()
