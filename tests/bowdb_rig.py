"""Seeded keyframe databases for the database query (xfh_bowdb_query*), each built for a condition that is ASSERTED here, on the CPU, with the
order-free rule of tests/ref_bowdb.py (tests/test_bowdb_ref.py holds that rule against the literal transcription on every one of them).

A case is dict(db, stride, queries = [dict(q = (ids, vals), exclude = slots)], state0): the queries run one after the other on ONE state array
per form (the persistent mRelocScore / mPlaceRecognitionScore), starting from state0.  For positive values a term of the score is
-2 * min(vi, wi), so score = the sum of min(vi, wi) over the shared words: the hand-made cases choose their values by that."""
import functools

import numpy as np

import ref_bowdb as RB

F = np.float32
FORMS = (RB.RELOC, RB.NBEST)


def mk(d):
    """{word: value} -> (ids ascending, vals)"""
    ks = sorted(d)
    return np.array(ks, np.uint32), np.array([d[k] for k in ks], np.float64)


def make_db(vecs, neigh=None, nn=0, seq=None):
    n = len(vecs)
    ng = np.full((n, nn), -1, np.int32)
    for s, lst in (neigh or {}).items():
        ng[s, :len(lst)] = lst
    return dict(vecs=list(vecs), neigh=ng, seq=None if seq is None else np.asarray(seq, np.uint32))


def pack(db, stride):
    """the database as the device arrays: ids [n][stride] (0xFFFFFFFF behind the words, as the transform pads), vals, n_words"""
    n = len(db["vecs"])
    ids, vals, nw = np.full((n, stride), 0xFFFFFFFF, np.uint32), np.zeros((n, stride), np.float64), np.zeros(n, np.int32)
    for s, v in enumerate(db["vecs"]):
        if v is not None:
            k = len(v[0])
            assert k <= stride and np.all(np.diff(v[0].astype(np.int64)) > 0)
            ids[s, :k], vals[s, :k], nw[s] = v[0], v[1], k
    return ids, vals, nw


def run_chain(case, form, fn=RB.rule, fresh=False):
    """the case's queries in order on one state array (fresh: every query on a copy of state0) -> the results"""
    state = case["state0"].copy()
    out = []
    for q in case["queries"]:
        if fresh:
            state = case["state0"].copy()
        out.append(fn(case["db"], q["q"], form, state, q["exclude"]))
    return out


def cands(r):
    return r["cand_slot"][:r["n_candidates"]].tolist()


def _case(db, stride, queries, state0=None):
    n = len(db["vecs"])
    return dict(db=db, stride=stride, queries=[dict(q=q, exclude=tuple(e)) for q, e in queries], state0=np.zeros(n, F) if state0 is None else state0)


def stale():
    """slot 1 is scored by the first query and only LISTED, below the threshold, by the second, where it is the neighbour of slot 0: its state
    from the first query changes acc of slot 0 and the candidate set of the second query"""
    q1 = mk({100 + i: 0.1 for i in range(10)})
    q2 = mk({10 + i: 0.1 for i in range(10)})
    vecs = [mk({10 + i: 0.03 for i in range(10)}),                                             # 0: all ten words of q2, score 0.3
            mk({**{100 + i: 0.09 for i in range(10)}, 10: 0.01, 11: 0.01}),                     # 1: q1's words (score 0.9), two of q2's
            mk({11 + i: 0.03 for i in range(9)}),                                              # 2: nine words of q2, score 0.27
            None]
    c = _case(make_db(vecs, {0: [1]}, nn=2), 16, [(q1, ()), (q2, ())])
    for form in FORMS:
        chain, fresh = run_chain(c, form), run_chain(c, form, fresh=True)
        assert chain[1]["status"].tolist() == [RB.SCORED, RB.BELOW_MIN, RB.SCORED, RB.EMPTY] and chain[0]["status"][1] == RB.SCORED
        assert chain[1]["list_acc"][0] != fresh[1]["list_acc"][0] and cands(chain[1]) != cands(fresh[1]), (cands(chain[1]), cands(fresh[1]))
    assert cands(run_chain(c, RB.RELOC)[1]) == [1] and cands(run_chain(c, RB.RELOC, fresh=True)[1]) == [0, 2]
    return c


def exclusion():
    """slot 0 would hold max_common (10) and is excluded: max_common is 5, min_common 4, and slot 3 with exactly 4 shared words is not scored"""
    q = mk({i: 0.1 for i in range(10)})
    vecs = [mk({i: 0.1 for i in range(10)}), mk({i: 0.05 for i in range(5)}), mk({i + 3: 0.04 for i in range(5)}), mk({i + 6: 0.2 for i in range(4)}),
            mk({50: 1.0}), None, mk({9: 0.3, 77: 0.1})]
    c = _case(make_db(vecs, {1: [0, 3, 6], 2: [1]}, nn=3), 12, [(q, (0, 4)), (q, ())])
    for form in FORMS:
        r = run_chain(c, form, fresh=True)
        assert (r[0]["max_common"], r[0]["min_common"]) == (5, 4) and (r[1]["max_common"], r[1]["min_common"]) == (10, 8)
        assert r[0]["status"].tolist() == [RB.EXCLUDED, RB.SCORED, RB.SCORED, RB.BELOW_MIN, RB.NOT_SHARING, RB.EMPTY, RB.BELOW_MIN] and r[0]["common"][3] == 4
        assert r[1]["status"].tolist()[:4] == [RB.SCORED, RB.BELOW_MIN, RB.BELOW_MIN, RB.BELOW_MIN]
    return c


def ladder():
    """slot j shares min(j, k) words with the query of k words: max_common = k for k in 1, 4, 5, 6, 10, so min_common = (int)(k * 0.8f) =
    0, 3, 4, 4, 8 (5 * 0.8f and 10 * 0.8f are a hair above 4 and 8 in fp32), and slot min_common has exactly min_common shared words"""
    vecs = [None] + [mk({**{i: 0.02 * (1 + (i + j) % 3) for i in range(j)}, 1000 + j: 0.5}) for j in range(1, 11)]
    ks = (1, 4, 5, 6, 10)
    c = _case(make_db(vecs, {j: [j - 1, j + 1] for j in range(1, 11)}, nn=2), 11, [(mk({i: 0.1 for i in range(k)}), ()) for k in ks])
    for form in FORMS:
        for k, r, mn in zip(ks, run_chain(c, form), (0, 3, 4, 4, 8)):
            assert (r["max_common"], r["min_common"]) == (k, mn) and r["n_scored"] == 10 - mn
            assert mn == 0 or (r["common"][mn] == mn and r["status"][mn] == RB.BELOW_MIN and r["status"][mn + 1] == RB.SCORED)
    return c


def samebest():
    """list order X(3), Z(1), N2(4), N1(2): X and Z both name Z as pBestKF; X fails the 0.75 test and comes EARLIER than Z (RELOC keeps Z with Z's
    acc); N1 and N2 have equal acc and the stable sort keeps the list order, which d_seq (slot 2 was reused: added last) decides"""
    q = mk({i: 1.0 for i in range(6)})
    X, Z, N1, N2 = 3, 1, 2, 4
    vecs = [None] * 5
    vecs[X] = mk({0: 0.025, 1: 0.025, 2: 0.025, 3: 0.025})
    vecs[Z] = mk({1: 0.125, 2: 0.125, 3: 0.125, 4: 0.125})
    vecs[N1] = mk({2: 0.125, 3: 0.125, 4: 0.125, 5: 0.0625})
    vecs[N2] = mk({2: 0.125, 3: 0.125, 4: 0.125, 5: 0.0625})
    seq = [0, 1, 9, 3, 4]
    c = _case(make_db(vecs, {X: [Z], Z: [N1, 7, N2]}, nn=3, seq=seq), 4, [(q, ())])
    rel, nb = run_chain(c, RB.RELOC)[0], run_chain(c, RB.NBEST)[0]
    assert rel["list_slot"][:4].tolist() == [X, Z, N2, N1] and rel["list_best"][:4].tolist() == [Z, Z, N2, N1]
    assert not rel["list_acc"][0] > F(0.75) * rel["best_acc"] and cands(rel) == [Z] and rel["cand_acc"][0] == rel["list_acc"][1]
    assert rel["list_acc"][2] == rel["list_acc"][3] and cands(nb) == [Z, N2, N1] and nb["cand_acc"][0] == nb["list_acc"][1]
    noseq = dict(c, db=dict(c["db"], seq=None))
    assert cands(run_chain(noseq, RB.NBEST)[0]) == [Z, N1, N2]                                # without d_seq the slot order decides: another output
    return c


def oneword_full():
    """a one-word query (max_common 1, min_common 0: every sharing slot is scored) against slots filled to the stride, an empty vector and
    words 0 and 0xFFFFFFFE"""
    stride = 8
    rng = np.random.RandomState(7)
    vecs = []
    for s in range(9):
        w = np.sort(rng.choice(np.arange(1, 40), stride, replace=False)).astype(np.uint32)
        if s % 2 == 0:
            w[0] = 0
        if s % 3 == 0:
            w[-1] = 0xFFFFFFFE
        vecs.append((w, rng.rand(stride) / stride))
    vecs[4] = None
    vecs[7] = (np.zeros(0, np.uint32), np.zeros(0))
    qs = [(mk({0: 1.0}), ()), (mk({0xFFFFFFFE: 1.0}), (0,)), (mk({0: 0.5, 0xFFFFFFFE: 0.5}), ()), ((np.zeros(0, np.uint32), np.zeros(0)), ())]
    c = _case(make_db(vecs, {s: [(s + 1) % 9, (s + 5) % 9, 9, -3] for s in range(9)}, nn=4), stride, qs)
    r = run_chain(c, RB.RELOC)
    assert (r[0]["max_common"], r[0]["min_common"]) == (1, 0) and r[0]["n_scored"] == r[0]["n_listed"] == 4 and r[3]["n_listed"] == 0
    assert all(len(v[0]) == stride for s, v in enumerate(vecs) if s not in (4, 7))
    return c


def long_sum():
    """an intersection of more than 64 words spread over several 64-entry chunks of the slot; the left-to-right sum, the reversed sum and
    the pairwise sum give three different bit patterns"""
    rng = np.random.RandomState(11)
    uni = rng.permutation(3000).astype(np.uint32)
    qw = np.sort(uni[:300])
    vecs = []
    for s in range(3):
        w = np.sort(np.concatenate([uni[100:300], uni[400 + 200 * s:600 + 200 * s]]))
        vecs.append((w, rng.rand(len(w)) ** 4 / 37.0))
    q = (qw, rng.rand(300) ** 4 / 41.0)
    c = _case(make_db(vecs, {0: [1, 2], 1: [2]}, nn=2), 512, [(q, ())])
    for v in vecs:
        t = RB.terms(q, v)
        _, p2 = RB.shared(q, v)
        assert len(t) == 200 and len(set((p2 // 64).tolist())) >= 4
        seqsum = np.cumsum(np.concatenate([[0.0], t]))[-1]
        assert seqsum != np.cumsum(np.concatenate([[0.0], t[::-1]]))[-1] and seqsum != np.sum(t), "the order of the sum does not show"
    return c


def random_db(n, stride, seed, nn=10):
    """random words from a universe sized so that slots share words with the queries; neighbours with out-of-range entries; a random insertion
    order; every fifth slot empty; three queries with random exclusions; a random state to start from"""
    rng = np.random.RandomState(seed)
    uni = max(3 * stride, 24)
    def vec():
        k = rng.randint(1, stride + 1)
        v = rng.rand(k) + 0.01
        return np.sort(rng.choice(uni, k, replace=False)).astype(np.uint32), v / v.sum()
    vecs = [None if (s % 5 == 3 and n > 1) else vec() for s in range(n)]
    neigh = {s: rng.randint(-2, n + 2, rng.randint(0, nn + 1)).tolist() for s in range(n)}
    db = make_db(vecs, neigh, nn=nn, seq=rng.permutation(n) if seed % 2 else None)
    qs = [(vec(), np.nonzero(rng.rand(n) < 0.1)[0].tolist()) for _ in range(3)]
    return _case(db, stride, qs, state0=(rng.rand(n) * 0.2).astype(F))


def many_slots(n=8192):
    """the largest database with vectors of at most 8 words: the select kernel's sort and LDS at their largest"""
    c = random_db(n, 8, 4243, nn=10)
    c["queries"].append(dict(q=mk({5: 1.0}), exclude=()))                                      # max_common 1: every sharing slot is scored, a long list
    assert run_chain(c, RB.NBEST)[3]["n_scored"] > 1000
    return c


def widest(stride=16384, n=4):
    """4 slots at the largest stride with 16384-word vectors and an intersection in the thousands"""
    rng = np.random.RandomState(99)
    def vec():
        v = rng.rand(stride) + 0.01
        return np.sort(rng.choice(40000, stride, replace=False)).astype(np.uint32), v / v.sum()
    vecs = [vec() for _ in range(n)]
    q = vec()
    c = _case(make_db(vecs, {0: [1, 2, 3], 2: [0]}, nn=3), stride, [(q, ())])
    assert min(RB.rule_score(q, v)[1] for v in vecs) > 5000
    return c


HAND = dict(stale=stale, exclusion=exclusion, ladder=ladder, samebest=samebest, oneword_full=oneword_full, long_sum=long_sum)
RANDOM = {f"random_{n}_{stride}": functools.partial(random_db, n, stride, 100 + n + stride) for n in (1, 63, 65, 300) for stride in (8, 257)}
NAMES = tuple(HAND) + tuple(RANDOM)


@functools.lru_cache(maxsize=None)
def case(name):
    return {**HAND, **RANDOM, "many_slots": many_slots, "widest": widest}[name]()


@functools.lru_cache(maxsize=None)
def want(name, form):
    """the rule's answers for the case's chain of queries, computed once"""
    return run_chain(case(name), form)


# ---- the device side (GPU tests only) -----------------------------------------------------------------------------------------------------
GUARD = 256
INT_KEYS = ("common", "status", "list_slot", "list_best", "cand_slot", "n_listed", "max_common", "min_common", "n_scored", "n_candidates")
F32_KEYS = ("list_acc", "cand_acc", "best_acc")


def check(res, w, tag):
    """one problem's outputs against the rule: integers equal, doubles and floats equal bit for bit"""
    for k in INT_KEYS:
        assert np.array_equal(res[k], w[k]), (tag, k, res[k], w[k])
    assert np.array_equal(np.ascontiguousarray(res["score"]).view(np.uint64), np.ascontiguousarray(w["score"]).view(np.uint64)), (tag, "score")
    for k in F32_KEYS:
        assert np.array_equal(np.ascontiguousarray(res[k], F).view(np.uint32), np.ascontiguousarray(w[k], F).view(np.uint32)), (tag, k, res[k], w[k])
    assert np.all(res["header"][5:] == 0), (tag, "header")


class DeviceRig:
    def __init__(self, L):
        from xfeatslam_amd.extractor import Context
        self.L, self.ctx = L, Context(nfeatures=1, max_height=32, max_width=32)
        self.dev = {}

    def close(self):
        for bufs in self.dev.values():
            for b in bufs.values():
                if b is not None:
                    b.free()
        self.ctx.close()

    def database(self, name, c):
        """the uploaded arrays of a case's database, kept for the module"""
        from xfeatslam_amd import capi
        if name not in self.dev:
            ids, vals, nw = pack(c["db"], c["stride"])
            for slot, claim in c.get("claims", {}).items():                                   # a word count the arrays do not back: clamped by the library
                nw[slot] = claim
            up = lambda a: capi.DeviceBuffer(a.nbytes + 16).upload(a)
            db = c["db"]
            self.dev[name] = dict(ids=up(ids), vals=up(vals), nw=up(nw), seq=None if db["seq"] is None else up(db["seq"]),
                                  neigh=None if db["neigh"].size == 0 else up(db["neigh"]))
        return self.dev[name]

    def run(self, name, c, form, queries, states):
        """B = len(queries) problems against the case's database in one call; states: float32 [B][n], the state each problem starts from.
        Guard bytes round every output, the workspace and the state are checked.  -> (results per problem, raw output bytes, states after)"""
        import guarded
        from xfeatslam_amd import capi
        from xfeatslam_amd.extractor import Context
        ctx = self.ctx
        B, n, stride = len(queries), len(c["db"]["vecs"]), c["stride"]
        d = self.database(name, c)
        qs = max(1, max(len(q["q"][0]) for q in queries))
        qi, qv, qn = np.full((B, qs), 0xFFFFFFFF, np.uint32), np.zeros((B, qs), np.float64), np.zeros(B, np.int32)
        ex = np.zeros((B, n), np.uint8)
        for b, q in enumerate(queries):
            k = len(q["q"][0])
            qi[b, :k], qv[b, :k], qn[b] = q["q"][0], q["q"][1], k
            ex[b, list(q["exclude"])] = 1
        up = lambda a: capi.DeviceBuffer(a.nbytes + 16).upload(a)
        dqi, dqv, dqn = up(qi), up(qv), up(qn)
        dex = up(ex) if ex.any() else None                                                   # no exclusion at all: the NULL form
        dst = guarded.Guarded(4 * B * n, GUARD, inner=np.ascontiguousarray(states, F), what="the state")
        ws = guarded.Guarded(Context.bowdb_query_workspace_bytes(n, B), GUARD)
        lay = Context.bowdb_query_layout(B, n, GUARD)
        out = guarded.outputs(lay)
        nn = c["db"]["neigh"].shape[1]
        ctx.bowdb_query_device(B, n, form, dqi.ptr, dqv.ptr, dqn.ptr, qs, d["ids"].ptr, d["vals"].ptr, d["nw"].ptr, stride, d["seq"].ptr if d["seq"] else None,
                               d["neigh"].ptr if d["neigh"] else None, nn, dex.ptr if dex else None, dst.ptr, ws.ptr, out.ptr, guard=GUARD)
        ctx.synchronize()
        raw = guarded.download(out, lay)
        ws.download()
        after = dst.download().view(F).reshape(B, n)
        for x in (dqi, dqv, dqn, dex, dst, ws, out):
            if x is not None:
                x.free()
        return Context.bowdb_query_parse(raw, lay, B, n), raw, after

    def chain(self, name, form):
        """the case's queries one after the other (B = 1) on one state array, each checked against the rule; -> the raw output bytes"""
        c = case(name)
        state = c["state0"].copy()
        ref_state = c["state0"].copy()
        raws = []
        for i, q in enumerate(c["queries"]):
            res, raw, after = self.run(name, c, form, [q], state[None])
            w = RB.rule(c["db"], q["q"], form, ref_state, q["exclude"])
            check(res[0], w, (name, form, i))
            assert np.array_equal(after[0].view(np.uint32), ref_state.view(np.uint32)), (name, form, i, "state")
            state = after[0]
            raws.append(raw)
        return raws
