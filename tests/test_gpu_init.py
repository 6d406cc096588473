"""xfh_init_search_device (k_init_candidates, k_init_resolve, k_init_final) against the literal transcription of SearchForInitialization in
tests/ref_init.py, output by output, on the scenes and with the guarded runs of tests/init_rig.py.  Every comparison is equality of integers
and bits.  The conditions the scenes are chosen for are asserted where the seeds are chosen, on the CPU (tests/test_init_ref.py); here the
counts are printed."""
import ctypes as C

import numpy as np
import pytest

import guarded
import ref_init as RI
import ref_window as RW
from init_rig import InitRig
from projection_rig import F, GUARD
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context

pytestmark = pytest.mark.gpu
NONE = RI.NONE


@pytest.fixture(scope="module")
def rig(gpu_lib, weights_dense, oracle_mod):
    r = InitRig(gpu_lib, weights_dense[1], 1000, 1200, oracle_mod)
    r.models = {}
    yield r
    r.close()


@pytest.fixture(scope="module")
def rig4096(gpu_lib, weights_dense, oracle_mod):
    r = InitRig(gpu_lib, weights_dense[1], 4096, 1201, oracle_mod)
    yield r
    r.close()


def model(rig, p, window):
    """the literal form of problem p, computed once per module"""
    if (p, window) not in rig.models:
        rig.models[(p, window)] = rig.model(p, window)
    return rig.models[(p, window)]


def compare(res, m, tag, prev=True):
    for k in RI.OUT_KEYS + (("prev_out",) if prev else ()):
        a, b = res[k], m[k]
        if np.isscalar(a):
            assert int(a) == int(b), (tag, k, a, b)
        else:
            assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), (tag, k, np.nonzero(np.asarray(a).reshape(len(a), -1) != np.asarray(b).reshape(len(a), -1))[0][:8])
    n = len(res["matches21"])
    assert np.all((res["claim_idx"] >= -1) & (res["claim_idx"] < n)) and np.all((res["matches12"] >= -1) & (res["matches12"] < n))


def report(tag, res, hdr, m=None):
    print(f"{tag}: statuses {np.bincount(res['status'], minlength=4).tolist()}, tested {int(res['n_tested'].sum())} of {int(res['n_window'].sum())} window members, "
          f"matches {res['n_matches']}, retracted {int(((res['claim_idx'] >= 0) & (res['matches12'] < 0)).sum())}; resolver rounds {int(hdr[0])}, full re-searches {int(hdr[1])}, "
          f"lists that ran out {int(hdr[2])}, K {int(hdr[3])}" + (f"; queries with more than K blocked ahead {int((m['blocked_ahead'] > hdr[3]).sum())}" if m else ""))


@pytest.mark.parametrize("window", [100.0, 10.0])
def test_one_problem_against_the_literal_form(rig, window):
    res, _, hdr = rig.run(1, window)
    m = model(rig, 0, window)
    report(f"nf 1000 window {window}", res[0], hdr[0], m)
    compare(res[0], m, window)
    assert hdr[0][3] == rig.K
    if window == 100.0:
        assert hdr[0][0] >= RI.DEPTH_MIN and hdr[0][2] >= 1            # the depth tests/test_init_ref.py asserts of this scene; a list ran out


def test_4096_features(rig4096):
    res, _, hdr = rig4096.run(1, 100.0)
    m = rig4096.model(0, 100.0)
    report("nf 4096 window 100", res[0], hdr[0], m)
    compare(res[0], m, "4096")
    assert hdr[0][0] >= RI.DEPTH_MIN and hdr[0][2] >= 1


def test_three_problems_with_their_own_centres(rig):
    res, _, hdr = rig.run(3, 100.0)
    for p in range(3):
        report(f"B=3 problem {p}", res[p], hdr[p])
        compare(res[p], model(rig, p, 100.0), ("B=3", p))
    assert res[0]["matches12"].tobytes() != res[1]["matches12"].tobytes()


def test_in_place_prev_out_equals_out_of_place_and_runs_repeat(rig):
    a, raw_a, hdr_a = rig.run(1, 100.0, fill=0x00)
    b, raw_b, hdr_b = rig.run(1, 100.0, fill=0xFF)
    assert raw_a.tobytes() == raw_b.tobytes() and np.array_equal(hdr_a, hdr_b)         # two runs, whatever the workspace held: identical bytes
    c, _, _ = rig.run(1, 100.0, in_place=True)
    for k in RI.OUT_KEYS + ("prev_out",):
        assert np.ascontiguousarray(a[0][k]).tobytes() == np.ascontiguousarray(c[0][k]).tobytes() if not np.isscalar(a[0][k]) else a[0][k] == c[0][k], k
    assert int((a[0]["matches12"] >= 0).sum()) > 0 and a[0]["prev_out"].tobytes() != rig.pm.tobytes()
    d, _, _ = rig.run(1, 100.0, prev_out=False)                                        # without target_xy / prev_out
    compare(d[0], model(rig, 0, 100.0), "no prev_out", prev=False)


def test_query_flags_leave_slots_out(rig):
    """the padding slots of frame 0 (and a seeded tenth of the others) cleared: INACTIVE with zeros, and the rest is the loop without them"""
    flags = (rig.valid1 & (np.random.RandomState(5).rand(rig.nf) >= 0.1)).astype(np.uint8) * 3          # (bit1 is ignored)
    res, _, hdr = rig.run(1, 100.0, flags=flags)
    m = rig.model(0, 100.0, flags=flags)
    report("flags", res[0], hdr[0])
    compare(res[0], m, "flags")
    off = flags == 0
    assert off.sum() >= 50 and np.all(res[0]["status"][off] == RI.INACTIVE) and np.all(res[0]["n_window"][off] == 0) and np.all(res[0]["claim_idx"][off] == -1)
    assert res[0]["prev_out"][off].tobytes() == rig.pm[off].tobytes()


def test_host_form_against_the_device_form(rig):
    dev, _, _ = rig.run(1, 100.0)
    k = rig.kps(1)
    for in_place in (False, True):
        h = rig.ctx.init_search(rig.q, rig.pm, k, rig.bounds, rig.tg, window=100.0, in_place=in_place)
        compare(h, dev[0], ("host", in_place))
    h = rig.ctx.init_search(rig.q, rig.pm, k, rig.bounds, rig.tg, window=10.0, query_flags=np.ones(rig.nf, np.uint8))
    compare(h, model(rig, 0, 10.0), "host window 10")


def test_hostile_coordinates_and_rows(rig):
    """NaN / Inf / 1e30 in window centres, query rows and target rows: every output matches the restatement, no index is out of range, a query
    whose row or centre is not finite matches nothing, and guard bytes are intact (InitRig.run checks them)"""
    vals = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 3.4e38], F)
    q, pm, tg = rig.q.copy(), rig.pm.copy(), rig.tg.copy()
    nf = rig.nf
    for j in range(nf // 5):
        v = vals[j % len(vals)]
        if j % 3 == 0:
            q[5 * j + 1, (7 * j) % 64] = v
        elif j % 3 == 1:
            pm[5 * j + 1, j % 2] = v
        else:
            tg[5 * j + 1, (11 * j) % 64] = v
    res, _, hdr = rig.run(1, 100.0, q=q, pm=pm, tg=tg)
    m = rig.model(0, 100.0, q=q, pm=pm, tg=tg)
    report("hostile", res[0], hdr[0])
    compare(res[0], m, "hostile")
    badq = ~np.isfinite(q).all(1) | (np.abs(q).max(1) > 1e20) | ~np.isfinite(pm).all(1)
    badt = ~np.isfinite(tg).all(1) | (np.abs(tg).max(1) > 1e20)
    assert badq.sum() >= 100 and badt.sum() >= 50
    assert np.all(res[0]["status"][badq] != RI.MATCHED) and np.all(res[0]["matches21"][badt] == -1) and np.all(res[0]["matched_distance"][badt] == NONE)
    assert np.all(res[0]["n_window"][~np.isfinite(pm).all(1)] == 0)


def test_16384_by_16384_runs_the_large_lds_path(rig, oracle_mod):
    """random keypoints and rows, no extraction; window 6 keeps the restatement cheap.  head[nt] + next[nq] are 128 KB of LDS here"""
    n = capi.GRID_MAX_N
    rng = np.random.RandomState(77)
    bounds = (0.0, 0.0, 640.0, 480.0)
    kp = np.zeros(n, capi.KP_DTYPE)
    kp["x"] = rng.uniform(1, 639, n).astype(F); kp["y"] = rng.uniform(1, 479, n).astype(F)
    tg = (rng.randn(n, 64) * 0.05).astype(F)
    src = rng.randint(n, size=n)                                                       # several queries draw the same keypoint
    noise = rng.randn(n, 64); noise /= np.linalg.norm(noise, axis=1, keepdims=True)
    q = (tg[src] + noise * np.sqrt(rng.uniform(0, 110, (n, 1)) / 512.0)).astype(F)
    pm = np.stack([kp["x"][src] + rng.uniform(-3, 3, n), kp["y"][src] + rng.uniform(-3, 3, n)], 1).astype(F)
    ctx = rig.ctx
    dk = capi.DeviceBuffer(kp.nbytes).upload(kp)
    dg = ctx.grid_build_device(dk.ptr, n, bounds)
    txy = np.stack([kp["x"], kp["y"]], 1).astype(F)
    bufs = [capi.DeviceBuffer(a.nbytes).upload(a) for a in (q, pm, tg, txy)]
    lay = Context.init_search_layout(1, n, n, GUARD)
    out = guarded.outputs(lay)
    ws = capi.DeviceBuffer(Context.init_search_workspace_bytes(n, n, 1))
    ctx.init_search_device(1, n, bufs[0].ptr, bufs[1].ptr, dg.ptr, bufs[2].ptr, 0, n, ws.ptr, out.ptr, window=6.0, d_target_xy=bufs[3].ptr, guard=GUARD)
    ctx.synchronize()
    res = guarded.problems(lay.parse(guarded.download(out, lay)), 1)[0]
    hdr = ws.download(np.int32, 4)
    x, y = kp["x"].copy(), kp["y"].copy()
    m = RI.literal(oracle_mod, q, pm, 6.0, RW.build(x, y, bounds), x, y, bounds, tg, txy=txy)
    report("16384 x 16384 window 6", res, hdr, m)
    compare(res, m, "16384")
    assert res["n_matches"] >= n // 8 and int(m["retractions"]) >= 16
    for b in bufs + [dk, dg, out, ws]:
        b.free()


def test_invalid_arguments_launch_nothing(rig):
    L, ctx, nf = rig.L, rig.ctx, rig.nf
    lay = Context.init_search_layout(1, nf, nf)
    sent = np.full(lay["bytes"], 0xA5, np.uint8)
    out = capi.DeviceBuffer(lay["bytes"]).upload(sent)
    mk = lambda a: capi.DeviceBuffer(np.ascontiguousarray(a).nbytes + 16).upload(a)
    qd, pm, fl, txy = (mk(a) for a in (rig.q, rig.pm, np.ones(nf, np.uint8), rig.xy[1]))
    ws = capi.DeviceBuffer(Context.init_search_workspace_bytes(nf, nf, 1))
    names = ("st",) + Context.INIT_OUT_Q + Context.INIT_OUT_T + ("nm",)
    keys = ("status",) + Context.INIT_OUT_Q + Context.INIT_OUT_T + ("n_matches",)
    base = dict(ctx=ctx.h, B=1, nq=nf, qd=qd.ptr, pm=pm.ptr, fl=fl.ptr, window=100.0, grids=rig.dgrid, tg=rig.dtg.ptr, tstride=0, txy=txy.ptr, nt=nf, low=100, ratio=0.9,
                ws=ws.ptr, **{n: out.ptr + lay[k] for n, k in zip(names, keys)}, po=out.ptr + lay["prev_out"])

    def call(**kw):
        a = dict(base); a.update(kw)
        return L.xfh_init_search_device(*[a[k] for k in base])

    nan, inf = float("nan"), float("inf")
    bad = [dict(ctx=None), dict(B=0), dict(B=-1), dict(B=65536), dict(nq=0), dict(nq=-1), dict(nq=capi.GRID_MAX_N + 1), dict(nt=0), dict(nt=capi.GRID_MAX_N + 1),
           dict(window=nan), dict(window=inf), dict(window=-inf), dict(ratio=nan), dict(ratio=inf), dict(ratio=-0.5), dict(low=-1), dict(txy=None), dict(po=None),
           dict(qd=None), dict(pm=None), dict(grids=None), dict(tg=None), dict(ws=None), dict(qd=qd.ptr + 4), dict(tg=base["tg"] + 8), dict(tstride=4), dict(tstride=260),
           dict(grids=base["grids"] + 8), dict(ws=ws.ptr + 8), dict(pm=pm.ptr + 2), dict(txy=txy.ptr + 1), dict(po=base["po"] + 2)]
    bad += [{n: None} for n in names] + [{n: base[n] + 2} for n in names[1:]]
    ctx.synchronize()
    ctx.timing_enable(capi.K["INIT_CANDIDATES"])
    for kw in bad:
        assert call(**kw) == 1, kw
    ctx.synchronize()
    assert ctx.timing_read()[0] == 0 and np.array_equal(out.download(np.uint8, lay["bytes"]), sent)
    # the valid calls still work afterwards
    assert call() == 0 and call(fl=None) == 0 and call(txy=None, po=None) == 0 and call(window=-1.0) == 0 and call(ratio=0.0, low=0) == 0 and call(po=pm.ptr) == 0
    ctx.synchronize()
    assert ctx.timing_read()[0] == 6 and not np.array_equal(out.download(np.uint8, lay["bytes"]), sent)
    ctx.timing_enable(capi.K["NONE"])
    # the host form refuses the same classes before it stages or launches anything
    k = rig.kps(1)
    gb = capi.GridBounds(*rig.bounds)
    hq, hp, ht = np.ascontiguousarray(rig.q), np.ascontiguousarray(rig.pm), np.ascontiguousarray(rig.tg)
    ho = {n: np.full(nf * 4, 0xA5, np.uint8) for n in names}
    hb = dict(ctx=ctx.h, nq=nf, qd=hq.ctypes.data, pm=hp.ctypes.data, fl=None, window=100.0, kps=k.ctypes.data, b=C.byref(gb), tg=ht.ctypes.data, nt=nf, low=100, ratio=0.9,
              **{n: a.ctypes.data for n, a in ho.items()}, po=None)

    def hcall(**kw):
        a = dict(hb); a.update(kw)
        return L.xfh_init_search(*[a[n] for n in hb])

    badb = [capi.GridBounds(*b) for b in ((0, 0, 0, 480), (0, 480, 640, 0), (nan, 0, 640, 480), (0, 0, inf, 480))]
    hbad = [dict(ctx=None), dict(nq=0), dict(nq=capi.GRID_MAX_N + 1), dict(nt=0), dict(nt=capi.GRID_MAX_N + 1), dict(window=nan), dict(window=inf), dict(ratio=nan), dict(ratio=-1.0),
            dict(low=-1), dict(qd=None), dict(pm=None), dict(kps=None), dict(tg=None), dict(b=None)] + [{n: None} for n in names] + [dict(b=C.byref(x)) for x in badb]
    ctx.timing_enable(capi.K["GRID_BUILD"])
    for kw in hbad:
        assert hcall(**kw) == 1, kw
    assert ctx.timing_read()[0] == 0 and all(np.all(a == 0xA5) for a in ho.values())
    assert hcall() == 0
    assert ctx.timing_read()[0] == 1 and not any(np.all(a[:nf] == 0xA5) for a in ho.values())
    ctx.timing_enable(capi.K["NONE"])
    for x in (out, qd, pm, fl, txy, ws):
        x.free()
