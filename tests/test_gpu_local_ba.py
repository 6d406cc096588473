"""xfh_local_ba_device on the scenes of tests/local_ba_rig.py through the guarded run (tests/guarded.py) against the Python rule (tests/ref_local_ba.py).

Equal to the rule: every erase flag and the whole header (status, counts, iterations, trials, rejected trials, factorisation failures, edges to erase).
Within LBA_TOL -- the spread of the float64 forms among themselves, measured on the CPU with nothing from the device in it: Tcw_out, points_out, chi2
and final_chi2.  The scenes reach 1, 2, 11, 22 and 128 free keyframes (the factorisation has no tile: one workgroup of 1024 lanes strides over the
trailing matrix, which 11 free keyframes already cross; 128 is the refusal limit and S's full 768 x 768), keyframes of 0, 1, 255, 256 and 257 edges
(the 256-lane fold), points seen once, twice and by every keyframe, a point without an edge, edge indices out of range, the initial keyframe fixed
inside the local set, a start far from the optimum (rejected trials), gross outliers and a point that ends behind a camera; chi2 folds over 266 and
300 keyframes (a second step of the fold's stride), keyframes of 400 to 520 edges (a second and a third pass of the 256 lanes, whole waves of them),
nK as the largest of (nK, nP, nE), max_iterations of 1 and 3, and information weights of 1 / 1.44 and 4.  G.FAILING: a NaN observation at a free and at a
fixed keyframe and a NaN point -- all 100 factorisations fail, x stays zero, the header says so and every flag is the rule's -- and an Inf observation,
after which no factorisation fails while b_S is NaN; their numbers are compared NaN for NaN.  No test asserts the device's trajectory of lambda."""
import ctypes as C

import numpy as np
import pytest

import local_ba_rig as G
import ref_local_ba as R
from xfeatslam_amd import capi, local_ba

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64
INVALID = 1
ALL = list(G.SCENES) + list(G.EARLY) + list(G.LIMIT) + list(G.FAILING)


@pytest.fixture(scope="module")
def rig():
    r = G.LbaRig(capi.lib())
    yield r
    r.close()


def check(got, ref, tag):
    print(f"{tag}: device {dict(zip(R.H_KEYS, np.asarray(got['header']).tolist()))}  distances {G.distances(got, ref)}")
    bad = G.outputs_agree(got, ref)
    assert bad == [], (tag, bad)


@pytest.mark.parametrize("name", ALL)
def test_scene_against_the_rule(rig, name):
    p = G.scene(name)
    got, raw = rig.run(p)
    check(got, G.rule_of(name), name)
    # a fixed keyframe's output is its input, by bits; so are both tables without write_back
    fixed = np.asarray(p["kf_fixed"]) != 0
    assert np.array_equal(got["Tcw_out"][fixed].view(np.uint32), np.asarray(p["pose_table"], F)[p["kf_row"]][fixed].view(np.uint32))
    assert np.array_equal(got["pose_table"].view(np.uint32), np.asarray(p["pose_table"], F).view(np.uint32))
    assert np.array_equal(got["point_table"].view(np.uint32), np.asarray(p["point_table"], F).view(np.uint32))
    # two runs, whatever the buffers held: identical bytes
    again, raw2 = rig.run(p, fill=0x5A, ws_fill=0xC3)
    assert raw.tobytes() == raw2.tobytes(), name
    # write_back: the same outputs, and the tables hold them where a free keyframe or a point with an edge has its row; every other row is untouched
    wb, raw3 = rig.run(p, write_back=True)
    assert raw.tobytes() == raw3.tobytes(), name
    T, X = np.asarray(p["pose_table"], F).copy(), np.asarray(p["point_table"], F).copy()
    if got["header"][0] == R.OK:
        T[p["kf_row"][~fixed]] = got["Tcw_out"][~fixed]
        seen = np.zeros(len(p["point_row"]), bool)
        b, kf = np.asarray(p["edge_begin"]), np.asarray(p["edge_kf"])
        for q in range(len(seen)):
            seen[q] = np.any((kf[b[q]:b[q + 1]] >= 0) & (kf[b[q]:b[q + 1]] < len(fixed)))
        X[p["point_row"][seen]] = got["points_out"][seen]
    assert np.array_equal(wb["pose_table"].view(np.uint32), T.view(np.uint32)) and np.array_equal(wb["point_table"].view(np.uint32), X.view(np.uint32))


def test_host_pointer_form_and_wrapper(rig):
    p = G.scene("outliers")
    dev, _ = rig.run(p, write_back=True)
    r = local_ba.local_ba(rig.ctx, *[p[k] for k, _ in G.INPUTS], G.cam_struct(), write_back=True)
    assert list(r["header"].values()) == dev["header"].tolist() and r["final_chi2"] == dev["final_chi2"]
    for k in ("Tcw_out", "points_out", "erase", "chi2", "pose_table", "point_table"):
        assert np.array_equal(np.asarray(r[k]).reshape(-1).view(np.uint8), np.asarray(dev[k]).reshape(-1).view(np.uint8)), k
    nK, nP, nE = G.dims(p)
    assert local_ba.workspace_bytes(nK, nP, nE, G.n_free_of(p)) == rig.L.xfh_local_ba_workspace_bytes(nK, nP, nE, G.n_free_of(p)) > 0


def test_free_count_mismatch(rig):
    p = G.scene("two_free_mono")
    got, _ = rig.run(p, n_free=1)
    assert got["header"][0] == R.FREE_MISMATCH and got["header"][1] == 2 and not got["erase"].any() and got["final_chi2"] == 0.0
    assert np.array_equal(got["Tcw_out"], np.asarray(p["pose_table"], F)[p["kf_row"]]) and np.array_equal(got["points_out"], np.asarray(p["point_table"], F)[p["point_row"]])


def hostile(seed, level):
    """level 0: NaN, Inf and 1e30 in points, poses and observations; level 1: also indices, rows, flags and the CSR hold anything"""
    p = dict(G.make(100 + seed, 3, 2, 40, 4, "mixed"))
    rng = np.random.RandomState(seed)
    bad = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0, 1e-30], F)
    for k in ("pose_table", "point_table", "edge_obs"):
        a = np.asarray(p[k], F).copy()
        m = rng.rand(*a.shape) < 0.15
        a[m] = rng.choice(bad, int(m.sum()))
        p[k] = a
    if level:
        for k, lo, hi in (("kf_row", -3, 12), ("point_row", -5, 60), ("edge_kf", -2, 9), ("edge_begin", -10, 200)):
            if k == "kf_row" and seed == 2:                                 # (a keyframe whose row is outside the table counts as fixed: FREE_MISMATCH, seed 3)
                continue
            a = np.asarray(p[k]).copy()
            m = rng.rand(len(a)) < 0.2
            a[m] = rng.randint(lo, hi, int(m.sum()))
            p[k] = a.astype(np.int32)
        p["edge_kf"][:3] = [2 ** 31 - 1, -2 ** 31, 7]
    return p


@pytest.mark.parametrize("seed,level", [(0, 0), (1, 0), (2, 1), (3, 1)])
def test_hostile_input_returns(rig, seed, level):
    """the call returns, the guards hold, and what does not depend on floating point -- the plan's counts -- equals the host form's"""
    p = hostile(seed, level)
    nf = G.n_free_of(p)
    got, _ = rig.run(p, write_back=True, n_free=nf)
    host = G.run_host(p, write_back=True, n_free=nf)
    assert got["header"][:5].tolist() == host["header"][:5].tolist(), (got["header"], host["header"])
    h = got["header"]
    assert 0 <= h[5] <= 10 and h[5] <= h[6] <= 100 and 0 <= h[7] <= h[6] and 0 <= h[8] <= h[6] and 0 <= h[9] <= len(p["edge_kf"])


def test_every_refusal(rig):
    L, p = rig.L, G.scene("one_free")
    nK, nP, nE = G.dims(p)
    arrays = [np.ascontiguousarray(np.asarray(p[k], dt)) for k, dt in G.INPUTS]
    dev = [capi.DeviceBuffer(a.nbytes + 16).upload(a) for a in arrays]
    lay = local_ba.local_ba_layout(nK, nP, nE)
    out, ws = capi.DeviceBuffer(lay["bytes"]), capi.DeviceBuffer(int(L.xfh_local_ba_workspace_bytes(nK, nP, nE, 1)))
    cam = G.cam_struct()

    def call(nK=nK, nf=1, nP=nP, nE=nE, rows=(len(arrays[0]), len(arrays[1])), ptrs=None, w=1.0, its=10, wb=0, wsp=ws.ptr, outs=None, cam=C.byref(cam), ctx=rig.ctx.h):
        ptrs = ptrs or [d.ptr for d in dev]
        outs = outs or [out.ptr + lay[k] for k in local_ba.NAMES]
        return L.xfh_local_ba_device(ctx, nK, nf, nP, nE, ptrs[0], rows[0], ptrs[1], rows[1], *ptrs[2:], cam, w, its, wb, wsp, *outs)

    assert call() == 0
    rig.ctx.synchronize()
    assert call(nf=G.local_ba.MAX_FREE + 1, nK=200) == INVALID and call(nf=-1) == INVALID and call(nf=nK + 1) == INVALID
    for kw in (dict(nK=0), dict(nP=0), dict(nE=0), dict(nK=65536), dict(rows=(0, 5)), dict(rows=(5, 0)), dict(its=0), dict(its=11), dict(wb=2), dict(wb=-1)):
        assert call(**kw) == INVALID, kw
    for w in (0.0, -1.0, np.nan, np.inf):
        assert call(w=w) == INVALID, w
    assert call(ctx=None) == INVALID and call(cam=None) == INVALID and call(wsp=None) == INVALID and call(wsp=ws.ptr + 8) == INVALID
    for i in range(len(dev)):
        ptrs = [d.ptr for d in dev]
        ptrs[i] = None
        assert call(ptrs=ptrs) == INVALID, i
        if G.INPUTS[i][1] != np.uint8:
            ptrs[i] = dev[i].ptr + 2
            assert call(ptrs=ptrs) == INVALID, i
    for i, k in enumerate(local_ba.NAMES):
        outs = [out.ptr + lay[n] for n in local_ba.NAMES]
        outs[i] = None
        assert call(outs=outs) == INVALID, k
        if k != "erase":
            outs[i] = out.ptr + lay[k] + (4 if k == "final_chi2" else 2)
            assert call(outs=outs) == INVALID, k
    assert L.xfh_local_ba_workspace_bytes(0, 1, 1, 0) == 0 and L.xfh_local_ba_workspace_bytes(3, 1, 1, 4) == 0 and L.xfh_local_ba_workspace_bytes(200, 1, 1, 129) == 0
    for d in dev + [out, ws]:
        d.free()
