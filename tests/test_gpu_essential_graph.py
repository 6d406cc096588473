"""xfh_essential_graph_device on the scenes of tests/essential_graph_rig.py through the guarded run (tests/guarded.py) against the Python rule
(tests/ref_essential_graph.py).

Equal to the rule: the whole header (status, free vertices, valid edges, kind-0 edges, iterations, trials, rejected trials, factorisation failures,
corrected points).  Within EG_TOL -- twice the spread of the float64 forms among themselves, measured on the CPU with nothing from the device in it:
Tcw_out, Sim3_out, points_out, chi2 and final_chi2; a NaN stands for a NaN.  Every scene passed the fairness condition on the CPU
(tests/test_essential_graph_ref.py::test_fairness_of_the_rig).  The scenes reach 1, 2, 9, 10 (63 and 70 unknowns around the 64-wide tile), 19, 37 and 128
free vertices; a chain with one loop edge between its ends; a kind-0 and a kind-1 edge between the same pair; vertices of 0, 1, 255, 256 and 257 edges (the
fold); a fixed vertex in the middle of the order; bFixScale on and off with a corrected scale of 1.3; corrected and non-corrected entries for only some
vertices; edges and point references out of range; a start far off; max_iterations of 1 and 3; the early statuses; a NaN pose entry.  write_back changes
the tables only in the rows the rule names; the host-pointer form gives the device form's bytes."""
import numpy as np
import pytest

import essential_graph_rig as G
import ref_essential_graph as R
from xfeatslam_amd import capi, essential_graph as EG

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64
ALL = list(G.SCENES) + list(G.EARLY) + list(G.LIMIT) + list(G.FAILING)


@pytest.fixture(scope="module")
def rig():
    r = G.EgRig(capi.lib())
    yield r
    r.close()


def check(got, ref, tag):
    print(f"{tag}: device {dict(zip(R.H_KEYS, np.asarray(got['header']).tolist()))}  distances {G.distances(got, ref)}")
    bad = G.outputs_agree(got, ref)
    assert bad == [], (tag, bad)


@pytest.mark.parametrize("name", ALL)
def test_scene_against_the_rule(rig, name):
    p = G.scene(name)
    ref = G.rule_of(name)
    got, raw = rig.run(p)
    check(got, ref, name)
    # without write_back both tables keep their bits
    assert np.array_equal(got["pose_table"].view(np.uint32), np.asarray(p["pose_table"], F).view(np.uint32))
    assert np.array_equal(got["point_table"].view(np.uint32), np.asarray(p["point_table"], F).view(np.uint32))
    # a fixed vertex's estimate is its vScw, by bits
    fixed = np.asarray(p["kf_fixed"]) != 0
    vS = np.array(R.Plan(p).vScw, D)
    assert G.same_bits(dict(x=got["Sim3_out"][fixed]), dict(x=vS[fixed]), names=("x",)) == []
    # two runs, whatever the buffers held: identical bytes
    again, raw2 = rig.run(p, fill=0x5A, ws_fill=0xC3)
    assert raw.tobytes() == raw2.tobytes(), name
    # write_back: the same outputs, and the tables hold them in the rows the rule names; every other row is untouched
    wb, raw3 = rig.run(p, write_back=True)
    assert raw.tobytes() == raw3.tobytes(), name
    T, X = np.asarray(p["pose_table"], F).copy(), np.asarray(p["point_table"], F).copy()
    row_ok = (p["kf_row"] >= 0) & (p["kf_row"] < len(T))
    T[p["kf_row"][row_ok]] = got["Tcw_out"][row_ok]
    pr, pf = np.asarray(p["point_row"]), np.asarray(p["point_ref"])
    corrected = (pr >= 0) & (pr < len(X)) & (pf >= 0) & (pf < len(p["kf_row"]))
    X[pr[corrected]] = got["points_out"][corrected]
    assert got["header"][8] == int(corrected.sum())
    assert G.same_bits(dict(T=wb["pose_table"], X=wb["point_table"]), dict(T=T, X=X), names=("T", "X")) == [], name
    assert np.array_equal(got["points_out"][~corrected & (pr >= 0) & (pr < len(X))], np.asarray(p["point_table"], F)[pr[~corrected & (pr >= 0) & (pr < len(X))]])


def test_host_pointer_form_and_wrapper(rig):
    p = G.scene("out_of_range")
    dev, _ = rig.run(p, write_back=True)
    r = EG.essential_graph(rig.ctx, *[p[k] for k, _ in EG.INPUTS], fix_scale=p["fix_scale"], max_iterations=p["max_iterations"], write_back=True)
    assert list(r["header"].values()) == dev["header"].tolist() and r["final_chi2"] == dev["final_chi2"]
    for k in ("Sim3_out", "Tcw_out", "points_out", "chi2", "pose_table", "point_table"):
        assert np.array_equal(np.asarray(r[k]).reshape(-1).view(np.uint8), np.asarray(dev[k]).reshape(-1).view(np.uint8)), k
    nV, nE, nP, nS = G.dims(p)
    assert EG.workspace_bytes(nV, nE, G.n_free_of(p)) == rig.L.xfh_essential_graph_workspace_bytes(nV, nE, G.n_free_of(p)) > 0


def test_free_count_mismatch(rig):
    p = G.scene("two_free")
    got, _ = rig.run(p, n_free=1, write_back=True)
    assert got["header"][0] == R.FREE_MISMATCH and got["header"][1] == 2 and not got["chi2"].any() and got["final_chi2"] == 0.0
    assert np.array_equal(got["pose_table"].view(np.uint32), np.asarray(p["pose_table"], F).view(np.uint32))
    assert G.same_bits(got, G.run_host(p, n_free=1)) == []


def hostile(seed):
    """NaN, Inf and 1e30 in poses, points and similarities; indices, rows, kinds and flags hold anything"""
    p = dict(G.make(100 + seed, 5, n_points=20))
    rng = np.random.RandomState(seed)
    bad = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0, 1e-30])
    for k in ("pose_table", "point_table", "sim3"):
        a = np.asarray(p[k]).copy()
        m = rng.rand(*a.shape) < 0.15
        a[m] = rng.choice(bad, int(m.sum())).astype(a.dtype)
        p[k] = a
    if seed % 2:
        for k, lo, hi in (("kf_row", -3, 12), ("point_row", -5, 40), ("point_ref", -4, 12), ("edge_i", -2, 9), ("edge_j", -2, 9), ("edge_kind", -3, 4),
                          ("corrected_index", -3, 9), ("noncorrected_index", -3, 9)):
            a = np.asarray(p[k]).copy()
            m = rng.rand(len(a)) < 0.25
            a[m] = rng.randint(lo, hi, int(m.sum()))
            p[k] = a.astype(np.int32)
        p["edge_i"][:2] = [2 ** 31 - 1, -2 ** 31]
    return p


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_hostile_input_returns(rig, seed):
    """the call returns, the guards hold, and what does not depend on floating point -- the plan's counts -- equals the host form's"""
    p = hostile(seed)
    got, _ = rig.run(p, write_back=True)
    host = G.run_host(p, write_back=True)
    assert got["header"][:4].tolist() == host["header"][:4].tolist() and got["header"][8] == host["header"][8], (got["header"], host["header"])
    h = got["header"]
    assert 0 <= h[4] <= 20 and h[4] <= h[5] <= 200 and 0 <= h[6] <= h[5] and 0 <= h[7] <= h[5]


def test_refusals_before_any_launch(rig):
    L, p = rig.L, G.scene("one_free")
    nV, nE, nP, nS = G.dims(p)
    a = EG.host_arrays(p)
    dev = [capi.DeviceBuffer(x.nbytes + 16).upload(x) for x in a]
    lay = EG.essential_graph_layout(nV, nP, nE)
    out, ws = capi.DeviceBuffer(lay["bytes"]), capi.DeviceBuffer(int(L.xfh_essential_graph_workspace_bytes(nV, nE, 1)))

    def call(nV=nV, nf=1, nE=nE, nP=nP, nS=nS, its=2, wb=0, fs=0, wsp=ws.ptr, ctx=rig.ctx.h):
        return L.xfh_essential_graph_device(ctx, nV, nf, nE, nP, nS, dev[0].ptr, len(a[0]), dev[1].ptr, len(a[1]), *[d.ptr for d in dev[2:]], fs, its, wb, wsp,
                                            *[out.ptr + lay[k] for k in EG.NAMES])

    assert call() == 0
    assert call(nf=EG.MAX_FREE + 1, nV=2000) == 1 and call(nf=-1) == 1 and call(nf=nV + 1) == 1
    for kw in (dict(nV=0), dict(nE=0), dict(nP=0), dict(nS=0), dict(its=0), dict(its=21), dict(wb=2), dict(fs=-1), dict(wsp=None), dict(wsp=ws.ptr + 8), dict(ctx=None)):
        assert call(**kw) == 1, kw
    for d in dev + [out, ws]:
        d.free()
