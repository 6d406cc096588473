"""The rule of xfh_mlpnp_solve_device (tests/ref_mlpnp.py) against the literal form of tests/ref_mlpnp_literal.py -- the reference's solver object with
its members, LAPACK's SVD / eigh, a pivoted LDL^T, pow(x, 1 / 3), the SVD null space of the bearing vector and a Jacobian derived on its own -- on
the scenes of tests/mlpnp_rig.py and on 200 random well-posed scenes (0.5 px of noise, 30 % wrong matches).

Two literal forms are held.  (1) With Refine's result stored into mRi / mti, which is what the rule states: every decision equal (status, winning
iteration, nInliers, every flag), the pose within 4x the deviation recorded in profiles/mlpnp.md (tools/time_mlpnp.py --forms) and never less than
one float32 step of the entry, the precision of the format both forms round to.  Scenes where the two least eigenvalues of A^T A of the REPORTED
solve are within 1e-6 relative are exempt from the value comparison only; at most 2 % of the random scenes.  (2) The reference AS WRITTEN: its
Refine() never copies the re-solved pose into mRi / mti (src/MLPnPsolver.cpp:325-334), so it counts and reports the pose of the iteration that called
it.  That is the stated deviation of the rule's step 7; the test holds the as-written form against exactly that prediction made from the rule's own
iterations -- the winner is the first qualifying iteration whose OWN count exceeds min_inliers_eff, with that iteration's pose and flags -- and
prints how often the two differ."""
import numpy as np
import pytest

import mlpnp_rig as G
import ref_mlpnp as R

F = np.float32
RECORDED_ROT, RECORDED_TR = 0.0, 0.0          # profiles/mlpnp.md, "Forms": the largest |Tcw rule - Tcw literal| over the 200 random scenes
EPS_OF = dict(its5=0.85, its70=0.4)


def pose_close(a, b):
    a, b = np.asarray(a, F).reshape(3, 4), np.asarray(b, F).reshape(3, 4)
    step = np.maximum(np.spacing(np.abs(a)), np.spacing(np.abs(b))).astype(np.float64)
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    tol = np.maximum(step, 4 * np.array([[RECORDED_ROT] * 3 + [RECORDED_TR]] * 3))
    return bool(np.all(d <= tol)), float(d[:, :3].max()), float(d[:, 3].max())


def same_decisions(r, o, name):
    h = dict(zip(R.HEADER, r["header"].tolist()))
    want = (h["status"] in (R.REFINED, R.BEST), h["status"] != R.REFINED, h["n_inliers"], h["winner"])
    assert (o["ret"], o["bNoMore"], o["nInliers"], o["at"]) == want, (name, h, {k: o[k] for k in ("ret", "bNoMore", "nInliers", "at")})
    if r["inliers"] is not None:
        assert np.array_equal(o["vbInliers"], r["inliers"]), name


def as_written_prediction(r, s, b=0):
    """what the reference as written returns, from the rule's own iterations: (ret, bNoMore, nInliers, at, pose, flags)"""
    h = dict(zip(R.HEADER, r["header"].tolist()))
    best = -1
    for k, c in enumerate(r["counts"]):
        if c < h["min_inliers"]:
            continue
        if best < 0 or c > r["counts"][best]:
            best = k
        if c > h["min_inliers"]:
            return True, False, c, k, k
    if best >= 0:
        return True, True, r["counts"][best], -1, best
    return False, True, 0, -1, None


@pytest.fixture(scope="module")
def cases():
    s = G.rig()
    out = [(n, sc, 0, EPS_OF.get(n, 0.5)) for n, sc in s.items()] + [("family%d" % b, G.family(), b, 0.5) for b in range(3)]
    return out + [("random%d" % k, sc, 0, 0.5) for k, sc in enumerate(G.random_scenes())]


def test_rule_equals_the_literal_form_with_the_refined_pose_stored(cases):
    exempt = compared = n_random = 0
    worst = [0.0, 0.0]
    for name, sc, b, eps in cases:
        r, o = G.rule_of(sc, b), G.literal_of(sc, b, True, eps).iterate(sc["chunk"])
        same_decisions(r, o, name)
        n_random += name.startswith("random")
        if r["Tcw"] is None:
            continue
        if o["gap"] < 1e-6:
            exempt += name.startswith("random")
            continue
        ok, dr, dt = pose_close(r["Tcw"], o["Tcw"])
        worst = [max(worst[0], dr), max(worst[1], dt)]
        compared += 1
        assert ok, (name, dr, dt)
    print(f"poses compared {compared}, largest |Tcw rule - Tcw literal|: rotation {worst[0]:.3g}, translation {worst[1]:.3g}; exempt {exempt} of {n_random} random scenes "
          f"({100.0 * exempt / n_random:.1f} %)")
    assert n_random == 200 and exempt <= 0.02 * n_random and compared > 100


def test_reference_as_written_reports_the_calling_iterations_pose(cases):
    """the stated deviation of step 7, pinned: the as-written form equals the prediction made from the rule's iterations, and differs from the rule in
    the share of scenes printed"""
    differ = total = 0
    for name, sc, b, eps in cases:
        r, o = G.rule_of(sc, b), G.literal_of(sc, b, False, eps).iterate(sc["chunk"])
        if r["header"][1] == R.TOO_FEW:
            assert not o["ret"] and o["bNoMore"]
            continue
        ret, no_more, n_inl, at, k = as_written_prediction(r, sc, b)
        assert (o["ret"], o["bNoMore"], o["nInliers"], o["at"]) == (ret, no_more, n_inl, at), (name, o["at"], o["nInliers"], at, n_inl)
        if k is not None:
            Rt = r["hyps"][k][0]
            assert pose_close(np.array(Rt, np.float64).astype(F), o["Tcw"])[0], name
            assert int(o["vbInliers"].sum()) == r["counts"][k]
        total += 1
        h = r["header"]
        differ += not (at == h[4] and n_inl == h[5] and (r["inliers"] is None or np.array_equal(o["vbInliers"], r["inliers"])))
    print(f"the reference as written differs from the rule (winner, nInliers or a flag) in {differ} of {total} scenes")
    assert differ > 0
