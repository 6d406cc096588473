"""The rule of xfh_local_ba_device (tests/ref_local_ba.py) against the literal form (tests/ref_local_ba_literal.py: vertex and edge objects, sequential
sums in g2o's order, push / pop, numpy.linalg for the point blocks and the reduced system) on the rig's scenes, those of failing factorisations
included -- every decision equal -- and the spread
of the float64 forms among themselves (literal, rule, rule with jittered libm under three seeds, the library's host form), from which LBA_TOL of
tests/local_ba_rig.py is taken.  Nothing from the device enters.  CPU only."""
import numpy as np
import pytest

import local_ba_rig as G

STREAM = 200


@pytest.mark.parametrize("name", list(G.SCENES) + list(G.EARLY) + list(G.LIMIT) + list(G.FAILING))
def test_rule_against_literal(name):
    """every erase flag, the status and the counts, and every accept / reject of every trial in every iteration, equal"""
    lit, rule = G.forms_of(name)[:2]
    assert G.decisions_differ(lit, rule) == [], (name, lit["header"], rule["header"])
    assert lit["events"] == rule["events"], name
    d = G.distances(lit, rule)
    assert all(d[k] <= getattr(G.LBA_TOL, k) for k in d), (name, d)


def test_spread_of_the_forms():
    """LBA_TOL is twice the largest spread seen on the rig's scenes and on the random small scenes whose forms all decide alike (a scene that has
    converged to rounding noise may flip a trial between two forms; its outputs then differ by that trial, which no tolerance is about), not below
    1 float step and 1e-13 relative; this test fails if it sees more than half of a constant."""
    worst, where, used = dict.fromkeys(G.Tol._fields, 0.0), {}, 0
    for name in list(G.SCENES) + list(G.LIMIT) + list(range(STREAM)):
        forms = G.forms_of(name)
        if not isinstance(name, str) and any(f["events"] != forms[1]["events"] for f in forms[:5]):
            continue
        used += 1
        for k, v in G.spread(forms).items():
            if v > worst[k]:
                worst[k], where[k] = v, name
    print("spread of the forms over %d scenes: %s at %s" % (used, worst, where))
    assert used >= len(G.SCENES) + STREAM * 3 // 4
    for k in G.Tol._fields:
        tol = getattr(G.LBA_TOL, k)
        assert worst[k] <= tol / 2, (k, worst[k], where.get(k), tol)
        assert tol >= (1e-13 if k == "final" else 1.0), (k, tol)
