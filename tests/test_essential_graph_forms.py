"""The spread of the float64 forms of OptimizeEssentialGraph among themselves on the rig's scenes: the literal form (tests/ref_essential_graph_literal.py:
g2o's lines one by one, numpy's products and solvers), the rule (tests/ref_essential_graph.py), the rule with its libm results moved by one ulp under three
seeds, and the library's host form -- for Tcw_out, Sim3_out, points_out, chi2 and final_chi2.  EG_TOL of tests/essential_graph_rig.py is twice that spread.
Nothing from the device enters.  CPU only."""
import numpy as np

import essential_graph_rig as G


def test_spread_of_the_forms():
    """this test fails if it sees more than half of a constant of EG_TOL, or if a form decides otherwise than the others (the fairness condition)"""
    worst, where = dict.fromkeys(G.Tol._fields, 0.0), {}
    for name in list(G.SCENES) + list(G.LIMIT):
        forms = G.forms_of(name)
        assert all(np.array_equal(f["header"], forms[0]["header"]) for f in forms), (name, [f["header"].tolist() for f in forms])
        for k, v in G.spread(forms).items():
            if v > worst[k]:
                worst[k], where[k] = v, name
    print("spread of the forms: %s at %s" % (worst, where))
    for k in G.Tol._fields:
        tol = getattr(G.EG_TOL, k)
        assert worst[k] <= tol / 2, (k, worst[k], where.get(k), tol)
        assert worst[k] >= tol / 2.2, (k, worst[k], tol)                     # and the constant is the measured one, not a wider one
