"""The float64 forms of OptimizeSim3 against each other, without a GPU: the literal transcription (tests/ref_optsim3_literal.py) against the kernel's
rule (tests/ref_optsim3.py) and against the library's host form (xfh_sim3_optimize_host, the kernel's own lines on one host thread) on the rig and on
200 random small scenes -- every decision equal -- and the spread of these forms among themselves, from which SIM3OPT_TOL of tests/optsim3_rig.py
is taken."""
import numpy as np

import optsim3_rig as G
import ref_optsim3 as R


def test_rule_against_literal_on_the_rig():
    for name in G.SCENES:
        lit, rule = G.forms_of(name)[:2]
        assert R.same_decisions(lit, rule) == [], (name, R.same_decisions(lit, rule), lit["header"], rule["header"])
        assert R.header_in_bounds(lit["header"]) and R.header_in_bounds(rule["header"]), name
        host = G.host_of(name)
        assert R.same_decisions(lit, host) == [] and R.header_in_bounds(host["header"]), (name, R.same_decisions(lit, host), lit["header"], host["header"])


def test_rule_against_literal_on_random_scenes():
    seen = set()
    for k in range(200):
        forms = G.forms_of(k)
        for f in forms[1:] + [G.host_of(k)]:
            d = R.same_decisions(forms[0], f)
            assert d == [], (k, d, forms[0]["header"], f["header"])
        h = forms[1]["header"]
        seen.add((int(h[5]), int(h[7])))
    assert seen >= {(5, 2), (10, 2)}, seen                                # n_more of 5 and of 10 both reached round 2


def test_spread_of_the_reference():
    """How far the float64 forms lie from each other -- the literal, the rule, the rule with exp / sin / cos / sqrt moved by one double step under
    three seeds, the library's host form -- in every output SIM3OPT_TOL names, on the rig's scenes and on the 200 stream scenes.  Nothing from the device enters.
    SIM3OPT_TOL is twice the largest value seen (the factor keeps one scene's rounding luck from deciding), not below 1 float step and 1e-13
    relative; this test fails if it sees more than half of a constant.  The numeric Jacobian is why the spread is what it is: a central difference
    over 2e-9 carries the rounding of its two errors, about 1e-7 relative in an entry, so two correct evaluations converge to estimates about
    1e-8 apart, and a chi2 that the first classification read at a rejected trial differs by that trial's own noise."""
    worst = dict.fromkeys(R.Tol._fields, 0.0)
    where = dict.fromkeys(R.Tol._fields, None)
    for name in list(G.SCENES) + list(range(200)):
        for k, v in G.spread(G.forms_of(name) + [G.host_of(name)]).items():
            if v > worst[k]:
                worst[k], where[k] = v, name
    print("spread of the float64 forms:", {k: (f"{v:.5g}", where[k]) for k, v in worst.items()})
    for k in R.Tol._fields:
        tol = getattr(G.SIM3OPT_TOL, k)
        assert worst[k] <= tol / 2, (k, worst[k], where[k], tol)
        assert tol >= (1e-13 if k in ("state", "final") else 1.0), (k, tol)
