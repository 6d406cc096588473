"""The LDL^T of LocalBundleAdjustment on the systems of tests/lba_solve_rig.py, on the CPU: the host piece xfh_lba_solve and the Python rule
ref_local_ba.ldlt_factor against the construction (exact systems: L0, d0 and x0 by bits; failing pivots: stop at column k, x untouched), against each other
by bits (every system), and the ill-conditioned results under the backward-error cap.  tests/test_gpu_lba_solve.py holds k_lba_solve to the same."""
import numpy as np
import pytest

import lba_solve_rig as G


@pytest.mark.parametrize("n", G.SIZES)
def test_exact_systems_are_exact(n):
    host, rule = G.host_of(("exact", n)), G.rule_of(("exact", n))
    G.check_exact(n, host, "host")
    G.check_exact(n, rule, "rule")


@pytest.mark.parametrize("n", G.SIZES)
def test_failing_pivots_stop_at_their_column(n):
    for kind in G.KINDS:
        for k in G.positions(n):
            case = ("failing", n, kind, k)
            host, rule = G.host_of(case), G.rule_of(case)
            G.check_failing(n, kind, k, host, "host")
            G.check_failing(n, kind, k, rule, "rule")
            assert G.same_bits(host[2], rule[2]), case


@pytest.mark.parametrize("n,c", G.ILL)
def test_ill_conditioned_systems(n, c):
    S, b = G.ill(n, c)
    host, rule = G.host_of(("ill", n, c)), G.rule_of(("ill", n, c))
    assert host[0] == rule[0] and G.same_bits(host[1], rule[1]) and G.same_bits(host[2], rule[2]), (n, c)
    assert G.upper_untouched(host[2])
    eta, cap = G.backward_error(S, b, host[1]), G.backward_error_cap(n)
    print("n = %d, condition 1e%d: solved %d, backward error %.3g (cap %.3g), |x|_inf %.3g, smallest pivot %.3g" %
          (n, c, host[0], eta, cap, np.max(np.abs(host[1])), np.min(np.diag(host[2]))))
    assert host[0] == 1 and eta <= cap, (n, c, host[0], eta, cap)
