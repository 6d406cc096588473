"""k_lba_solve alone (xfh_debug_lba_solve: the kernel the schedule of xfh_local_ba_device launches, once, on a caller-made S, b and previous x) on the
systems of tests/lba_solve_rig.py.

Exact-arithmetic systems at n = 6 .. 768: x, L and d equal the construction by bits.  Failing pivots (0.0, -0.0, -2.0, a NaN) in the first, the middle
and the last column: solved = 0, x keeps its input bits, the factorisation stops at that column, and S is the host piece's by bytes.  Ill-conditioned
SPD systems (1e6, 1e12): x and S equal the host piece xfh_lba_solve and the Python rule by bits -- the order of the operations is the contract, the
arithmetic IEEE.  Everywhere: the strict upper triangle of S comes back untouched, and two runs from workspaces filled differently give identical
bytes.  tests/test_lba_solve_ref.py holds the host piece and the Python rule to the same on the CPU."""
import ctypes as C

import numpy as np
import pytest

import lba_solve_rig as G
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context

pytestmark = pytest.mark.gpu
D = np.float64
INVALID = 1


@pytest.fixture(scope="module")
def ctx():
    c = Context(nfeatures=1, max_height=32, max_width=32)
    yield c
    c.close()


def device_twice(ctx, case):
    """-> the device's (solved, x, S); run from a workspace of 0x3C bytes and again from one of 0xC3: identical bytes"""
    S, b = G.system(case)
    a, again = G.run_device(ctx, S, b, 0x3C), G.run_device(ctx, S, b, 0xC3)
    assert a[0] == again[0] and a[1].tobytes() == again[1].tobytes() and a[2].tobytes() == again[2].tobytes(), (case, "two runs differ")
    assert G.upper_untouched(a[2]), (case, "the upper triangle")
    return a


@pytest.mark.parametrize("n", G.SIZES)
def test_exact_systems(ctx, n):
    got = device_twice(ctx, ("exact", n))
    G.check_exact(n, got, "device")
    host = G.host_of(("exact", n))
    assert got[2].tobytes() == host[2].tobytes() and got[1].tobytes() == host[1].tobytes()


@pytest.mark.parametrize("n", G.SIZES)
def test_failing_pivots(ctx, n):
    for kind in G.KINDS:
        for k in G.positions(n):
            case = ("failing", n, kind, k)
            got, host = device_twice(ctx, case), G.host_of(case)
            G.check_failing(n, kind, k, got, "device")
            assert got[2].tobytes() == host[2].tobytes(), (case, "S differs from the host piece's", int(np.sum(got[2].view(np.uint64) != host[2].view(np.uint64))))


@pytest.mark.parametrize("n,c", G.ILL)
def test_ill_conditioned_systems(ctx, n, c):
    case = ("ill", n, c)
    got = device_twice(ctx, case)
    for name, ref in (("the host piece", G.host_of(case)), ("the Python rule", G.rule_of(case))):
        assert got[0] == ref[0] == 1, (case, name, got[0], ref[0])
        assert G.same_bits(got[1], ref[1]), (case, name, "x", int(np.sum(got[1] != ref[1])))
        assert G.same_bits(got[2], ref[2]), (case, name, "S", int(np.sum(got[2] != ref[2])))
    S, b = G.system(case)
    eta = G.backward_error(S, b, got[1])
    print("n = %d, condition 1e%d: backward error %.3g (cap %.3g)" % (n, c, eta, G.backward_error_cap(n)))
    assert eta <= G.backward_error_cap(n)


def test_every_refusal(ctx):
    L = capi.lib()
    S, b, x, solved = np.eye(12), np.ones(12), np.zeros(12), C.c_int(0)
    call = lambda n=12, h=ctx.h, S=S.ctypes.data, b=b.ctypes.data, x=x.ctypes.data, s=C.byref(solved): L.xfh_debug_lba_solve(h, n, S, b, x, 0, s)
    assert call() == 0 and solved.value == 1 and np.array_equal(x, np.ones(12))
    for n in (0, -6, 5, 7, 13, 767, 774, 1536):
        assert call(n=n) == INVALID, n
    assert call(h=None) == INVALID and call(S=None) == INVALID and call(b=None) == INVALID and call(x=None) == INVALID and call(s=None) == INVALID
