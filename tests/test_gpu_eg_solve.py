"""xfh_debug_eg_solve (include/xfeat_hip_bench.h: the blocked LDL^T k_eg_ldlt_diag / k_eg_ldlt_panel and k_eg_subst of xfh_essential_graph_device, alone)
against xfh_eg_solve, the column form on the host, BY BITS: x, the flag, and the lower triangle of S (L and d).  The tile is 64 wide: n = 7; 63, 64 and 65;
129 (2 T + 1); 300 (five block columns, the last one 44 wide); 896 and 1344 (14 and 21 block columns, more panel tiles than one wave of workgroups needs).
The systems have the block pattern of a connected pose graph (7 x 7 blocks J^T J on a chain with chords, plus a diagonal), so they are SPD and moderately
conditioned.  A pivot that is not > 0 in the first block, in an inner block and in the last column, and a NaN entry below the diagonal: the flag is 0 and x
keeps its bits.  Two runs over differently filled upper triangles (which nothing reads) and differently filled x give identical bytes."""
import numpy as np
import pytest

import essential_graph_rig as G
from xfeatslam_amd import capi
from xfeatslam_amd.extractor import Context

pytestmark = pytest.mark.gpu
D = np.float64
SIZES = (7, 63, 64, 65, 129, 300, 896, 1344)


@pytest.fixture(scope="module")
def ctx():
    c = Context(nfeatures=1, max_height=32, max_width=32)
    yield c
    c.close()


def run_host(S, b, x0):
    S, x = np.ascontiguousarray(S, D).copy(), np.array(x0, D)
    ok = capi.lib().xfh_eg_solve(len(b), S.ctypes.data, np.ascontiguousarray(b, D).ctypes.data, x.ctypes.data)
    return ok, x, S


def run_device(ctx, S, b, x0):
    S, x, b, flag = np.ascontiguousarray(S, D).copy(), np.array(x0, D), np.ascontiguousarray(b, D), np.full(1, -7, np.int32)
    rc = capi.lib().xfh_debug_eg_solve(ctx.h, len(b), S.ctypes.data, b.ctypes.data, x.ctypes.data, flag.ctypes.data)
    assert rc == 0, rc
    return int(flag[0]), x, S


def with_upper(S, value):
    S = S.copy()
    S[np.triu_indices(len(S), 1)] = value
    return S


@pytest.mark.parametrize("n", SIZES)
def test_solve_equals_the_column_form_by_bits(ctx, n):
    S, b = G.spd_system(n, 100 + n)
    lower = np.tril_indices(n)
    ok_h, x_h, L_h = run_host(S, b, np.full(n, 7.0))
    ok_d, x_d, L_d = run_device(ctx, with_upper(S, 123.0), b, np.full(n, 7.0))
    assert ok_h == 1 and ok_d == 1
    print("n = %d: residual |S x - b| / |b| = %.3g" % (n, np.linalg.norm(S @ x_d - b) / np.linalg.norm(b)))
    assert x_d.tobytes() == x_h.tobytes(), n
    assert L_d[lower].tobytes() == L_h[lower].tobytes(), n
    assert np.all(L_d[np.triu_indices(n, 1)] == 123.0)                      # the strict upper triangle is neither read nor written
    # two runs over differently filled workspaces: identical bytes
    ok_2, x_2, L_2 = run_device(ctx, with_upper(S, np.nan), b, np.full(n, np.nan))
    assert ok_2 == 1 and x_2.tobytes() == x_d.tobytes() and L_2[lower].tobytes() == L_d[lower].tobytes(), n


@pytest.mark.parametrize("n", (65, 300, 896))
def test_a_failing_pivot_stops_the_factorisation(ctx, n):
    S, b = G.spd_system(n, 200 + n)
    x0 = np.linspace(-3.0, 5.0, n)
    places = (("first block", 3, 0.0), ("an inner block", (n // 128) * 64 + 17 if n > 128 else n // 2, -1.0), ("the last column", n - 1, -0.0), ("a NaN pivot", n // 3, np.nan))
    for what, k, v in places:
        Sb = S.copy()
        Sb[k, k] = v
        ok_h, x_h, _ = run_host(Sb, b, x0)
        ok_d, x_d, _ = run_device(ctx, Sb, b, x0)
        assert ok_h == 0 and ok_d == 0 and x_d.tobytes() == x0.tobytes() == x_h.tobytes(), (n, what)
    Sb = S.copy()
    Sb[n - 2, 1] = np.nan                                                   # a NaN entry below the diagonal reaches a later pivot
    ok_h, x_h, _ = run_host(Sb, b, x0)
    ok_d, x_d, _ = run_device(ctx, Sb, b, x0)
    assert ok_h == 0 and ok_d == 0 and x_d.tobytes() == x0.tobytes(), n


def test_refusals(ctx):
    L = capi.lib()
    S, b = G.spd_system(7, 1)
    x, flag = np.zeros(7), np.zeros(1, np.int32)
    args = [S.ctypes.data, b.ctypes.data, x.ctypes.data, flag.ctypes.data]
    assert L.xfh_debug_eg_solve(ctx.h, 0, *args) == 1 and L.xfh_debug_eg_solve(ctx.h, 7 * 192 + 1, *args) == 1 and L.xfh_debug_eg_solve(None, 7, *args) == 1
    for i in range(4):
        a = list(args)
        a[i] = None
        assert L.xfh_debug_eg_solve(ctx.h, 7, *a) == 1, i
