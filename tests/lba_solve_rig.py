"""Systems for the LDL^T of xfh_local_ba_device alone: xfh_debug_lba_solve (k_lba_solve on the device), xfh_lba_solve (the host piece) and
ref_local_ba.ldlt_factor (the Python rule) on the same S, b and previous x.

  exact(n)            S = L0 diag(d0) L0^T with L0 unit lower triangular, at most six entries of +-1 per row, d0 from {0.5, 1, 2, 4}, and b = S x0 with x0
                      integers in -4 .. 4: every operation of the unpivoted factorisation and of both substitutions is exact in fp64, so the construction
                      is the reference -- L, d and x come back as L0, d0 and x0 by bits.
  failing(n, kind, k) the same construction with d0[k] = 0.0 or -2.0, or a NaN or a -0.0 written over S[k][k]: the factorisation stops at column k exactly.
                      For the -0.0, row k of L0 is emptied first, so that no update of S[k][k] before column k subtracts anything but 0 * 0 * d = +0 and the
                      pivot that is read IS -0.0 (-0.0 - +0 = -0.0); a -0.0 inside d0 would be lost in the product's sums.
  ill(n, c)           Q diag(logspace(0, -c)) Q^T, not exact: the three forms must agree by bits (the order of the operations is the contract, the
                      arithmetic IEEE and uncontracted); the backward error of the result has the cap backward_error_cap(n).

The strict upper triangle of every S holds SENTINEL: no form may read or write it.  x is handed in as PREFILL: a failed factorisation leaves it."""
import ctypes as C
import functools

import numpy as np

import ref_local_ba as R
from xfeatslam_amd import capi

D = np.float64
SIZES = (6, 12, 36, 66, 198, 390, 768)            # one keyframe; two; a row longer than the 32-entry half-wave stride; more than 32 trailing rows; the limit
ILL = tuple((n, c) for n in (66, 198, 768) for c in (6, 12))
KINDS = ("zero", "minus_zero", "negative", "nan")
SENTINEL, PREFILL = -12345.678, 7.0


def positions(n):
    return (0, n // 2, n - 1)


def _construction(n, seed):
    rng = np.random.RandomState(seed)
    L0 = np.eye(n)
    for i in range(1, n):
        cols = rng.choice(i, min(i, int(rng.randint(1, 7))), replace=False)
        L0[i, cols] = rng.choice([-1.0, 1.0], len(cols))
    d0 = rng.choice([0.5, 1.0, 2.0, 4.0], n)
    x0 = rng.randint(-4, 5, n).astype(D)
    return L0, d0, x0


def _with_sentinel(S):
    S = np.tril(S) + 0.0                                                     # (no -0.0 from a product with a zero of L0: x - x and 0 - (+-0) are +0 from here on)
    S[np.triu_indices(len(S), 1)] = SENTINEL
    return S


def symmetric(S):
    """the matrix whose lower triangle a system's S holds"""
    T = np.tril(S)
    return T + np.tril(S, -1).T


@functools.lru_cache(maxsize=None)
def exact(n):
    """-> S (upper triangle = SENTINEL), b, L0, d0, x0"""
    L0, d0, x0 = _construction(n, 100 + n)
    S = (L0 * d0) @ L0.T
    # an entry of S is a sum of at most seven products +-1 * d * +-1 (a row of L0 has its 1 and at most six entries), d <= 4: halves of integers up to 28
    assert np.array_equal(S, S.T) and np.max(np.abs(S)) <= 28 and np.array_equal(S * 2, np.round(S * 2))
    return _with_sentinel(S), S @ x0 + 0.0, L0, d0, x0


@functools.lru_cache(maxsize=None)
def failing(n, kind, k):
    """-> S, b, L0: the factorisation must stop at column k with the columns before it equal to L0's"""
    L0, d0, x0 = _construction(n, 100 + n)
    L0, d0 = L0.copy(), d0.copy()
    if kind == "minus_zero":
        L0[k, :k] = 0.0
    if kind != "nan":
        d0[k] = {"zero": 0.0, "minus_zero": 0.0, "negative": -2.0}[kind]
    S = (L0 * d0) @ L0.T
    b = S @ x0 + 0.0
    S = _with_sentinel(S)
    if kind == "nan":
        S[k, k] = np.nan                                                     # (inside d0 it would be in every entry of S below and right of k)
    if kind == "minus_zero":
        assert S[k, k] == 0.0 and not S[k, :k].any()
        S[k, k] = -0.0
        assert np.signbit(S[k, k])
    return S, b, L0


@functools.lru_cache(maxsize=None)
def ill(n, c):
    """-> S, b"""
    rng = np.random.RandomState(1000 * c + n)
    Q = np.linalg.qr(rng.normal(0, 1, (n, n)))[0]
    S = (Q * np.logspace(0, -c, n)) @ Q.T
    return _with_sentinel(S), rng.normal(0, 1, n)


def backward_error(S, b, x):
    """eta = |b - S x|_inf / (|S|_inf |x|_inf + |b|_inf) in numpy.longdouble, S = the symmetric matrix of the lower triangle"""
    E = np.longdouble
    A, xv, bv = symmetric(S).astype(E), np.asarray(x).astype(E), np.asarray(b).astype(E)
    r = bv - A @ xv
    return float(np.max(np.abs(r)) / (np.max(np.sum(np.abs(A), 1)) * np.max(np.abs(xv)) + np.max(np.abs(bv))))


def backward_error_cap(n):
    """the Cholesky-type bound gamma_(3n+1) | |L||D||L^T| | with | |L||D||L^T| | <= n |S|: 4 n^2 2^-53, a cap and loose on purpose"""
    return 4.0 * n * n * 2.0 ** -53


# ---- the three forms: each -> (solved, x, S as the form left it) ----------------------------------------------------------------------------------------
def run_host(S, b, L=None):
    L = L or capi.lib()
    S, x = np.ascontiguousarray(S, D).copy(), np.full(len(b), PREFILL, D)
    ok = L.xfh_lba_solve(len(b), S.ctypes.data, np.ascontiguousarray(b, D).ctypes.data, x.ctypes.data)
    return int(ok), x, S


def run_rule(S, b):
    """the Python rule works on a matrix whose upper triangle it may use: it gets zeros there, and only its lower triangle is returned (SENTINEL above)"""
    ok, x, _, Sf = R.ldlt_factor(np.tril(S), b, np.full(len(b), PREFILL, D))
    Sf = np.tril(Sf)
    Sf[np.triu_indices(len(Sf), 1)] = SENTINEL
    return int(ok), x, Sf


def run_device(ctx, S, b, ws_fill, L=None):
    L = L or capi.lib()
    S, x, solved = np.ascontiguousarray(S, D).copy(), np.full(len(b), PREFILL, D), C.c_int(-7)
    capi.check(L.xfh_debug_lba_solve(ctx.h, len(b), S.ctypes.data, np.ascontiguousarray(b, D).ctypes.data, x.ctypes.data, ws_fill, C.byref(solved)), ctx.h)
    return solved.value, x, S


@functools.lru_cache(maxsize=None)
def host_of(case):
    """case: ("exact", n) | ("failing", n, kind, k) | ("ill", n, c) -> the host piece's result, computed once and shared"""
    S, b = system(case)
    return run_host(S, b)


@functools.lru_cache(maxsize=None)
def rule_of(case):
    S, b = system(case)
    return run_rule(S, b)


def system(case):
    return {"exact": exact, "failing": failing, "ill": ill}[case[0]](*case[1:])[:2]


def same_bits(a, b):
    """by bits; where a result holds NaNs, NaN-ness by position (the host's default NaN and the device's differ in sign)"""
    a, b = np.asarray(a, D), np.asarray(b, D)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def upper_untouched(S):
    return bool(np.all(S[np.triu_indices(len(S), 1)].view(np.uint64) == np.array(SENTINEL, D).view(np.uint64)))


def check_exact(n, got, tag):
    S, b, L0, d0, x0 = exact(n)
    ok, x, Sf = got
    lo = np.tril_indices(n, -1)
    assert ok == 1, (tag, n, ok)
    assert x.tobytes() == x0.tobytes(), (tag, n, "x", int(np.sum(x != x0)))
    assert Sf[lo].tobytes() == L0[lo].tobytes(), (tag, n, "L", int(np.sum(Sf[lo] != L0[lo])))
    assert np.diag(Sf).tobytes() == d0.tobytes(), (tag, n, "d")
    assert upper_untouched(Sf), (tag, n, "the upper triangle")


def check_failing(n, kind, k, got, tag):
    S, b, L0 = failing(n, kind, k)
    ok, x, Sf = got
    assert ok == 0, (tag, n, kind, k, ok)
    assert x.tobytes() == np.full(n, PREFILL, D).tobytes(), (tag, n, kind, k, "x moved")
    assert np.tril(Sf, -1)[:, :k].tobytes() == np.tril(L0, -1)[:, :k].tobytes(), (tag, n, kind, k, "a column before k")
    assert not Sf[k, k] > 0.0 and upper_untouched(Sf), (tag, n, kind, k)
    if kind == "minus_zero":                                                 # the pivot that was read, and left, is the -0.0 itself
        assert Sf[k, k] == 0.0 and np.signbit(Sf[k, k]), (tag, n, k, Sf[k, k])
