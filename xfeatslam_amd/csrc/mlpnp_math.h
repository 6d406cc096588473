// mlpnp_math.h -- the rule of xfh_mlpnp_solve_device, written ONCE for host and device (XFH_HD): MLPnPsolver (src/MLPnPsolver.cpp) as
// Tracking::Relocalization drives it (src/Tracking.cc:3678-3773) for the Pinhole camera: the compact correspondence list with bearing vectors and
// their null-space bases, the minimal sets from the caller's raw draws, computePose (planar test, A^T A, its least eigenvector, scale and nearest
// rotation, the candidate choice, Rodrigues, Gauss-Newton), CheckInliers, and the decision of the iterate(chunk) loop with Refine in its order-free
// form.  The contract is in include/xfeat_hip.h, line by line; the kernels of mlpnp.hip.h, the host entry points of capi_mlpnp.cpp (the
// single-thread form of the whole rule, xfh_mlpnp_solve_host, included) and tests/cpp/asan_mlpnp_test.cpp compile these very lines.
// All arithmetic is fp64 in the order written (the library is built with -ffp-contract=off) except where a float is spelled out.
#pragma once
#include "geom_common.h"
#include <math.h>
#include <float.h>
#include <stdint.h>
#include <stddef.h>
#include <limits.h>

enum { ML_TOO_FEW = 0, ML_NONE = 1, ML_BEST = 2, ML_REFINED = 3 };
enum { ML_H_N = 0, ML_H_STATUS = 1, ML_H_ITS = 2, ML_H_MIN_INLIERS = 3, ML_H_WINNER = 4, ML_H_NINL = 5, ML_H_BEST = 6, ML_H_BEST_COUNT = 7, ML_H_CONSUMED = 8,
       ML_H_REFINES = 9, ML_H_PLANAR = 10, ML_HEADER_INTS = 16 };
enum { ML_S_N = 0, ML_S_ITS = 1, ML_S_MIN = 2, ML_S_END = 3, ML_S_K0 = 4, ML_S_BEST_COUNT = 5, ML_S_BEST = 6, ML_S_NREC = 7 };      // the ints of a problem's `sel`
// one hypothesis or one Refine result: R [9], t [3] in double, the planar flag, the inlier count, two zeros
enum { ML_P_R = 0, ML_P_T = 9, ML_P_PLANAR = 12, ML_P_COUNT = 13, ML_HYP = 16 };
#define ML_MAX_ITERS 1024
#define ML_MIN_SET 6
#define ML_GN_ROUNDS 5
#define ML_GN_EPS 1e-5
#define ML_CHUNK 13                   // entries of A^T A (78 = 6 x 13, 45 = 3 x 13 + 6) folded per pass; J^T J and J^T r (27) take 9 per pass

XFH_HD double ml_dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
XFH_HD double ml_norm3(const double* a) { return sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]); }
// M v of a row-major 3 x 3; Mt v of its transpose
XFH_HD void ml_mv(const double* M, const double* v, double* o) { for (int r = 0; r < 3; ++r) o[r] = (M[3 * r] * v[0] + M[3 * r + 1] * v[1]) + M[3 * r + 2] * v[2]; }
XFH_HD void ml_mtv(const double* M, const double* v, double* o) { for (int c = 0; c < 3; ++c) o[c] = (M[c] * v[0] + M[3 + c] * v[1]) + M[6 + c] * v[2]; }

// ---- step 4: the minimal set of one iteration (:128-140): six draws on the shrinking vAvailableIndices, geo_set<ML_MIN_SET>.  N >= 6. ---------------------

// ---- step 2: SetRansacParameters (:225-260) for one N: host libm, so both values are tables the caller fills on the host ------------------------------
inline void ml_params(double prob, int min_inliers, int max_its, int min_set, float eps, int N, int* its, int* min_eff) {
    int nmin = (int)((float)N * eps);
    if (nmin < min_inliers) nmin = min_inliers;
    if (nmin < min_set) nmin = min_set;
    *min_eff = nmin;
    float e = eps;
    if (e < (float)nmin / (float)N) e = (float)nmin / (float)N;
    int n;
    if (nmin == N) n = 1;
    else {
        const double v = ceil(log(1.0 - prob) / log(1.0 - pow((double)e, 3.0)));
        if (!isfinite(v) || v > (double)INT_MAX || v < (double)INT_MIN) { *its = max_its > 1 ? max_its : 1; return; }     // the reference's cast is undefined there
        n = (int)v;
    }
    const int m = n < max_its ? n : max_its;
    *its = m > 1 ? m : 1;
}

// ---- step 1: the bearing vector of one keypoint, float: Pinhole::unproject, then `/= z` with z == 1 --------------------------------------------------
XFH_HD void ml_bearing(const GeoCam& k, float x, float y, float* f) { f[0] = (x - k.cx) / k.fx; f[1] = (y - k.cy) / k.fy; f[2] = 1.0f; }
// ---- step 5 (a): columns 2 and 3 of the Householder reflection that maps f = (x, y, 1) onto -sg |f| e_1 ------------------------------------------------
XFH_HD void ml_nullspace(const double* f, double* rs) {
    const double n = sqrt((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]), sg = f[0] >= 0.0 ? n : -n;
    const double v[3] = {f[0] + sg, f[1], f[2]};
    const double vv = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    const double c1 = 2.0 * v[1] / vv, c2 = 2.0 * v[2] / vv;
    rs[0] = -(c1 * v[0]); rs[1] = 1.0 - c1 * v[1]; rs[2] = -(c1 * v[2]);
    rs[3] = -(c2 * v[0]); rs[4] = -(c2 * v[1]); rs[5] = 1.0 - c2 * v[2];
}

// ---- the fp64 one-sided Jacobi for a square matrix of run-time size n (3, 9 or 12) in caller-given storage, with its column helpers ---------------------
// geo_jacobi<0>, geo_col_dot and geo_order3 of geom_common.h term by term, but written out here: k_mlpnp_fit sits at 256 VGPRs + 256 AGPRs with 1020
// bytes of scratch, and with the shared forms inlined the same registers and scratch are allocated differently and it runs 2.4 - 3 % slower
// (profiles/geometry_common.md).  U (n x n, row-major) <- U V with orthogonal columns; V accumulates from the identity.
XFH_HD void ml_jacobi(const GeoMat& U, const GeoMat& V, int n) {
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) V(r * n + c) = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < GEO_JACOBI_MAX_SWEEPS; ++sweep) {
        int rot = 0;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                double alpha = U(p) * U(p), beta = U(q) * U(q), gamma = U(p) * U(q);
                for (int r = 1; r < n; ++r) {
                    const double up = U(r * n + p), uq = U(r * n + q);
                    alpha = alpha + up * up; beta = beta + uq * uq; gamma = gamma + up * uq;
                }
                double c, s;
                if (!geo_jacobi_rotation(alpha, beta, gamma, &c, &s)) continue;
                for (int r = 0; r < n; ++r) {
                    const double up = U(r * n + p), uq = U(r * n + q), vp = V(r * n + p), vq = V(r * n + q);
                    U(r * n + p) = c * up - s * uq; U(r * n + q) = s * up + c * uq;
                    V(r * n + p) = c * vp - s * vq; V(r * n + q) = s * vp + c * vq;
                }
                ++rot;
            }
        if (rot == 0) break;
    }
}
XFH_HD double ml_col_norm2(const GeoMat& U, int n, int c) {
    double s = U(c) * U(c);
    for (int r = 1; r < n; ++r) s = s + U(r * n + c) * U(r * n + c);
    return s;
}
// the three columns of a 3 x 3 by squared norm: o[0..2] descending, stable
XFH_HD void ml_order3(const GeoMat& U, int* o) {
    double n2[3];
    for (int c = 0; c < 3; ++c) { n2[c] = ml_col_norm2(U, 3, c); o[c] = c; }
    for (int a = 1; a < 3; ++a)
        for (int b = a; b > 0 && n2[o[b]] > n2[o[b - 1]]; --b) { const int t = o[b]; o[b] = o[b - 1]; o[b - 1] = t; }
}
// U V^T of the SVD of A (row-major 3 x 3): (u0 v0^T + u1 v1^T) + u2 v2^T, columns by norm descending, u = column / norm
XFH_HD void ml_nearest_rotation(const double* A, const GeoMat& U, const GeoMat& V, double* R) {
    for (int k = 0; k < 9; ++k) U(k) = A[k];
    ml_jacobi(U, V, 3);
    int o[3]; double w[3];
    ml_order3(U, o);
    for (int k = 0; k < 3; ++k) w[k] = sqrt(ml_col_norm2(U, 3, o[k]));
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            R[3 * i + j] = ((U(3 * i + o[0]) / w[0]) * V(3 * j + o[0]) + (U(3 * i + o[1]) / w[1]) * V(3 * j + o[1])) + (U(3 * i + o[2]) / w[2]) * V(3 * j + o[2]);
}

// ---- step 5 (b): the rank of the symmetric S (xx, xy, xz, yy, yz, zz) by a full-pivot Householder QR ---------------------------------------------------
XFH_HD int ml_rank3(const double* S6) {
    double A[3][3] = {{S6[0], S6[1], S6[2]}, {S6[1], S6[3], S6[4]}, {S6[2], S6[4], S6[5]}};
    double piv[3] = {0.0, 0.0, 0.0}, first = 0.0;
    int np = 0;
    for (int k = 0; k < 3; ++k) {
        double big = -1.0; int br = k, bc = k;
        for (int r = k; r < 3; ++r)
            for (int c = k; c < 3; ++c) { const double a = fabs(A[r][c]); if (a > big) { big = a; br = r; bc = c; } }
        if (k == 0) first = big;
        if (!(big > 3.0 * DBL_EPSILON * first)) break;
        for (int c = 0; c < 3; ++c) { const double t = A[k][c]; A[k][c] = A[br][c]; A[br][c] = t; }
        for (int r = 0; r < 3; ++r) { const double t = A[r][k]; A[r][k] = A[r][bc]; A[r][bc] = t; }
        double ss = 0.0;
        for (int r = k; r < 3; ++r) ss = ss + A[r][k] * A[r][k];
        const double nrm = sqrt(ss);
        piv[np++] = nrm;
        if (k == 2) break;
        double v[3] = {0.0, 0.0, 0.0};
        for (int r = k; r < 3; ++r) v[r] = A[r][k];
        v[k] = v[k] - (A[k][k] >= 0.0 ? -nrm : nrm);
        double vv = 0.0;
        for (int r = k; r < 3; ++r) vv = vv + v[r] * v[r];
        for (int c = k + 1; c < 3; ++c) {
            double d = 0.0;
            for (int r = k; r < 3; ++r) d = d + v[r] * A[r][c];
            const double f = 2.0 * d / vv;
            for (int r = k; r < 3; ++r) A[r][c] = A[r][c] - f * v[r];
        }
    }
    double mx = 0.0;
    for (int k = 0; k < np; ++k) if (piv[k] > mx) mx = piv[k];
    int rank = 0;
    for (int k = 0; k < np; ++k) if (piv[k] > 3.0 * DBL_EPSILON * mx) ++rank;
    return rank;
}
// eigenRot: the eigenvectors of S as ROWS, increasing eigenvalue (column norm of the Jacobi's U), stable
XFH_HD void ml_eigen_rot(const double* S6, const GeoMat& U, const GeoMat& V, double* E) {
    const double A[9] = {S6[0], S6[1], S6[2], S6[1], S6[3], S6[4], S6[2], S6[4], S6[5]};
    for (int k = 0; k < 9; ++k) U(k) = A[k];
    ml_jacobi(U, V, 3);
    double n2[3];
    for (int c = 0; c < 3; ++c) n2[c] = ml_col_norm2(U, 3, c);
    int inc[3] = {0, 1, 2};                                                 // ascending, stable: equal norms keep their column order
    for (int a = 1; a < 3; ++a)
        for (int b = a; b > 0 && n2[inc[b]] < n2[inc[b - 1]]; --b) { const int t = inc[b]; inc[b] = inc[b - 1]; inc[b - 1] = t; }
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) E[3 * r + c] = V(3 * c + inc[r]);
}

// ---- step 5 (c): the two rows of the design matrix of one point, and the upper entries of A^T A in row-major order ------------------------------------------
XFH_HD void ml_design_rows(const double* r, const double* s, const double* q, bool planar, double* a, double* b) {
    if (planar) {
        for (int k = 0; k < 3; ++k) {
            a[2 * k] = r[k] * q[1]; a[2 * k + 1] = r[k] * q[2]; a[6 + k] = r[k];
            b[2 * k] = s[k] * q[1]; b[2 * k + 1] = s[k] * q[2]; b[6 + k] = s[k];
        }
        for (int k = 9; k < 12; ++k) { a[k] = 0.0; b[k] = 0.0; }
    } else {
        for (int k = 0; k < 3; ++k) {
            for (int c = 0; c < 3; ++c) { a[3 * k + c] = r[k] * q[c]; b[3 * k + c] = s[k] * q[c]; }
            a[9 + k] = r[k]; b[9 + k] = s[k];
        }
    }
}
XFH_HD void ml_upper_ij(int cols, int e, int* i, int* j) {
    int r = 0, left = e;
    while (r < cols - 1 && left >= cols - r) { left -= cols - r; ++r; }
    *i = r; *j = r + left;
}

// ---- step 5 (f) ---------------------------------------------------------------------------------------------------------------------------------------------
XFH_HD void ml_rodrigues2rot(const double* w, double* R) {
    const double n = ml_norm3(w);
    for (int k = 0; k < 9; ++k) R[k] = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
    if (!(n > DBL_EPSILON)) return;
    const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
    const double a = sin(n) / n, b = (1.0 - cos(n)) / (n * n);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double kk = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j];
            R[3 * i + j] = (R[3 * i + j] + a * K[3 * i + j]) + b * kk;
        }
}
XFH_HD void ml_rot2rodrigues(const double* R, double* w) {
    w[0] = 0.0; w[1] = 0.0; w[2] = 0.0;
    const double trace = ((R[0] + R[4]) + R[8]) - 1.0;
    const double wn = acos(trace / 2.0);
    if (!(wn > DBL_EPSILON)) return;
    const double sc = wn / (2.0 * sin(wn));
    w[0] = (R[7] - R[5]) * sc; w[1] = (R[2] - R[6]) * sc; w[2] = (R[3] - R[1]) * sc;
}

// ---- step 5 (g): one round of mlpnp_gn at x = (w, T) -----------------------------------------------------------------------------------------------------------
struct MlGn { double R[9], P[9], T[3]; };
XFH_HD void ml_gn_begin(const double* x, MlGn* g) {
    ml_rodrigues2rot(x, g->R);
    const double w[3] = {x[0], x[1], x[2]};
    const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
    double D[9];                                                            // R^T - I
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) D[3 * i + j] = g->R[3 * j + i] - (i == j ? 1.0 : 0.0);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double q = (D[3 * i] * K[j] + D[3 * i + 1] * K[3 + j]) + D[3 * i + 2] * K[6 + j];
            g->P[3 * i + j] = (w[i] * w[j] + q) / th2;
        }
    g->T[0] = x[3]; g->T[1] = x[4]; g->T[2] = x[5];
}
// the two residuals and the two rows of the Jacobian (J [12]: the r row, then the s row) of one point X with basis r, s
XFH_HD void ml_gn_rows(const MlGn& g, const double* X, const double* r, const double* s, double* res, double* J) {
    double q[3], v[3], u[3];
    ml_mv(g.R, X, q);
    for (int k = 0; k < 3; ++k) v[k] = q[k] + g.T[k];
    const double nv = ml_norm3(v);
    for (int k = 0; k < 3; ++k) u[k] = v[k] / nv;
    for (int a = 0; a < 2; ++a) {
        const double* n = a ? s : r;
        const double d = ml_dot3(n, u);
        res[a] = d;
        double gg[3], k3[3], h[3];
        for (int k = 0; k < 3; ++k) gg[k] = (n[k] - d * u[k]) / nv;
        ml_mtv(g.R, gg, k3);
        h[0] = k3[1] * X[2] - k3[2] * X[1]; h[1] = k3[2] * X[0] - k3[0] * X[2]; h[2] = k3[0] * X[1] - k3[1] * X[0];
        for (int j = 0; j < 3; ++j) J[6 * a + j] = -((g.P[j] * h[0] + g.P[3 + j] * h[1]) + g.P[6 + j] * h[2]);
        for (int j = 0; j < 3; ++j) J[6 * a + 3 + j] = gg[j];
    }
}
// term e of the 27 sums: the 21 upper entries of J^T J (row-major, i <= j), then the 6 of J^T r
XFH_HD double ml_gn_term(const double* J, const double* res, int e) {
    if (e >= 21) { const int i = e - 21; return J[i] * res[0] + J[6 + i] * res[1]; }
    int i, j;
    ml_upper_ij(6, e, &i, &j);
    return J[i] * J[j] + J[6 + i] * J[6 + j];
}
// the 6 x 6 solve and :744; true: the rounds end here without an update
XFH_HD bool ml_gn_solve(const double* sums27, double* dx) {
    for (int k = 0; k < 6; ++k) dx[k] = 0.0;
    if (!pose_ldlt_solve(sums27, 0.0, sums27 + 21, dx)) return true;
    bool any5 = false, all1 = true;
    for (int k = 0; k < 6; ++k) { const double a = fabs(dx[k]); if (a > 5.0) any5 = true; if (!(a > 1.0)) all1 = false; }
    return any5 || all1;
}
// :748 of one point: how many of its two rows are NOT below the bound
XFH_HD int ml_gn_not_below(const double* J, const double* dx) {
    int c = 0;
    for (int a = 0; a < 2; ++a) {
        const double* j = J + 6 * a;
        const double d = ((((j[0] * dx[0] + j[1] * dx[1]) + j[2] * dx[2]) + j[3] * dx[3]) + j[4] * dx[4]) + j[5] * dx[5];
        if (!(fabs(d) < ML_GN_EPS)) ++c;
    }
    return c;
}

// ---- step 5 (d), (e): from the finished A^T A in U (cols x cols, symmetric) to the linear estimate x = (w, T) -------------------------------------------
// f6, p6: the FIRST six correspondences (bearing vector, point), [6][3]
XFH_HD void ml_linear(const GeoMat& U, const GeoMat& V, bool planar, const double* E, const double* f6, const double* p6, double* x) {
    const int cols = planar ? 9 : 12;
    ml_jacobi(U, V, cols);
    const int col = geo_min_col(U, cols, cols, true);
    double res[12];
    for (int k = 0; k < 12; ++k) res[k] = k < cols ? V(k * cols + col) : 0.0;
    double Rout[9], tout[3];
    if (planar) {
        double c1[3] = {res[0], res[2], res[4]}, c2[3] = {res[1], res[3], res[5]};
        double c0[3] = {c1[1] * c2[2] - c1[2] * c2[1], c1[2] * c2[0] - c1[0] * c2[2], c1[0] * c2[1] - c1[1] * c2[0]};
        const double tmp[9] = {c0[0], c0[1], c0[2], c1[0], c1[1], c1[2], c2[0], c2[1], c2[2]};       // transposed: the columns became the rows
        const double k1[3] = {tmp[1], tmp[4], tmp[7]}, k2[3] = {tmp[2], tmp[5], tmp[8]};
        const double scale = 1.0 / sqrt(fabs(ml_norm3(k1) * ml_norm3(k2)));
        double R1[9], Rb[9];
        ml_nearest_rotation(tmp, U, V, R1);
        if (geo_det3(R1) < 0.0) for (int k = 0; k < 9; ++k) R1[k] = R1[k] * -1.0;
        for (int i = 0; i < 3; ++i)                                             // eigenRot^T R1, then transposed and negated
            for (int j = 0; j < 3; ++j) Rb[3 * j + i] = ((E[i] * R1[j] + E[3 + i] * R1[3 + j]) + E[6 + i] * R1[6 + j]) * -1.0;
        const double t[3] = {scale * res[6], scale * res[7], scale * res[8]};
        if (geo_det3(Rb) < 0.0) { Rb[2] = Rb[2] * -1.0; Rb[5] = Rb[5] * -1.0; Rb[8] = Rb[8] * -1.0; }
        double best = 0.0; int bi = 0;
        for (int i = 0; i < 4; ++i) {
            const double sr = i >= 2 ? -1.0 : 1.0, st = (i & 1) ? -1.0 : 1.0;
            double norms = 0.0;
            for (int p = 0; p < 6; ++p) {
                double v[3];
                for (int r = 0; r < 3; ++r) v[r] = (((sr * Rb[3 * r]) * p6[3 * p] + (sr * Rb[3 * r + 1]) * p6[3 * p + 1]) + Rb[3 * r + 2] * p6[3 * p + 2]) + st * t[r];
                const double n = ml_norm3(v);
                for (int r = 0; r < 3; ++r) v[r] = v[r] / n;
                norms = norms + (1.0 - ml_dot3(v, f6 + 3 * p));
            }
            if (i == 0 || norms < best) { best = norms; bi = i; }
        }
        const double sr = bi >= 2 ? -1.0 : 1.0, st = (bi & 1) ? -1.0 : 1.0;
        for (int r = 0; r < 3; ++r) { Rout[3 * r] = sr * Rb[3 * r]; Rout[3 * r + 1] = sr * Rb[3 * r + 1]; Rout[3 * r + 2] = Rb[3 * r + 2]; tout[r] = st * t[r]; }
    } else {
        const double tmp[9] = {res[0], res[3], res[6], res[1], res[4], res[7], res[2], res[5], res[8]};
        const double k0[3] = {tmp[0], tmp[3], tmp[6]}, k1[3] = {tmp[1], tmp[4], tmp[7]}, k2[3] = {tmp[2], tmp[5], tmp[8]};
        const double scale = 1.0 / cbrt(fabs((ml_norm3(k0) * ml_norm3(k1)) * ml_norm3(k2)));
        double R[9];
        ml_nearest_rotation(tmp, U, V, R);
        if (geo_det3(R) < 0.0) for (int k = 0; k < 9; ++k) R[k] = R[k] * -1.0;
        const double ts[3] = {scale * res[9], scale * res[10], scale * res[11]};
        double t0[3], ti[3];
        ml_mv(R, ts, t0);
        ml_mtv(R, t0, ti);                                                     // the inverse of [R | +-t0] is [R^T | -+R^T t0]
        double err[2];
        for (int sg = 0; sg < 2; ++sg) {
            err[sg] = 0.0;
            for (int p = 0; p < 6; ++p) {
                double v[3];
                ml_mtv(R, p6 + 3 * p, v);
                for (int r = 0; r < 3; ++r) v[r] = v[r] + (sg == 0 ? -ti[r] : ti[r]);
                const double n = ml_norm3(v);
                for (int r = 0; r < 3; ++r) v[r] = v[r] / n;
                err[sg] = err[sg] + (1.0 - ml_dot3(v, f6 + 3 * p));
            }
        }
        for (int r = 0; r < 3; ++r) {
            tout[r] = err[0] < err[1] ? -ti[r] : ti[r];
            for (int c = 0; c < 3; ++c) Rout[3 * r + c] = R[3 * c + r];
        }
    }
    ml_rot2rodrigues(Rout, x);
    x[3] = tout[0]; x[4] = tout[1]; x[5] = tout[2];
}

// ---- step 5 as a whole.  Cx supplies the points and the sums: the six points of a set in index order (MlSet6), the flagged correspondences in the
// 256-lane fold on one host thread (MlHostFold) or by a workgroup (mlpnp.hip.h).  Its members:
//   corr(c, f, p, r, s)        the doubles of correspondence c
//   first(j)                   the j-th of the first six correspondences
//   sum<K>(term, out)          out[k] = the rule's sum over the correspondences of term(c, t)[k]
//   leader() / sync()          one thread runs the serial parts on the shared state (U, V, *w), the others wait
struct MlShared { double E[9], x[6], dx[6], s6[6]; int planar, stop; };
template <class Cx>
XFH_HD void ml_compute_pose(Cx& cx, const GeoMat& U, const GeoMat& V, MlShared* w, double* Rt, int* planar_out) {
    double t[ML_CHUNK];
    cx.template sum<6>([&](int c, double* o) {
        double f[3], p[3], r[3], s[3];
        cx.corr(c, f, p, r, s);
        o[0] = p[0] * p[0]; o[1] = p[0] * p[1]; o[2] = p[0] * p[2]; o[3] = p[1] * p[1]; o[4] = p[1] * p[2]; o[5] = p[2] * p[2];
    }, t);
    if (cx.leader()) {
        for (int k = 0; k < 6; ++k) w->s6[k] = t[k];
        w->planar = ml_rank3(w->s6) == 2;
        for (int k = 0; k < 9; ++k) w->E[k] = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
        if (w->planar) ml_eigen_rot(w->s6, U, V, w->E);
    }
    cx.sync();
    const bool planar = w->planar != 0;
    const int cols = planar ? 9 : 12, entries = cols * (cols + 1) / 2;
    double E[9];
    for (int k = 0; k < 9; ++k) E[k] = w->E[k];
    for (int e0 = 0; e0 < entries; e0 += ML_CHUNK) {
        cx.template sum<ML_CHUNK>([&](int c, double* o) {
            double f[3], p[3], r[3], s[3], q[3], a[12], b[12];
            cx.corr(c, f, p, r, s);
            if (planar) ml_mv(E, p, q); else { q[0] = p[0]; q[1] = p[1]; q[2] = p[2]; }
            ml_design_rows(r, s, q, planar, a, b);
            int i, j;
            ml_upper_ij(cols, e0, &i, &j);
            for (int k = 0; k < ML_CHUNK; ++k) {
                o[k] = e0 + k < entries ? a[i] * a[j] + b[i] * b[j] : 0.0;
                if (++j == cols) { ++i; j = i; }
                if (i >= cols) { i = cols - 1; j = cols - 1; }
            }
        }, t);
        if (cx.leader()) {
            int i, j;
            ml_upper_ij(cols, e0, &i, &j);
            for (int k = 0; k < ML_CHUNK && e0 + k < entries; ++k) {
                U(i * cols + j) = t[k]; U(j * cols + i) = t[k];
                if (++j == cols) { ++i; j = i; }
            }
        }
    }
    if (cx.leader()) {
        double f6[18], p6[18];
        for (int j = 0; j < 6; ++j) { double r[3], s[3]; cx.corr(cx.first(j), f6 + 3 * j, p6 + 3 * j, r, s); }
        ml_linear(U, V, planar, E, f6, p6, w->x);
        w->stop = 0;
    }
    cx.sync();
    for (int round = 0; round < ML_GN_ROUNDS; ++round) {
        double x[6], dx[6], sums[27];
        for (int k = 0; k < 6; ++k) x[k] = w->x[k];
        MlGn g;
        ml_gn_begin(x, &g);
        for (int e0 = 0; e0 < 27; e0 += 9) {
            cx.template sum<9>([&](int c, double* o) {
                double f[3], p[3], r[3], s[3], res[2], J[12];
                cx.corr(c, f, p, r, s);
                ml_gn_rows(g, p, r, s, res, J);
                for (int k = 0; k < 9; ++k) o[k] = ml_gn_term(J, res, e0 + k);
            }, t);
            for (int k = 0; k < 9; ++k) sums[e0 + k] = t[k];
        }
        cx.sync();                                                              // (every thread has read w->x and holds the same sums)
        if (cx.leader()) {
            w->stop = ml_gn_solve(sums, w->dx) ? 2 : 0;
        }
        cx.sync();
        if (w->stop == 2) break;
        for (int k = 0; k < 6; ++k) dx[k] = w->dx[k];
        cx.template sum<1>([&](int c, double* o) {
            double f[3], p[3], r[3], s[3], res[2], J[12];
            cx.corr(c, f, p, r, s);
            ml_gn_rows(g, p, r, s, res, J);
            o[0] = (double)ml_gn_not_below(J, dx);
        }, t);
        cx.sync();
        if (cx.leader()) {
            for (int k = 0; k < 6; ++k) w->x[k] = x[k] - dx[k];
            w->stop = t[0] == 0.0 ? 1 : 0;
        }
        cx.sync();
        if (w->stop == 1) break;
    }
    cx.sync();
    double R[9];
    ml_rodrigues2rot(w->x, R);
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) Rt[4 * r + c] = R[3 * r + c]; Rt[4 * r + 3] = w->x[3 + r]; }
    *planar_out = planar ? 1 : 0;
    cx.sync();
}

// the six points of a minimal set, sums in index order from 0.0
struct MlSet6 {
    double f[18], p[18], rs[36];
    XFH_HD void corr(int c, double* fo, double* po, double* r, double* s) const {
        for (int k = 0; k < 3; ++k) { fo[k] = f[3 * c + k]; po[k] = p[3 * c + k]; r[k] = rs[6 * c + k]; s[k] = rs[6 * c + 3 + k]; }
    }
    XFH_HD int first(int j) const { return j; }
    XFH_HD bool leader() const { return true; }
    XFH_HD void sync() const {}
    template <int K, class F> XFH_HD void sum(F term, double* out) const {
        double t[K];
        for (int k = 0; k < K; ++k) out[k] = 0.0;
        for (int c = 0; c < 6; ++c) { term(c, t); for (int k = 0; k < K; ++k) out[k] = out[k] + t[k]; }
    }
};

// ---- step 6: CheckInliers of one correspondence; a NaN never passes ---------------------------------------------------------------------------------------
XFH_HD int ml_check(const double* Rt, const GeoCam& k, const float* X, const float* xy, float max_err, float* error2) {
    const float xc = (float)(((Rt[0] * (double)X[0] + Rt[1] * (double)X[1]) + Rt[2] * (double)X[2]) + Rt[3]);
    const float yc = (float)(((Rt[4] * (double)X[0] + Rt[5] * (double)X[1]) + Rt[6] * (double)X[2]) + Rt[7]);
    const float zc = (float)(((Rt[8] * (double)X[0] + Rt[9] * (double)X[1]) + Rt[10] * (double)X[2]) + Rt[11]);
    const float u = k.fx * xc / zc + k.cx, v = k.fy * yc / zc + k.cy;
    const float dx = xy[0] - u, dy = xy[1] - v;
    *error2 = dx * dx + dy * dy;
    return *error2 < max_err;
}

// ---- step 7: the scan of the counts of the iterations 0 .. end - 1: the distinct bests (records) and, per record, the first qualifying k >= k0 at
// which it is the current best (-1: never consulted).  sel[ML_S_BEST_COUNT / _BEST / _NREC] receive the final state.
XFH_HD void ml_scan(const int* cnt, int end, int k0, int min_eff, int* rec_it, int* rec_use, int* sel) {
    int best_count = 0, best_it = -1, nrec = 0;
    for (int k = 0; k < end; ++k) {
        const int c = cnt[k];
        if (c < min_eff) continue;
        if (nrec == 0 || c > best_count) { best_count = c; best_it = k; rec_it[nrec] = k; rec_use[nrec] = -1; ++nrec; }
        if (k >= k0 && rec_use[nrec - 1] < 0) rec_use[nrec - 1] = k;
    }
    sel[ML_S_BEST_COUNT] = best_count; sel[ML_S_BEST] = best_it; sel[ML_S_NREC] = nrec;
}
// the winner from the Refine results of the records (rec [nrec][ML_HYP]): the record index, or -1; *refines = the Refine evaluations up to there
XFH_HD int ml_winner(const int* rec_use, const double* rec, int nrec, int min_eff, int* refines) {
    int n = 0;
    for (int r = 0; r < nrec; ++r) {
        if (rec_use[r] < 0) continue;
        ++n;
        if ((int)rec[(size_t)r * ML_HYP + ML_P_COUNT] > min_eff) { *refines = n; return r; }
    }
    *refines = n;
    return -1;
}
XFH_HD void ml_too_few_header(int* hdr, int N) {
    for (int k = 0; k < ML_HEADER_INTS; ++k) hdr[k] = k == ML_H_N ? N : (k == ML_H_WINNER || k == ML_H_BEST ? -1 : 0);
}
// end of the loop of a call that starts at k0 (overflow-free: chunk and k0 are clamped to max_iters first)
XFH_HD int ml_end(int its, int k0, int chunk, int max_iters) {
    const int c = chunk > max_iters ? max_iters : chunk, s = k0 > max_iters ? max_iters : k0;
    const int e = its > s + c ? its : s + c;
    return e > max_iters ? max_iters : e;
}

// ---- the workspace of one call (device memory, B problems): offsets in bytes, every piece 16-byte aligned ----------------------------------------------
struct MlLayout { size_t cm, pt, xy, f, rs, sel, hyp, cnt, rec_it, rec_use, rec, per_problem; };
XFH_HD MlLayout ml_layout(int n, int max_iters) {
    MlLayout L; size_t o = 0;
    L.cm = o; o += geo_al16((size_t)n * 4);                   // int: the keypoint of correspondence c
    L.pt = o; o += geo_al16((size_t)n * 12);                  // float [n][3]: its point
    L.xy = o; o += geo_al16((size_t)n * 8);                   // float [n][2]: its keypoint position
    L.f = o; o += geo_al16((size_t)n * 12);                   // float [n][3]: its bearing vector
    L.rs = o; o += geo_al16((size_t)n * 48);                  // double [n][6]: its basis
    L.sel = o; o += 32;                                      // int [8]: ML_S_*
    L.hyp = o; o += (size_t)max_iters * ML_HYP * 8;          // double [max_iters][16]
    L.cnt = o; o += geo_al16((size_t)max_iters * 4);
    L.rec_it = o; o += geo_al16((size_t)max_iters * 4);
    L.rec_use = o; o += geo_al16((size_t)max_iters * 4);
    L.rec = o; o += (size_t)max_iters * ML_HYP * 8;          // double [max_iters][16]: the Refine of record r
    L.per_problem = geo_al16(o);
    return L;
}

// ---- the argument block of the kernels (mlpnp.hip.h), filled by capi_mlpnp.cpp ------------------------------------------------------------------------------
struct MlArgs {
    int B, n, nq, max_iters, rand_max, min_matches, chunk;
    size_t draws_stride;
    GeoCam cam;
    float max_err;
    const float *xy_un, *points;
    const int *assigned, *n_matches, *iters_of_N, *min_of_N, *start_iter, *draws;
    const unsigned char* valid;
    unsigned char* ws;
    int* header; float* Tcw; unsigned char* inliers; int* assigned_out;
};
struct MlWs { int *cm, *sel, *cnt, *rec_it, *rec_use; float *pt, *xy, *f; double *rs, *hyp, *rec; };
XFH_HD MlWs ml_ws(const MlArgs& a, int b) {
    const MlLayout L = ml_layout(a.n, a.max_iters);
    unsigned char* p = a.ws + (size_t)b * L.per_problem;
    MlWs w;
    w.cm = (int*)(p + L.cm); w.sel = (int*)(p + L.sel); w.cnt = (int*)(p + L.cnt); w.rec_it = (int*)(p + L.rec_it); w.rec_use = (int*)(p + L.rec_use);
    w.pt = (float*)(p + L.pt); w.xy = (float*)(p + L.xy); w.f = (float*)(p + L.f); w.rs = (double*)(p + L.rs); w.hyp = (double*)(p + L.hyp);
    w.rec = (double*)(p + L.rec);
    return w;
}
// the correspondence of keypoint i of problem b: false when it has no valid point
XFH_HD bool ml_corr_of(const MlArgs& a, int b, int i, float* pt) {
    const int q = a.assigned[(size_t)b * a.n + i];
    if (q < 0 || q >= a.nq) return false;
    if (a.valid && !a.valid[(size_t)b * a.nq + q]) return false;
    const float* p = a.points + ((size_t)b * a.nq + q) * 3;
    pt[0] = p[0]; pt[1] = p[1]; pt[2] = p[2];
    return true;
}
// what prepare's last thread writes: N and the parameters of the loop; its == 0 means TOO_FEW
XFH_HD void ml_select(const MlArgs& a, int b, int N, int* sel) {
    int min_eff = a.min_of_N[N];                                            // N <= n: inside the tables of n + 1 entries
    if (min_eff < ML_MIN_SET) min_eff = ML_MIN_SET;                         // (max(.., min_set) of step 2, whatever the table holds)
    const bool few = N < min_eff || N < ML_MIN_SET || (a.n_matches && a.n_matches[b] < a.min_matches);
    const int its = few ? 0 : geo_clamp_its(a.iters_of_N[N], a.max_iters);
    int k0 = a.start_iter ? a.start_iter[b] : 0;
    if (k0 < 0) k0 = 0;
    sel[ML_S_N] = N; sel[ML_S_ITS] = its; sel[ML_S_MIN] = min_eff; sel[ML_S_END] = few ? 0 : ml_end(its, k0, a.chunk, a.max_iters); sel[ML_S_K0] = k0;
    sel[ML_S_BEST_COUNT] = 0; sel[ML_S_BEST] = -1; sel[ML_S_NREC] = 0;
}
// one hypothesis: the set of iteration `it`, step 5 on its six points -> hyp [ML_HYP]
XFH_HD void ml_fit_iteration(const MlArgs& a, int b, const MlWs& w, int it, const GeoMat& U, const GeoMat& V, double* hyp) {
    int set[ML_MIN_SET];
    geo_set<ML_MIN_SET>(a.draws + (size_t)b * a.draws_stride + (size_t)ML_MIN_SET * it, a.rand_max, w.sel[ML_S_N], set);
    MlSet6 cx;
    for (int j = 0; j < ML_MIN_SET; ++j) {
        const size_t c = (size_t)set[j];
        for (int k = 0; k < 3; ++k) { cx.f[3 * j + k] = (double)w.f[3 * c + k]; cx.p[3 * j + k] = (double)w.pt[3 * c + k]; }
        for (int k = 0; k < 6; ++k) cx.rs[6 * j + k] = w.rs[6 * c + k];
    }
    MlShared sh;
    double Rt[12]; int planar;
    ml_compute_pose(cx, U, V, &sh, Rt, &planar);
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) hyp[ML_P_R + 3 * r + c] = Rt[4 * r + c]; hyp[ML_P_T + r] = Rt[4 * r + 3]; }
    hyp[ML_P_PLANAR] = (double)planar; hyp[ML_P_COUNT] = 0.0; hyp[14] = 0.0; hyp[15] = 0.0;
}
XFH_HD void ml_hyp_Rt(const double* hyp, double* Rt) {
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) Rt[4 * r + c] = hyp[ML_P_R + 3 * r + c]; Rt[4 * r + 3] = hyp[ML_P_T + r]; }
}
// the header of a problem that ran, from the scan and the Refine results; returns the hypothesis to report (NULL: none)
XFH_HD const double* ml_decide(const MlWs& w, int* hdr) {
    const int* sel = w.sel;
    const int min_eff = sel[ML_S_MIN], nrec = sel[ML_S_NREC];
    int refines = 0;
    const int wr = ml_winner(w.rec_use, w.rec, nrec, min_eff, &refines);
    const double* rep = nullptr;
    int status = ML_NONE, winner = -1, ninl = 0, consumed = sel[ML_S_END];
    int best = sel[ML_S_BEST], best_count = sel[ML_S_BEST_COUNT];
    if (wr >= 0) {                                                          // the loop returns at the winner: the best is the one it refined
        status = ML_REFINED; rep = w.rec + (size_t)wr * ML_HYP; winner = w.rec_use[wr]; ninl = (int)rep[ML_P_COUNT]; consumed = winner + 1;
        best = w.rec_it[wr]; best_count = w.cnt[best];
    } else if (best >= 0 && best_count >= min_eff) { status = ML_BEST; rep = w.hyp + (size_t)best * ML_HYP; ninl = best_count; }
    for (int k = 0; k < ML_HEADER_INTS; ++k) hdr[k] = 0;
    hdr[ML_H_N] = sel[ML_S_N]; hdr[ML_H_STATUS] = status; hdr[ML_H_ITS] = sel[ML_S_ITS]; hdr[ML_H_MIN_INLIERS] = min_eff; hdr[ML_H_WINNER] = winner; hdr[ML_H_NINL] = ninl;
    hdr[ML_H_BEST] = best; hdr[ML_H_BEST_COUNT] = best_count; hdr[ML_H_CONSUMED] = consumed; hdr[ML_H_REFINES] = refines;
    hdr[ML_H_PLANAR] = rep ? (int)rep[ML_P_PLANAR] : 0;
    return rep;
}

// ---- the flagged correspondences of a problem in the 256-lane fold, on one host thread ------------------------------------------------------------------
struct MlHostFold {
    int N; const float *f, *pt; const double* rs; const unsigned char* flag; bool fold; int first6[6];
    XFH_HD void corr(int c, double* fo, double* po, double* r, double* s) const {
        for (int k = 0; k < 3; ++k) { fo[k] = (double)f[3 * (size_t)c + k]; po[k] = (double)pt[3 * (size_t)c + k]; r[k] = rs[6 * (size_t)c + k]; s[k] = rs[6 * (size_t)c + 3 + k]; }
    }
    XFH_HD int first(int j) const { return first6[j]; }
    XFH_HD bool leader() const { return true; }
    XFH_HD void sync() const {}
    template <int K, class F> XFH_HD void sum(F term, double* out) const {
        double t[K];
        if (!fold) {
            for (int k = 0; k < K; ++k) out[k] = 0.0;
            for (int c = 0; c < N; ++c) if (!flag || flag[c]) { term(c, t); for (int k = 0; k < K; ++k) out[k] = out[k] + t[k]; }
            return;
        }
        double s[K][GEO_LANES];
        for (int k = 0; k < K; ++k) for (int l = 0; l < GEO_LANES; ++l) s[k][l] = 0.0;
        for (int c = 0; c < N; ++c) if (!flag || flag[c]) { term(c, t); for (int k = 0; k < K; ++k) s[k][c % GEO_LANES] = s[k][c % GEO_LANES] + t[k]; }
        for (int k = 0; k < K; ++k) out[k] = geo_tree_fold(s[k]);
    }
};
// step 5 of the flagged correspondences (at least six flagged); false when fewer than six are
inline bool ml_host_pose(int N, const float* f, const float* pt, const double* rs, const unsigned char* flag, bool fold, double* Rt, int* planar) {
    MlHostFold cx{N, f, pt, rs, flag, fold, {0, 0, 0, 0, 0, 0}};
    int nf = 0;
    for (int c = 0; c < N && nf < 6; ++c) if (!flag || flag[c]) cx.first6[nf++] = c;
    if (nf < 6) return false;
    double Um[144], Vm[144];
    MlShared sh;
    ml_compute_pose(cx, GeoMat{Um, 1}, GeoMat{Vm, 1}, &sh, Rt, planar);
    return true;
}

// ---- the whole rule for problem b on ONE host thread, over host pointers in the same argument block and workspace layout as the kernels -------------------
inline void ml_host_problem(const MlArgs& a, int b, unsigned char* flag /* n bytes */) {
    const MlWs w = ml_ws(a, b);
    const int n = a.n;
    int* hdr = a.header + (size_t)b * ML_HEADER_INTS;
    int N = 0;
    for (int i = 0; i < n; ++i) {
        float pt[3];
        if (!ml_corr_of(a, b, i, pt)) continue;
        const size_t c = (size_t)N++;
        w.cm[c] = i;
        for (int k = 0; k < 3; ++k) w.pt[3 * c + k] = pt[k];
        w.xy[2 * c] = a.xy_un[2 * (size_t)i]; w.xy[2 * c + 1] = a.xy_un[2 * (size_t)i + 1];
        ml_bearing(a.cam, w.xy[2 * c], w.xy[2 * c + 1], w.f + 3 * c);
        const double fd[3] = {(double)w.f[3 * c], (double)w.f[3 * c + 1], (double)w.f[3 * c + 2]};
        ml_nullspace(fd, w.rs + 6 * c);
    }
    ml_select(a, b, N, w.sel);
    if (w.sel[ML_S_ITS] == 0) {                                             // TOO_FEW: the header, and no match for the optimiser behind
        ml_too_few_header(hdr, N);
        for (int i = 0; i < n; ++i) a.assigned_out[(size_t)b * n + i] = -1;
        return;
    }
    const int end = w.sel[ML_S_END];
    double Um[144], Vm[144];
    for (int it = 0; it < end; ++it) {
        double* h = w.hyp + (size_t)it * ML_HYP;
        ml_fit_iteration(a, b, w, it, GeoMat{Um, 1}, GeoMat{Vm, 1}, h);
        double Rt[12];
        ml_hyp_Rt(h, Rt);
        int c = 0;
        for (int k = 0; k < N; ++k) { float e; c += ml_check(Rt, a.cam, w.pt + 3 * (size_t)k, w.xy + 2 * (size_t)k, a.max_err, &e); }
        w.cnt[it] = c;
    }
    ml_scan(w.cnt, end, w.sel[ML_S_K0], w.sel[ML_S_MIN], w.rec_it, w.rec_use, w.sel);
    for (int r = 0; r < w.sel[ML_S_NREC]; ++r) {
        double* rec = w.rec + (size_t)r * ML_HYP;
        for (int k = 0; k < ML_HYP; ++k) rec[k] = 0.0;
        if (w.rec_use[r] < 0) continue;
        double Rt[12], Rr[12];
        ml_hyp_Rt(w.hyp + (size_t)w.rec_it[r] * ML_HYP, Rt);
        for (int k = 0; k < N; ++k) { float e; flag[k] = (unsigned char)ml_check(Rt, a.cam, w.pt + 3 * (size_t)k, w.xy + 2 * (size_t)k, a.max_err, &e); }
        int planar = 0;
        ml_host_pose(N, w.f, w.pt, w.rs, flag, true, Rr, &planar);         // (the record has count >= min_eff >= 6 flags)
        int c = 0;
        for (int k = 0; k < N; ++k) { float e; c += ml_check(Rr, a.cam, w.pt + 3 * (size_t)k, w.xy + 2 * (size_t)k, a.max_err, &e); }
        for (int rr = 0; rr < 3; ++rr) { for (int cc = 0; cc < 3; ++cc) rec[ML_P_R + 3 * rr + cc] = Rr[4 * rr + cc]; rec[ML_P_T + rr] = Rr[4 * rr + 3]; }
        rec[ML_P_PLANAR] = (double)planar; rec[ML_P_COUNT] = (double)c;
    }
    const double* rep = ml_decide(w, hdr);
    for (int i = 0; i < n; ++i) { a.inliers[(size_t)b * n + i] = 0; a.assigned_out[(size_t)b * n + i] = -1; }
    if (!rep) return;
    double Rt[12];
    ml_hyp_Rt(rep, Rt);
    for (int k = 0; k < 12; ++k) a.Tcw[(size_t)b * 12 + k] = (float)Rt[k];
    for (int k = 0; k < N; ++k) {
        float e;
        if (!ml_check(Rt, a.cam, w.pt + 3 * (size_t)k, w.xy + 2 * (size_t)k, a.max_err, &e)) continue;
        const size_t i = (size_t)b * n + w.cm[k];
        a.inliers[i] = 1; a.assigned_out[i] = a.assigned[i];
    }
}
