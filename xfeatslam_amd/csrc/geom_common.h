// geom_common.h -- what every geometry solver (triangulate_math.h, twoview_math.h, sim3solve_math.h, mlpnp_math.h, poseopt_math.h) needs of the
// others, written ONCE for host and device (XFH_HD): the pinhole camera and the strided matrix view, the minimal set from raw draws, the
// rotation of a column pair and the fp64 one-sided Jacobi built on it with its column helpers, the 3 x 3 determinant, the unpivoted LDL^T solve,
// the Levenberg step of the two optimisers (poseopt_math.h, optsim3_math.h) on top of it and two one-liners.  Plain C++;
// tests/cpp/geom_common_test.cpp runs these very lines against the obvious forms, asan_poseopt_test.cpp and asan_optsim3_test.cpp the Levenberg step.
// Every product and sum is in the order written (the library is built with -ffp-contract=off).
#pragma once
#include "hd.h"
#include <math.h>
#include <float.h>
#include <stddef.h>

struct GeoCam { float fx, fy, cx, cy; };
// element k of a matrix lives at p[k * stride]: stride 1 on the host, the block width in LDS (one matrix per lane, bank-conflict free)
struct GeoMat { double* p; int stride; XFH_HD double& operator()(int k) const { return p[(size_t)k * stride]; } };

XFH_HD size_t geo_al16(size_t x) { return (x + 15) & ~(size_t)15; }
XFH_HD int geo_clamp_its(int v, int max_iters) { return v < 1 ? 1 : (v > max_iters ? max_iters : v); }

// ---- reductions --------------------------------------------------------------------------------------------------------------------------------
// Every sum that a workgroup folds: lane l of GEO_LANES adds the terms l, l + 256, l + 512, ... in that order to 0, then the 256 partial sums are folded
// s[l] += s[l + h] for h = 128, 64, .. 1.  geo_tree_fold is that fold on one thread (block_tree_fold of block_common.hip.h puts a barrier between the steps).
#define GEO_LANES 256
template <class T>
XFH_HD T geo_tree_fold(T* s) {
    for (int h = GEO_LANES / 2; h >= 1; h >>= 1)
        for (int l = 0; l < h; ++l) s[l] = s[l] + s[l + h];
    return s[0];
}

// ---- the minimal set of one RANSAC iteration ---------------------------------------------------------------------------------------------------
// DUtils::Random::RandomInt(0, d - 1) of one raw draw: int(((double)draw / ((double)rand_max + 1.0)) * d).  A draw outside 0 .. rand_max (the
// reference cannot produce one) is clamped into the vector: index 0 .. d - 1 always.
XFH_HD int geo_draw_index(int draw, int rand_max, int d) {
    const double v = ((double)draw / ((double)rand_max + 1.0)) * (double)d;
    return !(v >= 0.0) ? 0 : (v >= (double)d ? d - 1 : (int)v);
}
// K draws on the shrinking vAvailableIndices with swap-remove, without the vector: only the (at most K) positions a removal has overwritten
// are kept.  N >= K.
template <int K>
XFH_HD void geo_set(const int* draws, int rand_max, int N, int* set) {
    int pos[K], val[K], nd = 0;
    for (int j = 0; j < K; ++j) {
        const int size = N - j, r = geo_draw_index(draws[j], rand_max, size), last = size - 1;
        int idx = r, back = last, at = -1;
        for (int k = 0; k < nd; ++k) {
            if (pos[k] == r) { idx = val[k]; at = k; }
            if (pos[k] == last) back = val[k];
        }
        set[j] = idx;
        if (at >= 0) val[at] = back; else { pos[nd] = r; val[nd] = back; ++nd; }
    }
}

// ---- the fp64 one-sided Jacobi -----------------------------------------------------------------------------------------------------------------
#define GEO_JACOBI_MAX_SWEEPS 30
#define GEO_JACOBI_TOL 1e-15
// the rotation of one column pair from alpha = |U_p|^2, beta = |U_q|^2, gamma = U_p . U_q; false: the pair is orthogonal enough (or a NaN) and
// does not rotate.  Shared by the 4 x 4 register instance of triangulate_math.h and geo_jacobi below.
XFH_HD bool geo_jacobi_rotation(double alpha, double beta, double gamma, double* c, double* s) {
    if (!(fabs(gamma) > GEO_JACOBI_TOL * sqrt(alpha * beta))) return false;
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    *c = 1.0 / sqrt(1.0 + t * t); *s = *c * t;
    return true;
}
// columns p and q of A (rows x N, row-major) rotated by (c, s)
XFH_HD void geo_rotate_cols(const GeoMat& A, int rows, int N, int p, int q, double c, double s) {
    for (int r = 0; r < rows; ++r) {
        const double ap = A(r * N + p), aq = A(r * N + q);
        A(r * N + p) = c * ap - s * aq; A(r * N + q) = s * ap + c * aq;
    }
}
// U (rows x N, row-major, caller-given storage) <- U V with orthogonal columns; V (N x N) accumulates from the identity.  Cyclic sweeps over the
// pairs p < q in lexicographic order until a sweep rotates nothing, at most GEO_JACOBI_MAX_SWEEPS; returns the number of rotations.  For a
// symmetric U the columns of V are its eigenvectors and the column norms of U the magnitudes of its eigenvalues.
//   M > 0   the rows at compile time: the two columns of a pair are read ONCE into registers (2 M doubles) for the three dot products and the
//           rotation (k_twoview_fit reads LDS once per pair);
//   M == 0  `rows` at run time, the columns streamed: nothing is cached, and a square matrix rotates U and V in one row loop (ml_jacobi's form).
// Both forms add the same terms in the same order: their results are equal to the bit.
template <int M>
XFH_HD int geo_jacobi(const GeoMat& U, const GeoMat& V, int N, int rows = M) {
    for (int r = 0; r < N; ++r)
        for (int c = 0; c < N; ++c) V(r * N + c) = r == c ? 1.0 : 0.0;
    int total = 0;
    for (int sweep = 0; sweep < GEO_JACOBI_MAX_SWEEPS; ++sweep) {
        int rot = 0;
        for (int p = 0; p < N - 1; ++p)
            for (int q = p + 1; q < N; ++q) {
                double c, s;
                if constexpr (M > 0) {
                    double up[M], uq[M];
#pragma unroll
                    for (int r = 0; r < M; ++r) { up[r] = U(r * N + p); uq[r] = U(r * N + q); }
                    double alpha = up[0] * up[0], beta = uq[0] * uq[0], gamma = up[0] * uq[0];
#pragma unroll
                    for (int r = 1; r < M; ++r) { alpha = alpha + up[r] * up[r]; beta = beta + uq[r] * uq[r]; gamma = gamma + up[r] * uq[r]; }
                    if (!geo_jacobi_rotation(alpha, beta, gamma, &c, &s)) continue;
#pragma unroll
                    for (int r = 0; r < M; ++r) { U(r * N + p) = c * up[r] - s * uq[r]; U(r * N + q) = s * up[r] + c * uq[r]; }
                    geo_rotate_cols(V, N, N, p, q, c, s);
                } else {
                    double alpha = U(p) * U(p), beta = U(q) * U(q), gamma = U(p) * U(q);
                    for (int r = 1; r < rows; ++r) {
                        const double up = U(r * N + p), uq = U(r * N + q);
                        alpha = alpha + up * up; beta = beta + uq * uq; gamma = gamma + up * uq;
                    }
                    if (!geo_jacobi_rotation(alpha, beta, gamma, &c, &s)) continue;
                    if (rows == N) {
                        for (int r = 0; r < N; ++r) {
                            const double up = U(r * N + p), uq = U(r * N + q), vp = V(r * N + p), vq = V(r * N + q);
                            U(r * N + p) = c * up - s * uq; U(r * N + q) = s * up + c * uq;
                            V(r * N + p) = c * vp - s * vq; V(r * N + q) = s * vp + c * vq;
                        }
                    } else { geo_rotate_cols(U, rows, N, p, q, c, s); geo_rotate_cols(V, N, N, p, q, c, s); }
                }
                ++rot;
            }
        if (rot == 0) break;
        total += rot;
    }
    return total;
}
// the dot product of columns a and b of U (rows x N); a == b: the squared norm
XFH_HD double geo_col_dot(const GeoMat& U, int rows, int N, int a, int b) {
    double s = U(a) * U(b);
    for (int r = 1; r < rows; ++r) s = s + U(r * N + a) * U(r * N + b);
    return s;
}
// the column of least squared norm; on a tie the first, or with last_on_tie the last (a NaN never wins)
XFH_HD int geo_min_col(const GeoMat& U, int rows, int N, bool last_on_tie) {
    int best = 0;
    double bn = geo_col_dot(U, rows, N, 0, 0);
    for (int c = 1; c < N; ++c) {
        const double n = geo_col_dot(U, rows, N, c, c);
        if (last_on_tie ? n <= bn : n < bn) { bn = n; best = c; }
    }
    return best;
}
// the three columns of a 3 x 3 by squared norm n2, descending, stable (the earlier column first on a tie; a NaN stays where it is)
XFH_HD void geo_order3(const GeoMat& U, int* o, double* n2) {
    for (int c = 0; c < 3; ++c) { n2[c] = geo_col_dot(U, 3, 3, c, c); o[c] = c; }
    for (int a = 1; a < 3; ++a)
        for (int b = a; b > 0 && n2[o[b]] > n2[o[b - 1]]; --b) { const int t = o[b]; o[b] = o[b - 1]; o[b - 1] = t; }
}
template <class T>
XFH_HD T geo_det3(const T* A) {
    return (A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6])) + A[2] * (A[3] * A[7] - A[4] * A[6]);
}

// (H + lambda I) x = b by an unpivoted LDL^T in place of Eigen's pivoting LDLT + isPositive(): false, with x untouched, as soon as a pivot is not > 0
// (a NaN pivot included).  H is the N (N + 1) / 2 upper entries of the N x N (row-major, i <= j).  N = 6: PoseOptimization's Levenberg step and MLPnP's
// Gauss-Newton (pose_ldlt_solve); N = 7: OptimizeSim3's Levenberg step.
template <int N>
XFH_HD bool geo_ldlt_solve(const double* H, double lambda, const double* b, double* x) {
    double A[N][N], d[N], y[N];
    int n = 0;
    _Pragma("unroll")
    for (int i = 0; i < N; ++i)
        _Pragma("unroll")
        for (int j = i; j < N; ++j, ++n) { A[i][j] = H[n]; A[j][i] = H[n]; }
    _Pragma("unroll")
    for (int i = 0; i < N; ++i) A[i][i] = A[i][i] + lambda;
    _Pragma("unroll")
    for (int j = 0; j < N; ++j) {                                           // the strict lower triangle of A becomes L
        double dj = A[j][j];
        _Pragma("unroll")
        for (int k = 0; k < j; ++k) dj = dj - A[j][k] * A[j][k] * d[k];
        if (!(dj > 0.0)) return false;
        d[j] = dj;
        _Pragma("unroll")
        for (int i = j + 1; i < N; ++i) {
            double s = A[i][j];
            _Pragma("unroll")
            for (int k = 0; k < j; ++k) s = s - A[i][k] * A[j][k] * d[k];
            A[i][j] = s / dj;
        }
    }
    _Pragma("unroll")
    for (int i = 0; i < N; ++i) { double s = b[i]; for (int k = 0; k < i; ++k) s = s - A[i][k] * y[k]; y[i] = s; }
    _Pragma("unroll")
    for (int i = 0; i < N; ++i) y[i] = y[i] / d[i];
    _Pragma("unroll")
    for (int i = N - 1; i >= 0; --i) { double s = y[i]; for (int k = i + 1; k < N; ++k) s = s - A[k][i] * x[k]; x[i] = s; }
    return true;
}
XFH_HD bool pose_ldlt_solve(const double* H, double lambda, const double* b, double* x) { return geo_ldlt_solve<6>(H, lambda, b, x); }

// ---- the Levenberg step ------------------------------------------------------------------------------------------------------------------------
// g2o's optimize() loop (optimization_algorithm_levenberg.cpp:61-194) as a state machine that one lane or one host thread drives, written ONCE for
// PoseOptimization (PoseLM of poseopt_math.h, 6 unknowns) and OptimizeSim3 (Os3LM of optsim3_math.h, 7).  The driver runs the pass an action asks for
// over every edge at S.est and hands the folded sums back: BUILD wants the N (N + 1) / 2 upper entries of H, the N of b and the robust chi2
// (computeActiveErrors + activeRobustChi2 + buildSystem), TRIAL the robust chi2 alone, CLASSIFY is the optimiser's own step between two optimize() calls.
// LM is a flat struct with the fields est, backup, H, b, x, lambda, ni, currentChi, iniChi, iter, qmax, nbad_lm, solved and hdr, and the statics
//   N              the number of unknowns
//   H_ITERATIONS   where hdr counts the iterations; the trials, the rejected trials and the LDL^T failures follow it in that order
//   iterations(S)  the argument of the optimize() call that is running
//   oplus(S)       oplusImpl: the estimate S.est updated by S.x
enum { GEO_LM_BUILD = 0, GEO_LM_TRIAL = 1, GEO_LM_CLASSIFY = 2, GEO_LM_DONE = 3 };
#define GEO_LM_MAX_TRIALS 10              /* _maxTrialsAfterFailure */

template <class LM>
XFH_HD int geo_lm_trial(LM& S) {                                            // push(); setLambda; solve(); update(x)
    S.backup = S.est;
    S.solved = geo_ldlt_solve<LM::N>(S.H, S.lambda, S.b, S.x) ? 1 : 0;
    S.est = LM::oplus(S);
    ++S.hdr[LM::H_ITERATIONS + 1];
    if (!S.solved) ++S.hdr[LM::H_ITERATIONS + 3];
    return GEO_LM_TRIAL;
}
template <class LM>
XFH_HD int geo_lm_after_build(LM& S, const double* sums) {
    constexpr int N = LM::N, NH = N * (N + 1) / 2;
    _Pragma("unroll")
    for (int k = 0; k < NH; ++k) S.H[k] = sums[k];
    _Pragma("unroll")
    for (int k = 0; k < N; ++k) S.b[k] = sums[NH + k];
    S.currentChi = sums[NH + N]; S.iniChi = S.currentChi;
    if (S.iter == 0) {                                                      // computeLambdaInit: std::max(fabs(H_jj), maxDiagonal), a NaN first argument wins
        double m = 0.0;
        _Pragma("unroll")
        for (int j = 0, n = 0; j < N; n += N - j, ++j) { const double a = fabs(S.H[n]); m = (a < m) ? m : a; }
        S.lambda = 1e-5 * m; S.ni = 2.0; S.nbad_lm = 0;
    }
    S.qmax = 0;
    ++S.hdr[LM::H_ITERATIONS];
    return geo_lm_trial(S);
}
template <class LM>
XFH_HD int geo_lm_after_trial(LM& S, double chi) {
    const double tempChi = S.solved ? chi : DBL_MAX;
    double rho = S.currentChi - tempChi, scale = 0.0;
    _Pragma("unroll")
    for (int j = 0; j < LM::N; ++j) scale += S.x[j] * (S.lambda * S.x[j] + S.b[j]);
    scale += 1e-3;
    rho /= scale;
    if (rho > 0.0 && isfinite(tempChi)) {
        const double t = 2.0 * rho - 1.0;
        double alpha = 1.0 - t * t * t;
        alpha = (2.0 / 3.0 < alpha) ? 2.0 / 3.0 : alpha;                    // std::min(alpha, _goodStepUpperScale)
        const double f = (1.0 / 3.0 < alpha) ? alpha : 1.0 / 3.0;           // std::max(_goodStepLowerScale, alpha)
        S.lambda *= f; S.ni = 2.0; S.currentChi = tempChi;
    } else {
        S.lambda *= S.ni; S.ni *= 2.0;
        S.est = S.backup;                                                   // pop(): the edges keep the errors of the rejected estimate
        ++S.hdr[LM::H_ITERATIONS + 2];
    }
    ++S.qmax;
    if (rho < 0.0 && S.qmax < GEO_LM_MAX_TRIALS) return geo_lm_trial(S);
    if (S.qmax == GEO_LM_MAX_TRIALS || rho == 0.0) return GEO_LM_CLASSIFY;
    if ((S.iniChi - S.currentChi) * 1e3 < S.iniChi) ++S.nbad_lm; else S.nbad_lm = 0;
    if (S.nbad_lm >= 3) return GEO_LM_CLASSIFY;
    return ++S.iter < LM::iterations(S) ? GEO_LM_BUILD : GEO_LM_CLASSIFY;
}
