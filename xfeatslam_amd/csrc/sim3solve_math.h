// sim3solve_math.h -- the rule of xfh_sim3_solve_device and xfh_sim3_merge_matches_device, written ONCE for host and device (XFH_HD): Sim3Solver
// (src/Sim3Solver.cc) as LoopClosing::DetectCommonRegionsFromBoW drives it (src/LoopClosing.cc:670-749) for the Pinhole camera: the merge of the
// per-covisible match lists, the compact correspondence list, the minimal sets from the caller's raw draws, Horn's closed form (ComputeSim3),
// CheckInliers, the decision of the iterate(20) loop in its order-free form, and the composition gScm * gSmw for the next projection search.
// The contract is in include/xfeat_hip.h, line by line; the kernels of sim3solve.hip.h, the host entry points of capi_sim3solve.cpp (the
// single-thread form of the whole rule, xfh_sim3_solve_host, included) and tests/cpp/asan_sim3solve_test.cpp compile these very lines.
// All arithmetic is fp32 in the order written (the library is built with -ffp-contract=off) except where a double is spelled out.
#pragma once
#include "geom_common.h"
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include <limits.h>

enum { S3_TOO_FEW = 0, S3_NO_MORE = 1, S3_CONVERGED = 2 };
enum { S3_H_N = 0, S3_H_STATUS = 1, S3_H_ITS = 2, S3_H_WINNER = 3, S3_H_NINL = 4, S3_H_BEST = 5, S3_H_BEST_COUNT = 6, S3_H_CONSUMED = 7, S3_HEADER_INTS = 16 };
// one hypothesis: T12 [3][4] = [sR|t], R12 [3][3], t12 [3], s12, T21 [3][4], three zeros; d_floats holds the first S3_FLOATS of the reported one
enum { S3_F_T12 = 0, S3_F_R12 = 12, S3_F_T = 21, S3_F_S = 24, S3_F_T21 = 25, S3_HYP = 40, S3_FLOATS = 32 };
#define S3_MAX_ITERS 4096
#define S3_MAX_SWEEPS 30
#define S3_JACOBI_TOL 1e-15

XFH_HD bool s3_row_ok(int r, int M) { return r >= 0 && r < M; }
// Rcw * X + tcw of a row-major [R|t]: each row ((a*x + b*y) + c*z) + t
XFH_HD void s3_transform(const float* T, const float* p, float* X) {
    for (int r = 0; r < 3; ++r) X[r] = ((T[4 * r] * p[0] + T[4 * r + 1] * p[1]) + T[4 * r + 2] * p[2]) + T[4 * r + 3];
}
// Pinhole::project (src/CameraModels/Pinhole.cpp:43-49)
XFH_HD void s3_project(const GeoCam& k, const float* X, float* uv) { uv[0] = k.fx * X[0] / X[2] + k.cx; uv[1] = k.fy * X[1] / X[2] + k.cy; }

// ---- the minimal set of one iteration (:245-259): three draws on the shrinking vAvailableIndices, geo_set<3>.  N >= 3. ----------------------------------

// ---- SetRansacParameters (:123-147): host libm, so the count is a table the caller fills on the host ---------------------------------------------------
inline int s3_iterations(double prob, int min_inliers, int max_its, int N) {
    int n;
    if (min_inliers == N) n = 1;
    else {
        const float epsilon = (float)min_inliers / (float)N;
        const double v = ceil(log(1.0 - prob) / log(1.0 - pow((double)epsilon, 3.0)));
        if (!isfinite(v) || v > (double)INT_MAX || v < (double)INT_MIN) return max_its > 1 ? max_its : 1;      // the reference's cast is undefined there
        n = (int)v;
    }
    const int m = n < max_its ? n : max_its;
    return m > 1 ? m : 1;
}

// ---- the eigenvector of the largest eigenvalue of the symmetric 4 x 4 N: cyclic two-sided Jacobi in fp64 --------------------------------------------
// pairs p < q in lexicographic order; a pair rotates iff |a_pq| > 1e-15 * |A|_F of the matrix as given; theta = (a_qq - a_pp) / (2 a_pq),
// t = sgn(theta) / (|theta| + sqrt(1 + theta^2)), c = 1 / sqrt(1 + t^2), s = c t; a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0, and for the other
// k: a_kp' = c a_kp - s a_kq, a_kq' = s a_kp + c a_kq (V's rows likewise).  Stop after the first sweep that rotates nothing, at most 30.
// q = V's column of the largest diagonal entry, the first of equal ones (a NaN rotates nothing and never wins: column 0 of the identity).
XFH_HD void s3_max_eigenvector(double (&A)[4][4], double* q) {
    double V[4][4];
    double f2 = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) { V[r][c] = r == c ? 1.0 : 0.0; f2 = f2 + A[r][c] * A[r][c]; }
    const double thr = S3_JACOBI_TOL * sqrt(f2);
    for (int sweep = 0; sweep < S3_MAX_SWEEPS; ++sweep) {
        int rot = 0;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int qq = p + 1; qq < 4; ++qq) {
                const double apq = A[p][qq];
                if (!(fabs(apq) > thr)) continue;
                const double theta = (A[qq][qq] - A[p][p]) / (2.0 * apq);
                const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(1.0 + theta * theta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                A[p][p] = A[p][p] - t * apq; A[qq][qq] = A[qq][qq] + t * apq; A[p][qq] = 0.0; A[qq][p] = 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (k != p && k != qq) {
                        const double akp = A[k][p], akq = A[k][qq];
                        A[k][p] = c * akp - s * akq; A[p][k] = A[k][p];
                        A[k][qq] = s * akp + c * akq; A[qq][k] = A[k][qq];
                    }
                    const double vp = V[k][p], vq = V[k][qq];
                    V[k][p] = c * vp - s * vq; V[k][qq] = s * vp + c * vq;
                }
                ++rot;
            }
        if (rot == 0) break;
    }
    double best = A[0][0];
    q[0] = V[0][0]; q[1] = V[1][0]; q[2] = V[2][0]; q[3] = V[3][0];
#pragma unroll
    for (int c = 1; c < 4; ++c)
        if (A[c][c] > best) { best = A[c][c]; q[0] = V[0][c]; q[1] = V[1][c]; q[2] = V[2][c]; q[3] = V[3][c]; }
}

// ---- ComputeSim3 (:311-412) of one minimal set: P1, P2 = the three camera-frame points of each keyframe, point j at [3j .. 3j + 3) ----------------------
XFH_HD void s3_horn(const float* P1, const float* P2, bool fix_scale, float* hyp) {
    float O1[3], O2[3], Pr1[9], Pr2[9];
    for (int c = 0; c < 3; ++c) {
        O1[c] = ((P1[c] + P1[3 + c]) + P1[6 + c]) / 3.0f;
        O2[c] = ((P2[c] + P2[3 + c]) + P2[6 + c]) / 3.0f;
    }
    for (int j = 0; j < 3; ++j)
        for (int c = 0; c < 3; ++c) { Pr1[3 * j + c] = P1[3 * j + c] - O1[c]; Pr2[3 * j + c] = P2[3 * j + c] - O2[c]; }
    float M[3][3];                                                          // M = Pr2 * Pr1^T, the sum over the three points in order
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[i][j] = (Pr2[i] * Pr1[j] + Pr2[3 + i] * Pr1[3 + j]) + Pr2[6 + i] * Pr1[6 + j];
    const double N11 = (double)((M[0][0] + M[1][1]) + M[2][2]), N12 = (double)(M[1][2] - M[2][1]), N13 = (double)(M[2][0] - M[0][2]),
                 N14 = (double)(M[0][1] - M[1][0]), N22 = (double)((M[0][0] - M[1][1]) - M[2][2]), N23 = (double)(M[0][1] + M[1][0]),
                 N24 = (double)(M[2][0] + M[0][2]), N33 = (double)((-M[0][0] + M[1][1]) - M[2][2]), N34 = (double)(M[1][2] + M[2][1]),
                 N44 = (double)((-M[0][0] - M[1][1]) + M[2][2]);
    double A[4][4] = {{N11, N12, N13, N14}, {N12, N22, N23, N24}, {N13, N23, N33, N34}, {N14, N24, N34, N44}};
    double q[4];
    s3_max_eigenvector(A, q);
    // the rotation of the unit quaternion (w, x, y, z) in double, rounded once: no atan2, no angle-axis, no 0 / 0 for a zero rotation
    const double qn = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    const double w = q[0] / qn, x = q[1] / qn, y = q[2] / qn, z = q[3] / qn;
    float R[9];
    R[0] = (float)(1.0 - 2.0 * (y * y + z * z)); R[1] = (float)(2.0 * (x * y - w * z)); R[2] = (float)(2.0 * (x * z + w * y));
    R[3] = (float)(2.0 * (x * y + w * z)); R[4] = (float)(1.0 - 2.0 * (x * x + z * z)); R[5] = (float)(2.0 * (y * z - w * x));
    R[6] = (float)(2.0 * (x * z - w * y)); R[7] = (float)(2.0 * (y * z + w * x)); R[8] = (float)(1.0 - 2.0 * (x * x + y * y));
    float s = 1.0f;
    if (!fix_scale) {
        double nom = 0.0, den = 0.0;                                        // column-major over the 3 x 3: point by point, x y z inside
        for (int j = 0; j < 3; ++j)
            for (int r = 0; r < 3; ++r) {
                const float p3 = (R[3 * r] * Pr2[3 * j] + R[3 * r + 1] * Pr2[3 * j + 1]) + R[3 * r + 2] * Pr2[3 * j + 2];
                nom = nom + (double)Pr1[3 * j + r] * (double)p3; den = den + (double)p3 * (double)p3;
            }
        s = (float)(nom / den);
    }
    const float inv = (float)(1.0 / (double)s);
    float sR[9], sRi[9], t[3];
    for (int k = 0; k < 9; ++k) sR[k] = s * R[k];
    for (int r = 0; r < 3; ++r) {
        t[r] = O1[r] - ((sR[3 * r] * O2[0] + sR[3 * r + 1] * O2[1]) + sR[3 * r + 2] * O2[2]);
        for (int c = 0; c < 3; ++c) sRi[3 * r + c] = inv * R[3 * c + r];
    }
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) { hyp[S3_F_T12 + 4 * r + c] = sR[3 * r + c]; hyp[S3_F_T21 + 4 * r + c] = sRi[3 * r + c]; hyp[S3_F_R12 + 3 * r + c] = R[3 * r + c]; }
        hyp[S3_F_T12 + 4 * r + 3] = t[r]; hyp[S3_F_T + r] = t[r];
        hyp[S3_F_T21 + 4 * r + 3] = -((sRi[3 * r] * t[0] + sRi[3 * r + 1] * t[1]) + sRi[3 * r + 2] * t[2]);
    }
    hyp[S3_F_S] = s; hyp[37] = 0.0f; hyp[38] = 0.0f; hyp[39] = 0.0f;
}

// ---- CheckInliers (:415-439) of one correspondence: err[0] against image 1, err[1] against image 2; a NaN never passes ------------------------------
XFH_HD int s3_check(const float* T12, const float* T21, const GeoCam& k1, const GeoCam& k2, const float* X1, const float* X2, const float* p1, const float* p2,
                    float max_err1, float max_err2, float* err) {
    float q[3], uv[2];
    s3_transform(T12, X2, q); s3_project(k1, q, uv);
    const float d0 = p1[0] - uv[0], d1 = p1[1] - uv[1];
    err[0] = d0 * d0 + d1 * d1;
    s3_transform(T21, X1, q); s3_project(k2, q, uv);
    const float e0 = uv[0] - p2[0], e1 = uv[1] - p2[1];
    err[1] = e0 * e0 + e1 * e1;
    return err[0] < max_err1 && err[1] < max_err2;
}

// ---- the composition for the next search (LoopClosing.cc:746-749, ORBmatcher.cc:621-622): Scw = S12 o T2w in double, rounded once -------------------
XFH_HD void s3_compose(const float* hyp, const float* T2w, float* Tcw, float* Ow) {
    double R[9], ts[3];
    const double s = (double)hyp[S3_F_S];
    for (int r = 0; r < 3; ++r) {
        const double a = (double)hyp[S3_F_R12 + 3 * r], b = (double)hyp[S3_F_R12 + 3 * r + 1], c = (double)hyp[S3_F_R12 + 3 * r + 2];
        for (int k = 0; k < 3; ++k) R[3 * r + k] = (a * (double)T2w[k] + b * (double)T2w[4 + k]) + c * (double)T2w[8 + k];
        const double t = s * ((a * (double)T2w[3] + b * (double)T2w[7]) + c * (double)T2w[11]) + (double)hyp[S3_F_T + r];
        ts[r] = t / s;
    }
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) Tcw[4 * r + k] = (float)R[3 * r + k];
        Tcw[4 * r + 3] = (float)ts[r];
        Ow[r] = (float)(-((R[r] * ts[0] + R[3 + r] * ts[1]) + R[6 + r] * ts[2]));
    }
}

// ---- the decision (:240-293 under `while(!bConverge && !bNoMore) iterate(20, ..)`) from the counts of its iterations, order-free ---------------------
// winner = the first k with count > min_inliers; best = the last k whose count is the largest (count * 4096 + k is its key)
XFH_HD int s3_best_key(int count, int k) { return count * S3_MAX_ITERS + k; }

// ---- the workspace of one call (device memory, B problems): offsets in bytes, every piece 16-byte aligned ----------------------------------------
struct S3Layout { size_t cm, X1, X2, P1, P2, sel, hyp, cnt, per_problem; };
XFH_HD S3Layout s3_layout(int n1) {
    S3Layout L; size_t o = 0;
    L.cm = o; o += geo_al16((size_t)n1 * 4);                  // int i1 of correspondence k
    L.X1 = o; o += geo_al16((size_t)n1 * 12);                 // float [n1][3] mvX3Dc1
    L.X2 = o; o += geo_al16((size_t)n1 * 12);
    L.P1 = o; o += geo_al16((size_t)n1 * 8);                  // float [n1][2] mvP1im1
    L.P2 = o; o += geo_al16((size_t)n1 * 8);
    L.sel = o; o += 32;                                      // int N, its (0: TOO_FEW)
    L.hyp = o; o += (size_t)S3_MAX_ITERS * S3_HYP * 4;       // float [4096][40]
    L.cnt = o; o += (size_t)S3_MAX_ITERS * 4;                // int [4096]
    L.per_problem = geo_al16(o);
    return L;
}
XFH_HD size_t s3_workspace_bytes(int n1, int M, int B) {
    const size_t solve = s3_layout(n1).per_problem * (size_t)B, merge = geo_al16((size_t)M * 4);       // the merge's owner table lies over the solver's part
    return solve > merge ? solve : merge;
}

// ---- the argument block of the kernels (sim3solve.hip.h), filled by capi_sim3solve.cpp ----------------------------------------------------------------
struct S3Args {
    int B, n1, M, max_iters, rand_max, min_inliers, min_matches, fix_scale;
    size_t draws_stride, T1w_stride;
    GeoCam cam1, cam2;
    float max_err1, max_err2;
    const float *points, *T1w, *T2w;
    const int *point1, *matched, *num_matches, *iters_of_N, *draws;
    unsigned char* ws;
    int* header; float* fout; unsigned char* inliers; float *Tcw, *Ow;
};
// the correspondence at slot i1 of problem b: false when either index is no row of the table
XFH_HD bool s3_corr(const S3Args& a, int b, int i1, float* X1, float* X2, float* p1, float* p2) {
    const int r1 = a.point1[i1], r2 = a.matched[(size_t)b * a.n1 + i1];
    if (!s3_row_ok(r1, a.M) || !s3_row_ok(r2, a.M)) return false;
    s3_transform(a.T1w + (size_t)b * a.T1w_stride, a.points + 3 * (size_t)r1, X1);
    s3_transform(a.T2w + (size_t)b * 12, a.points + 3 * (size_t)r2, X2);
    s3_project(a.cam1, X1, p1); s3_project(a.cam2, X2, p2);
    return true;
}
XFH_HD void s3_too_few_header(int* hdr, int N) {
    for (int k = 0; k < S3_HEADER_INTS; ++k) hdr[k] = k == S3_H_N ? N : (k == S3_H_WINNER || k == S3_H_BEST ? -1 : 0);
}

// ---- the whole rule for problem b on ONE host thread, over host pointers in the same argument block and workspace layout as the kernels ------------
inline void s3_host_problem(const S3Args& a, int b) {
    const S3Layout L = s3_layout(a.n1);
    unsigned char* wp = a.ws + (size_t)b * L.per_problem;
    int *cm = (int*)(wp + L.cm), *sel = (int*)(wp + L.sel), *cnt = (int*)(wp + L.cnt);
    float *X1 = (float*)(wp + L.X1), *X2 = (float*)(wp + L.X2), *P1 = (float*)(wp + L.P1), *P2 = (float*)(wp + L.P2), *hyp = (float*)(wp + L.hyp);
    const int n1 = a.n1;
    int* hdr = a.header + (size_t)b * S3_HEADER_INTS;
    int N = 0;
    for (int i = 0; i < n1; ++i)
        if (s3_corr(a, b, i, X1 + 3 * (size_t)N, X2 + 3 * (size_t)N, P1 + 2 * (size_t)N, P2 + 2 * (size_t)N)) cm[N++] = i;
    const bool few = N < 3 || N < a.min_inliers || (a.num_matches && *a.num_matches < a.min_matches);
    sel[0] = N; sel[1] = few ? 0 : geo_clamp_its(a.iters_of_N[N], a.max_iters);
    if (few) { s3_too_few_header(hdr, N); return; }
    const int its = sel[1];
    const int* draws = a.draws + (size_t)b * a.draws_stride;
    int winner = -1, best_key = -1;
    for (int it = 0; it < its; ++it) {
        int set[3]; float p1[9], p2[9];
        geo_set<3>(draws + 3 * (size_t)it, a.rand_max, N, set);
        for (int j = 0; j < 3; ++j)
            for (int c = 0; c < 3; ++c) { p1[3 * j + c] = X1[3 * (size_t)set[j] + c]; p2[3 * j + c] = X2[3 * (size_t)set[j] + c]; }
        float* h = hyp + (size_t)it * S3_HYP;
        s3_horn(p1, p2, a.fix_scale != 0, h);
        int c = 0;
        for (int k = 0; k < N; ++k) {
            float err[2];
            c += s3_check(h + S3_F_T12, h + S3_F_T21, a.cam1, a.cam2, X1 + 3 * (size_t)k, X2 + 3 * (size_t)k, P1 + 2 * (size_t)k, P2 + 2 * (size_t)k, a.max_err1, a.max_err2, err);
        }
        cnt[it] = c;
        if (winner < 0 && c > a.min_inliers) winner = it;
        const int key = s3_best_key(c, it);
        if (key > best_key) best_key = key;
    }
    const int best = winner >= 0 ? winner : best_key % S3_MAX_ITERS;
    const float* h = hyp + (size_t)best * S3_HYP;
    float* fo = a.fout + (size_t)b * S3_FLOATS;
    for (int k = 0; k < S3_FLOATS; ++k) fo[k] = k < S3_F_T21 ? h[k] : 0.0f;
    for (int i = 0; i < n1; ++i) a.inliers[(size_t)b * n1 + i] = 0;
    if (winner >= 0) {
        for (int k = 0; k < N; ++k) {
            float err[2];
            a.inliers[(size_t)b * n1 + cm[k]] = (unsigned char)s3_check(h + S3_F_T12, h + S3_F_T21, a.cam1, a.cam2, X1 + 3 * (size_t)k, X2 + 3 * (size_t)k, P1 + 2 * (size_t)k,
                                                                       P2 + 2 * (size_t)k, a.max_err1, a.max_err2, err);
        }
        s3_compose(h, a.T2w + (size_t)b * 12, a.Tcw + (size_t)b * 12, a.Ow + (size_t)b * 3);
    }
    for (int k = 0; k < S3_HEADER_INTS; ++k) hdr[k] = 0;
    hdr[S3_H_N] = N; hdr[S3_H_STATUS] = winner >= 0 ? S3_CONVERGED : S3_NO_MORE; hdr[S3_H_ITS] = its; hdr[S3_H_WINNER] = winner;
    hdr[S3_H_NINL] = winner >= 0 ? cnt[winner] : 0; hdr[S3_H_BEST] = best; hdr[S3_H_BEST_COUNT] = cnt[best]; hdr[S3_H_CONSUMED] = winner >= 0 ? winner + 1 : its;
}

// ---- the merge of LoopClosing.cc:670-687 in its order-free form ------------------------------------------------------------------------------------------
struct S3MergeArgs { int J, n1, n2, M; const int *match12, *point2; int *owner, *matched, *matched_kf, *num; };
// the row of entry (j, k): the map point of covisible j at the keypoint the BoW search matched to slot k of the current keyframe, or -1
XFH_HD int s3_merge_row(const int* match12, const int* point2, int n1, int n2, int M, int j, int k) {
    const int m = match12[(size_t)j * n1 + k];
    if (m < 0 || m >= n2) return -1;
    const int r = point2[(size_t)j * n2 + m];
    return s3_row_ok(r, M) ? r : -1;
}
// slot k from the finished owner table: the owner entry with the largest j; returns the number of owners among the slot's J entries
XFH_HD int s3_merge_slot(const int* match12, const int* point2, const int* owner, int J, int n1, int n2, int M, int k, int* matched, int* kf) {
    int owners = 0, row_out = -1, j_out = -1;
    for (int j = 0; j < J; ++j) {
        const int r = s3_merge_row(match12, point2, n1, n2, M, j, k);
        if (r >= 0 && owner[r] == j * n1 + k) { ++owners; row_out = r; j_out = j; }
    }
    *matched = row_out; *kf = j_out;
    return owners;
}
inline void s3_merge_host(int J, int n1, int n2, int M, const int* match12, const int* point2, int* owner, int* matched, int* matched_kf, int* num) {
    for (int r = 0; r < M; ++r) owner[r] = INT_MAX;
    for (int j = 0; j < J; ++j)
        for (int k = 0; k < n1; ++k) {
            const int r = s3_merge_row(match12, point2, n1, n2, M, j, k);
            if (r >= 0 && j * n1 + k < owner[r]) owner[r] = j * n1 + k;
        }
    int total = 0;
    for (int k = 0; k < n1; ++k) total += s3_merge_slot(match12, point2, owner, J, n1, n2, M, k, matched + k, matched_kf + k);
    *num = total;
}
