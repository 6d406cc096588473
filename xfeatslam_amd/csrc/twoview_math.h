// twoview_math.h -- the rule of xfh_two_view_device, written ONCE for host and device (XFH_HD): TwoViewReconstruction::Reconstruct
// (src/TwoViewReconstruction.cc) for the Pinhole camera: the compact match list, the minimal sets from the caller's raw draws, Normalize,
// ComputeH21 / ComputeF21, CheckHomography / CheckFundamental, the argmax, ReconstructH / ReconstructF with DecomposeE, and CheckRT.
// The contract is in include/xfeat_hip.h, line by line; the kernels of twoview.hip.h, the host entry points of capi_twoview.cpp (the
// single-thread form of the whole rule, xfh_two_view_host, included) and tests/cpp/asan_twoview_test.cpp compile these very lines.
// All arithmetic is fp32 in the order written (the library is built with -ffp-contract=off) except where a double is spelled out.
#pragma once
#include "geom_common.h"
#include "triangulate_math.h"
#include <math.h>
#include <stdint.h>
#include <stddef.h>

enum { TV_TOO_FEW = 0, TV_BOTH_ZERO = 1, TV_H_DEGENERATE = 2, TV_F_NO_WINNER = 3, TV_H_GATES = 4, TV_LOW_PARALLAX = 5, TV_OK_H = 6, TV_OK_F = 7 };
enum { TV_MODEL_NONE = 0, TV_MODEL_H = 1, TV_MODEL_F = 2 };
enum { TV_H_N = 0, TV_H_STATUS = 1, TV_H_MODEL = 2, TV_H_WIN_H = 3, TV_H_WIN_F = 4, TV_H_NGOOD = 5, TV_H_CHOSEN = 13, TV_H_INL_H = 14, TV_H_INL_F = 15,
       TV_H_NTRI = 16, TV_H_NHYP = 17, TV_H_NMATCHES = 18, TV_HEADER_INTS = 24 };
enum { TV_F_SH = 0, TV_F_SF = 1, TV_F_RH = 2, TV_F_H21 = 3, TV_F_F21 = 12, TV_F_T21 = 21, TV_F_COS = 33, TV_FLOATS = 48 };
#define TV_MAX_ITERS 4096
#define TV_MIN_SET 8                  // the minimal set of one iteration: geo_set on eight raw draws.  N >= 8.

// Normalize (:737-784) of one frame from its two passes: mean = sum / n, s = 1 / (sum |x - mean| / n)
XFH_HD float tv_mean(float sum, int n) { return sum / (float)n; }
XFH_HD float tv_inv_dev(float sum_dev, int n) { const float md = sum_dev / (float)n; return (float)(1.0 / (double)md); }
// nrm = (meanX, meanY, sX, sY)
XFH_HD void tv_normalized(const float* nrm, float x, float y, float* o) { o[0] = (x - nrm[0]) * nrm[2]; o[1] = (y - nrm[1]) * nrm[3]; }

// ---- the fp64 one-sided Jacobi (geo_jacobi) for the M x N matrices of the rule, rows cached: a column pair is read from LDS once ---------------------
XFH_HD void tv_jacobi(const GeoMat& U, const GeoMat& V, int M, int N) {
    if (M == 16) geo_jacobi<16>(U, V, N); else if (M == 8) geo_jacobi<8>(U, V, N); else geo_jacobi<3>(U, V, N);     // the three instances of the rule
}

// ---- the two fits of eight normalised point pairs (p1, p2: [8][2]); U has room for 16 x 9 doubles, V for 9 x 9 -------------------------------------
// ComputeH21 (:232-272): V's column of the least singular value of the 16 x 9 A, row-major 3 x 3, rounded to float once
XFH_HD void tv_fit_h(const float* p1, const float* p2, const GeoMat& U, const GeoMat& V, float* Hn) {
    for (int i = 0; i < 8; ++i) {
        const float u1 = p1[2 * i], v1 = p1[2 * i + 1], u2 = p2[2 * i], v2 = p2[2 * i + 1];
        const float r0[9] = {0.0f, 0.0f, 0.0f, -u1, -v1, -1.0f, v2 * u1, v2 * v1, v2};
        const float r1[9] = {u1, v1, 1.0f, 0.0f, 0.0f, 0.0f, -u2 * u1, -u2 * v1, -u2};
        for (int c = 0; c < 9; ++c) { U((2 * i) * 9 + c) = (double)r0[c]; U((2 * i + 1) * 9 + c) = (double)r1[c]; }
    }
    tv_jacobi(U, V, 16, 9);
    const int k = geo_min_col(U, 16, 9, false);
    for (int c = 0; c < 9; ++c) Hn[c] = (float)V(c * 9 + k);
}
// ComputeF21 (:274-308): the null vector of the 8 x 9 A as above, then the rank-2 projection: the 3 x 3 Jacobi of Fpre gives the columns
// a_i = sigma_i u_i of Fpre V; Fn = a_i0 v_i0^T + a_i1 v_i1^T over the two columns of largest norm, in double, rounded to float once
XFH_HD void tv_fit_f(const float* p1, const float* p2, const GeoMat& U, const GeoMat& V, float* Fn) {
    for (int i = 0; i < 8; ++i) {
        const float u1 = p1[2 * i], v1 = p1[2 * i + 1], u2 = p2[2 * i], v2 = p2[2 * i + 1];
        const float r0[9] = {u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.0f};
        for (int c = 0; c < 9; ++c) U(i * 9 + c) = (double)r0[c];
    }
    tv_jacobi(U, V, 8, 9);
    const int k = geo_min_col(U, 8, 9, false);
    float f[9];
    for (int c = 0; c < 9; ++c) f[c] = (float)V(c * 9 + k);
    for (int c = 0; c < 9; ++c) U(c) = (double)f[c];
    tv_jacobi(U, V, 3, 3);
    int o[3]; double n2[3];
    geo_order3(U, o, n2);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Fn[r * 3 + c] = (float)(U(r * 3 + o[0]) * V(c * 3 + o[0]) + U(r * 3 + o[1]) * V(c * 3 + o[1]));
}

// M = X * T with T = [sX 0 -meanX*sX; 0 sY -meanY*sY; 0 0 1] (the products with T's zeros are not formed)
XFH_HD void tv_times_T(const float* X, const float* nrm, float* M) {
    const float tx = -nrm[0] * nrm[2], ty = -nrm[1] * nrm[3];
    for (int r = 0; r < 3; ++r) {
        M[r * 3] = X[r * 3] * nrm[2]; M[r * 3 + 1] = X[r * 3 + 1] * nrm[3];
        M[r * 3 + 2] = (X[r * 3] * tx + X[r * 3 + 1] * ty) + X[r * 3 + 2];
    }
}
XFH_HD void tv_inv3(const float* A, float* I) {
    const float id = 1.0f / geo_det3(A);
    I[0] = (A[4] * A[8] - A[5] * A[7]) * id; I[1] = (A[2] * A[7] - A[1] * A[8]) * id; I[2] = (A[1] * A[5] - A[2] * A[4]) * id;
    I[3] = (A[5] * A[6] - A[3] * A[8]) * id; I[4] = (A[0] * A[8] - A[2] * A[6]) * id; I[5] = (A[2] * A[3] - A[0] * A[5]) * id;
    I[6] = (A[3] * A[7] - A[4] * A[6]) * id; I[7] = (A[1] * A[6] - A[0] * A[7]) * id; I[8] = (A[0] * A[4] - A[1] * A[3]) * id;
}
// H21i = T2inv * Hn * T1 with T2inv = [1/sX 0 meanX; 0 1/sY meanY; 0 0 1] written out, H12i = its cofactor inverse: out[0..9) = H21i, out[9..18) = H12i
XFH_HD void tv_compose_h(const float* Hn, const float* nrm1, const float* nrm2, float* out) {
    float M[9];
    tv_times_T(Hn, nrm1, M);
    const float ix = 1.0f / nrm2[2], iy = 1.0f / nrm2[3];
    for (int c = 0; c < 3; ++c) {
        out[c] = ix * M[c] + nrm2[0] * M[6 + c]; out[3 + c] = iy * M[3 + c] + nrm2[1] * M[6 + c]; out[6 + c] = M[6 + c];
    }
    tv_inv3(out, out + 9);
}
// F21i = T2^T * Fn * T1: out[0..9), out[9..18) = 0
XFH_HD void tv_compose_f(const float* Fn, const float* nrm1, const float* nrm2, float* out) {
    float M[9];
    tv_times_T(Fn, nrm1, M);
    const float tx = -nrm2[0] * nrm2[2], ty = -nrm2[1] * nrm2[3];
    for (int c = 0; c < 3; ++c) {
        out[c] = nrm2[2] * M[c]; out[3 + c] = nrm2[3] * M[3 + c]; out[6 + c] = (tx * M[c] + ty * M[3 + c]) + M[6 + c];
        out[9 + c] = 0.0f; out[12 + c] = 0.0f; out[15 + c] = 0.0f;
    }
}

// ---- the score terms of one match (:310-473) --------------------------------------------------------------------------------------------------
XFH_HD float tv_inv_sigma2(float sigma) { return (float)(1.0 / (double)(sigma * sigma)); }
// CheckHomography: chi[0] = chiSquare1 (x2 into image 1 by H12), chi[1] = chiSquare2; returns the match's share of the score, *in = bIn
XFH_HD float tv_score_h(const float* H, float inv_s2, float u1, float v1, float u2, float v2, float* chi, int* in) {
    const float* G = H + 9;
    const float w2 = (float)(1.0 / (double)((G[6] * u2 + G[7] * v2) + G[8]));
    const float a = ((G[0] * u2 + G[1] * v2) + G[2]) * w2, b = ((G[3] * u2 + G[4] * v2) + G[5]) * w2;
    chi[0] = ((u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)) * inv_s2;
    const float w1 = (float)(1.0 / (double)((H[6] * u1 + H[7] * v1) + H[8]));
    const float c = ((H[0] * u1 + H[1] * v1) + H[2]) * w1, d = ((H[3] * u1 + H[4] * v1) + H[5]) * w1;
    chi[1] = ((u2 - c) * (u2 - c) + (v2 - d) * (v2 - d)) * inv_s2;
    const float th = 5.991f;
    const bool o1 = chi[0] > th, o2 = chi[1] > th;
    *in = !o1 && !o2;
    return (o1 ? 0.0f : th - chi[0]) + (o2 ? 0.0f : th - chi[1]);
}
// CheckFundamental: chi[0] = the distance to l2 = F21 x1 in image 2, chi[1] = to l1 = x2^T F21 in image 1
XFH_HD float tv_score_f(const float* F, float inv_s2, float u1, float v1, float u2, float v2, float* chi, int* in) {
    const float a2 = (F[0] * u1 + F[1] * v1) + F[2], b2 = (F[3] * u1 + F[4] * v1) + F[5], c2 = (F[6] * u1 + F[7] * v1) + F[8];
    const float num2 = (a2 * u2 + b2 * v2) + c2;
    chi[0] = ((num2 * num2) / (a2 * a2 + b2 * b2)) * inv_s2;
    const float a1 = (F[0] * u2 + F[3] * v2) + F[6], b1 = (F[1] * u2 + F[4] * v2) + F[7], c1 = (F[2] * u2 + F[5] * v2) + F[8];
    const float num1 = (a1 * u1 + b1 * v1) + c1;
    chi[1] = ((num1 * num1) / (a1 * a1 + b1 * b1)) * inv_s2;
    const float th = 3.841f, ts = 5.991f;
    const bool o1 = chi[0] > th, o2 = chi[1] > th;
    *in = !o1 && !o2;
    return (o1 ? 0.0f : ts - chi[0]) + (o2 ? 0.0f : ts - chi[1]);
}
XFH_HD float tv_score(int model, const float* M, float inv_s2, float u1, float v1, float u2, float v2, float* chi, int* in) {
    return model == TV_MODEL_H ? tv_score_h(M, inv_s2, u1, v1, u2, v2, chi, in) : tv_score_f(M, inv_s2, u1, v1, u2, v2, chi, in);
}
// the argmax of FindHomography / FindFundamental: the first iteration with the highest score; a score that is not > 0 (a NaN included) never wins
XFH_HD int tv_argmax(const float* score, int iters, float* best) {
    int w = -1; float s = 0.0f;
    for (int it = 0; it < iters; ++it) if (score[it] > s) { s = score[it]; w = it; }
    *best = s;
    return w;
}

// ---- the 3 x 3 SVD of the motion recovery -----------------------------------------------------------------------------------------------------
// A = U diag(w) V^T from the Jacobi: the columns by norm, descending; w_i = sqrt |a_i|^2, u_i = a_i / w_i in double.  rank2 (DecomposeE): u_2 is
// not a_2 / w_2 (w_2 is 0 up to rounding) but the cross product u_0 x u_1.  U, V (row-major, columns in the sorted order), w rounded to float once.
struct TvSvd3 { float U[9], V[9], w[3]; };
XFH_HD void tv_svd3(const float* A, bool rank2, const GeoMat& U, const GeoMat& V, TvSvd3* o) {
    for (int k = 0; k < 9; ++k) U(k) = (double)A[k];
    tv_jacobi(U, V, 3, 3);
    int ord[3]; double n2[3], u[9];
    geo_order3(U, ord, n2);
    for (int k = 0; k < 3; ++k) {
        const double w = sqrt(n2[ord[k]]);
        o->w[k] = (float)w;
        for (int r = 0; r < 3; ++r) { u[r * 3 + k] = U(r * 3 + ord[k]) / w; o->V[r * 3 + k] = (float)V(r * 3 + ord[k]); }
    }
    if (rank2) {
        u[2] = u[3] * u[7] - u[6] * u[4];
        u[5] = u[6] * u[1] - u[0] * u[7];
        u[8] = u[0] * u[4] - u[3] * u[1];
    }
    for (int k = 0; k < 9; ++k) o->U[k] = (float)u[k];
}
XFH_HD void tv_times_K(const float* X, const GeoCam& k, float* G) {
    for (int r = 0; r < 3; ++r) {
        G[r * 3] = X[r * 3] * k.fx; G[r * 3 + 1] = X[r * 3 + 1] * k.fy; G[r * 3 + 2] = (X[r * 3] * k.cx + X[r * 3 + 1] * k.cy) + X[r * 3 + 2];
    }
}
XFH_HD void tv_unit3(const float* t, float* o) {
    const float n = sqrtf((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
    o[0] = t[0] / n; o[1] = t[1] / n; o[2] = t[2] / n;
}
// ReconstructF's four hypotheses (:483-503, DecomposeE :903-927): E = K^T F K, (R1, t) (R2, t) (R1, -t) (R2, -t) as rows [R|t] of Rt[4][12]
XFH_HD void tv_motions_f(const float* F, const GeoCam& k, const GeoMat& U, const GeoMat& V, float* Rt) {
    float G[9], E[9];
    tv_times_K(F, k, G);
    for (int c = 0; c < 3; ++c) { E[c] = k.fx * G[c]; E[3 + c] = k.fy * G[3 + c]; E[6 + c] = (k.cx * G[c] + k.cy * G[3 + c]) + G[6 + c]; }
    TvSvd3 s;
    tv_svd3(E, true, U, V, &s);
    const float t0[3] = {s.U[2], s.U[5], s.U[8]};
    float t[3], R1[9], R2[9];
    tv_unit3(t0, t);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            R1[r * 3 + c] = (s.U[r * 3 + 1] * s.V[c * 3] - s.U[r * 3] * s.V[c * 3 + 1]) + s.U[r * 3 + 2] * s.V[c * 3 + 2];
            R2[r * 3 + c] = (s.U[r * 3] * s.V[c * 3 + 1] - s.U[r * 3 + 1] * s.V[c * 3]) + s.U[r * 3 + 2] * s.V[c * 3 + 2];
        }
    const bool n1 = geo_det3(R1) < 0.0f, n2 = geo_det3(R2) < 0.0f;
    for (int h = 0; h < 4; ++h) {
        const float* R = (h & 1) ? R2 : R1;
        const bool neg = (h & 1) ? n2 : n1;
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) Rt[h * 12 + r * 4 + c] = neg ? -R[r * 3 + c] : R[r * 3 + c];
            Rt[h * 12 + r * 4 + 3] = h < 2 ? t[r] : -t[r];
        }
    }
}
// ReconstructH's eight hypotheses (:582-690): A = K^-1 H K with K^-1 = [1/fx 0 -cx/fx; 0 1/fy -cy/fy; 0 0 1] written out.  false: d1/d2 or
// d2/d3 < 1.00001 (nothing is written).
XFH_HD bool tv_motions_h(const float* H, const GeoCam& k, const GeoMat& Um, const GeoMat& Vm, float* Rt) {
    float G[9], A[9];
    tv_times_K(H, k, G);
    const float ifx = 1.0f / k.fx, ify = 1.0f / k.fy, icx = -k.cx * ifx, icy = -k.cy * ify;
    for (int c = 0; c < 3; ++c) { A[c] = ifx * G[c] + icx * G[6 + c]; A[3 + c] = ify * G[3 + c] + icy * G[6 + c]; A[6 + c] = G[6 + c]; }
    TvSvd3 sv;
    tv_svd3(A, false, Um, Vm, &sv);
    const float* U = sv.U; const float* V = sv.V;
    const float s = geo_det3(U) * geo_det3(V);
    const float d1 = sv.w[0], d2 = sv.w[1], d3 = sv.w[2];
    if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) return false;
    const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)), aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    const float x1[4] = {aux1, aux1, -aux1, -aux1}, x3[4] = {aux3, -aux3, aux3, -aux3};
    const float root = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3));
    const float ast = root / ((d1 + d3) * d2), ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
    const float asp = root / ((d1 - d3) * d2), cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
    const float sgn[4] = {1.0f, -1.0f, -1.0f, 1.0f};
    for (int h = 0; h < 8; ++h) {
        const int i = h & 3;
        const bool second = h >= 4;
        const float sn = sgn[i] * (second ? asp : ast);
        float X[9], tp0, tp2;
        for (int r = 0; r < 3; ++r) {
            if (!second) { X[r * 3] = U[r * 3] * ct + U[r * 3 + 2] * sn; X[r * 3 + 1] = U[r * 3 + 1]; X[r * 3 + 2] = U[r * 3 + 2] * ct - U[r * 3] * sn; }
            else { X[r * 3] = U[r * 3] * cp + U[r * 3 + 2] * sn; X[r * 3 + 1] = -U[r * 3 + 1]; X[r * 3 + 2] = U[r * 3] * sn - U[r * 3 + 2] * cp; }
        }
        if (!second) { tp0 = x1[i] * (d1 - d3); tp2 = -x3[i] * (d1 - d3); } else { tp0 = x1[i] * (d1 + d3); tp2 = x3[i] * (d1 + d3); }
        float t[3], tn[3];
        for (int r = 0; r < 3; ++r) t[r] = U[r * 3] * tp0 + U[r * 3 + 2] * tp2;
        tv_unit3(t, tn);
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) Rt[h * 12 + r * 4 + c] = s * ((X[r * 3] * V[c * 3] + X[r * 3 + 1] * V[c * 3 + 1]) + X[r * 3 + 2] * V[c * 3 + 2]);
            Rt[h * 12 + r * 4 + 3] = tn[r];
        }
    }
    return true;
}

// ---- CheckRT (:786-901) for one inlier pair: 0 = not counted, 1 = counted (nGood, vCosParallax, vP3D), 2 = counted and vbGood -------------------
XFH_HD float tv_th2(float sigma) { return (float)(4.0 * (double)(sigma * sigma)); }
XFH_HD int tv_check_rt_pair(const GeoCam& k, const float* Rt, float th2, float x1, float y1, float x2, float y2, float* cosp, float* p) {
    float A[4][4], P2[3][4];
    for (int c = 0; c < 4; ++c) {
        P2[0][c] = k.fx * Rt[c] + k.cx * Rt[8 + c]; P2[1][c] = k.fy * Rt[4 + c] + k.cy * Rt[8 + c]; P2[2][c] = Rt[8 + c];
    }
    const float P1[3][4] = {{k.fx, 0.0f, k.cx, 0.0f}, {0.0f, k.fy, k.cy, 0.0f}, {0.0f, 0.0f, 1.0f, 0.0f}};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        A[0][c] = x1 * P1[2][c] - P1[0][c]; A[1][c] = y1 * P1[2][c] - P1[1][c];
        A[2][c] = x2 * P2[2][c] - P2[0][c]; A[3][c] = y2 * P2[2][c] - P2[1][c];
    }
    double xh[4];
    triang_null_vector(A, xh);
    const float h[4] = {(float)xh[0], (float)xh[1], (float)xh[2], (float)xh[3]};
    p[0] = h[0] / h[3]; p[1] = h[1] / h[3]; p[2] = h[2] / h[3];
    *cosp = 0.0f;
    if (!isfinite(p[0]) || !isfinite(p[1]) || !isfinite(p[2])) return 0;
    float O2[3], n2[3];
    for (int c = 0; c < 3; ++c) { O2[c] = -((Rt[c] * Rt[3] + Rt[4 + c] * Rt[7]) + Rt[8 + c] * Rt[11]); n2[c] = p[c] - O2[c]; }
    const float dist1 = sqrtf(triang_dot3(p[0], p[1], p[2], p[0], p[1], p[2])), dist2 = sqrtf(triang_dot3(n2[0], n2[1], n2[2], n2[0], n2[1], n2[2]));
    const float cosv = triang_dot3(p[0], p[1], p[2], n2[0], n2[1], n2[2]) / (dist1 * dist2);
    *cosp = cosv;
    const bool parallax = (double)cosv < 0.99998;
    if (p[2] <= 0.0f && parallax) return 0;
    const float q0 = triang_dot3(Rt[0], Rt[1], Rt[2], p[0], p[1], p[2]) + Rt[3], q1 = triang_dot3(Rt[4], Rt[5], Rt[6], p[0], p[1], p[2]) + Rt[7],
                q2 = triang_dot3(Rt[8], Rt[9], Rt[10], p[0], p[1], p[2]) + Rt[11];
    if (q2 <= 0.0f && parallax) return 0;
    const float iz1 = (float)(1.0 / (double)p[2]);
    const float e1x = (k.fx * p[0] * iz1 + k.cx) - x1, e1y = (k.fy * p[1] * iz1 + k.cy) - y1;
    if (e1x * e1x + e1y * e1y > th2) return 0;
    const float iz2 = (float)(1.0 / (double)q2);
    const float e2x = (k.fx * q0 * iz2 + k.cx) - x2, e2y = (k.fy * q1 * iz2 + k.cy) - y2;
    if (e2x * e2x + e2y * e2y > th2) return 0;
    return parallax ? 2 : 1;
}
// a float as an unsigned key of the same order (by value; -0 before +0, NaNs by their bits at the two ends)
XFH_HD uint32_t tv_float_key(float f) {
    union { float f; uint32_t u; } v; v.f = f;
    return (v.u & 0x80000000u) ? ~v.u : (v.u | 0x80000000u);
}
XFH_HD float tv_key_float(uint32_t k) {
    union { float f; uint32_t u; } v; v.u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return v.f;
}

// ---- the decision (:113-128, :505-568, :693-733) from the counts: status, and *chosen = the winning hypothesis or -1 ----------------------------
// cosv[h] = the cosine at sorted index min(50, nGood - 1), 1.0f (0 degrees) with nGood = 0; "parallax > minParallax" is cos < min_parallax_cos
XFH_HD int tv_decide(int model, bool h_degenerate, const int* nGood, const float* cosv, int n_inliers, double min_parallax_cos, int min_tri, int* chosen) {
    *chosen = -1;
    if (model == TV_MODEL_F) {
        int maxGood = nGood[0];
        for (int h = 1; h < 4; ++h) maxGood = nGood[h] > maxGood ? nGood[h] : maxGood;
        const int n09 = (int)(0.9 * (double)n_inliers), nMinGood = n09 > min_tri ? n09 : min_tri;
        int nsimilar = 0;
        for (int h = 0; h < 4; ++h) nsimilar += (double)nGood[h] > 0.7 * (double)maxGood;
        if (maxGood < nMinGood || nsimilar > 1) return TV_F_NO_WINNER;
        int h = 0;
        while (nGood[h] != maxGood) ++h;
        if ((double)cosv[h] < min_parallax_cos) { *chosen = h; return TV_OK_F; }
        return TV_LOW_PARALLAX;
    }
    if (h_degenerate) return TV_H_DEGENERATE;
    int best = 0, second = 0, idx = -1;
    for (int h = 0; h < 8; ++h) {
        if (nGood[h] > best) { second = best; best = nGood[h]; idx = h; }
        else if (nGood[h] > second) second = nGood[h];
    }
    const bool counts = (double)second < 0.75 * (double)best && best > min_tri && (double)best > 0.9 * (double)n_inliers;
    if (!counts || idx < 0) return TV_H_GATES;
    if (!((double)cosv[idx] <= min_parallax_cos)) return TV_LOW_PARALLAX;
    *chosen = idx;
    return TV_OK_H;
}

// ---- the workspace of one call (device memory, B problems): offsets in bytes, every piece 16-byte aligned ----------------------------------------
struct TvLayout { size_t cm1, cm2, nrm, sel, hyp, score, motion, ngood, cosk, verdict, cosv, p3d, per_problem; };
XFH_HD TvLayout tv_layout(int n1, int iters) {
    TvLayout L; size_t o = 0;
    L.cm1 = o; o += geo_al16((size_t)n1 * 4);                 // int idx1 of compact match k
    L.cm2 = o; o += geo_al16((size_t)n1 * 4);                 // int idx2
    L.nrm = o; o += 32;                                      // float (meanX, meanY, sX, sY) of frame 1, of frame 2
    L.sel = o; o += 32;                                      // int N, winH, winF, model, inliers of the model, h_degenerate, nhyp, 0
    L.hyp = o; o += (size_t)2 * iters * 18 * 4;              // float [2][iters][18]
    L.score = o; o += geo_al16((size_t)2 * iters * 4);        // float [2][iters]
    L.motion = o; o += 8 * 12 * 4;                           // float [8][12]
    L.ngood = o; o += 32;                                    // int [8]
    L.cosk = o; o += 32;                                     // float [8]
    L.verdict = o; o += geo_al16((size_t)8 * n1);             // u8 [8][n1]
    L.cosv = o; o += geo_al16((size_t)8 * n1 * 4);            // float [8][n1]
    L.p3d = o; o += geo_al16((size_t)8 * n1 * 12);            // float [8][n1][3]
    L.per_problem = geo_al16(o);
    return L;
}
enum { TV_S_N = 0, TV_S_WIN_H = 1, TV_S_WIN_F = 2, TV_S_MODEL = 3, TV_S_NINL = 4, TV_S_HDEG = 5, TV_S_NHYP = 6 };

// ---- the argument block of the kernels (twoview.hip.h), filled by capi_twoview.cpp ------------------------------------------------------------------
struct TvArgs {
    int B, n1, n2, iters, rand_max, min_tri;
    size_t draws_stride;
    GeoCam cam;
    float sigma;
    double min_parallax_cos;
    const float *xy1, *xy2;
    const int *match12, *draws;
    unsigned char* ws;
    int* header; float* fout;
    unsigned char *inl_h, *inl_f, *tri;
    float* p3d; int* matches_out;
};
XFH_HD bool tv_match_ok(int m, int n2) { return m >= 0 && m < n2; }

// ---- the whole rule for problem b on ONE host thread, over host pointers in the same argument block and workspace layout as the kernels ------------
// (xfh_two_view_host and tests/cpp/asan_twoview_test.cpp; the kernels of twoview.hip.h do these steps with 256 lanes)
inline float tv_host_sum(const float* term, int n) {
    float s[GEO_LANES];
    for (int l = 0; l < GEO_LANES; ++l) { float acc = 0.0f; for (int i = l; i < n; i += GEO_LANES) acc = acc + term[i]; s[l] = acc; }
    return geo_tree_fold(s);
}
inline void tv_host_problem(const TvArgs& a, int b, float* scratch /* max(n1, n2) floats */) {
    const TvLayout L = tv_layout(a.n1, a.iters);
    unsigned char* wp = a.ws + (size_t)b * L.per_problem;
    int *cm1 = (int*)(wp + L.cm1), *cm2 = (int*)(wp + L.cm2), *sel = (int*)(wp + L.sel), *ngood = (int*)(wp + L.ngood);
    float *nrm = (float*)(wp + L.nrm), *hyp = (float*)(wp + L.hyp), *score = (float*)(wp + L.score), *motion = (float*)(wp + L.motion);
    float *cosk = (float*)(wp + L.cosk), *cosv = (float*)(wp + L.cosv), *p3d = (float*)(wp + L.p3d);
    unsigned char* verdict = wp + L.verdict;
    const int n1 = a.n1, n2 = a.n2;
    const float* xy1 = a.xy1 + (size_t)b * n1 * 2;
    const float* xy2 = a.xy2 + (size_t)b * n2 * 2;
    const int* m12 = a.match12 + (size_t)b * n1;
    int* hdr = a.header + (size_t)b * TV_HEADER_INTS;
    float* fo = a.fout + (size_t)b * TV_FLOATS;
    int N = 0;
    for (int i = 0; i < n1; ++i) if (tv_match_ok(m12[i], n2)) { cm1[N] = i; cm2[N] = m12[i]; ++N; }
    if (N < 8) {
        for (int k = 0; k < TV_HEADER_INTS; ++k) hdr[k] = k == TV_H_N ? N : (k == TV_H_STATUS ? TV_TOO_FEW : (k == TV_H_WIN_H || k == TV_H_WIN_F || k == TV_H_CHOSEN ? -1 : 0));
        return;
    }
    for (int f = 0; f < 2; ++f) {
        const int n = f ? n2 : n1;
        const float* xy = f ? xy2 : xy1;
        for (int d = 0; d < 2; ++d) {
            for (int i = 0; i < n; ++i) scratch[i] = xy[2 * (size_t)i + d];
            const float mean = tv_mean(tv_host_sum(scratch, n), n);
            for (int i = 0; i < n; ++i) scratch[i] = fabsf(xy[2 * (size_t)i + d] - mean);
            nrm[4 * f + d] = mean; nrm[4 * f + 2 + d] = tv_inv_dev(tv_host_sum(scratch, n), n);
        }
    }
    const float inv_s2 = tv_inv_sigma2(a.sigma);
    double um[144], vm[81];
    const GeoMat U{um, 1}, V{vm, 1};
    for (int model = TV_MODEL_H; model <= TV_MODEL_F; ++model)
        for (int it = 0; it < a.iters; ++it) {
            int set[8]; float p1[16], p2[16], M[9];
            geo_set<TV_MIN_SET>(a.draws + (size_t)b * a.draws_stride + (size_t)it * 8, a.rand_max, N, set);
            for (int j = 0; j < 8; ++j) {
                const int i1 = cm1[set[j]], i2 = cm2[set[j]];
                tv_normalized(nrm, xy1[2 * (size_t)i1], xy1[2 * (size_t)i1 + 1], p1 + 2 * j);
                tv_normalized(nrm + 4, xy2[2 * (size_t)i2], xy2[2 * (size_t)i2 + 1], p2 + 2 * j);
            }
            float* out = hyp + ((size_t)(model - 1) * a.iters + it) * 18;
            if (model == TV_MODEL_H) { tv_fit_h(p1, p2, U, V, M); tv_compose_h(M, nrm, nrm + 4, out); }
            else { tv_fit_f(p1, p2, U, V, M); tv_compose_f(M, nrm, nrm + 4, out); }
            for (int k = 0; k < N; ++k) {
                float chi[2]; int in;
                scratch[k] = tv_score(model, out, inv_s2, xy1[2 * (size_t)cm1[k]], xy1[2 * (size_t)cm1[k] + 1], xy2[2 * (size_t)cm2[k]], xy2[2 * (size_t)cm2[k] + 1], chi, &in);
            }
            score[(size_t)(model - 1) * a.iters + it] = tv_host_sum(scratch, N);
        }
    float SH, SF;
    const int winH = tv_argmax(score, a.iters, &SH), winF = tv_argmax(score + a.iters, a.iters, &SF);
    float MH[18], MF[9];
    for (int k = 0; k < 18; ++k) MH[k] = winH >= 0 ? hyp[(size_t)winH * 18 + k] : 0.0f;
    for (int k = 0; k < 9; ++k) MF[k] = winF >= 0 ? hyp[((size_t)a.iters + winF) * 18 + k] : 0.0f;
    int cH = 0, cF = 0;
    for (int i = 0; i < n1; ++i) {
        const int m = m12[i];
        int inH = 0, inF = 0;
        if (tv_match_ok(m, n2)) {
            float chi[2];
            if (winH >= 0) tv_score_h(MH, inv_s2, xy1[2 * (size_t)i], xy1[2 * (size_t)i + 1], xy2[2 * (size_t)m], xy2[2 * (size_t)m + 1], chi, &inH);
            if (winF >= 0) tv_score_f(MF, inv_s2, xy1[2 * (size_t)i], xy1[2 * (size_t)i + 1], xy2[2 * (size_t)m], xy2[2 * (size_t)m + 1], chi, &inF);
        }
        a.inl_h[(size_t)b * n1 + i] = (unsigned char)inH; a.inl_f[(size_t)b * n1 + i] = (unsigned char)inF;
        cH += inH; cF += inF;
    }
    for (int k = 0; k < TV_FLOATS; ++k) fo[k] = 0.0f;
    fo[TV_F_SH] = SH; fo[TV_F_SF] = SF;
    for (int k = 0; k < 9; ++k) { fo[TV_F_H21 + k] = MH[k]; fo[TV_F_F21 + k] = MF[k]; }
    int model = TV_MODEL_NONE, nhyp = 0, hdeg = 0;
    if (SH + SF != 0.0f) {
        const float RH = SH / (SH + SF);
        fo[TV_F_RH] = RH;
        model = (double)RH > 0.50 ? TV_MODEL_H : TV_MODEL_F;
        if (model == TV_MODEL_H) { hdeg = !tv_motions_h(MH, a.cam, U, V, motion); nhyp = hdeg ? 0 : 8; }
        else { tv_motions_f(MF, a.cam, U, V, motion); nhyp = 4; }
    }
    const int ninl = model == TV_MODEL_H ? cH : cF;
    sel[TV_S_N] = N; sel[TV_S_WIN_H] = winH; sel[TV_S_WIN_F] = winF; sel[TV_S_MODEL] = model; sel[TV_S_NINL] = ninl; sel[TV_S_HDEG] = hdeg; sel[TV_S_NHYP] = nhyp;
    const unsigned char* inl = (model == TV_MODEL_H ? a.inl_h : a.inl_f) + (size_t)b * n1;
    const float th2 = tv_th2(a.sigma);
    for (int h = 0; h < 8; ++h) {
        ngood[h] = 0; cosk[h] = 1.0f;
        if (h >= nhyp) continue;
        int cnt = 0;
        for (int i = 0; i < n1; ++i) {
            int v = 0; float c = 0.0f, p[3] = {0.0f, 0.0f, 0.0f};
            if (inl[i]) v = tv_check_rt_pair(a.cam, motion + h * 12, th2, xy1[2 * (size_t)i], xy1[2 * (size_t)i + 1], xy2[2 * (size_t)m12[i]], xy2[2 * (size_t)m12[i] + 1], &c, p);
            verdict[(size_t)h * n1 + i] = (unsigned char)v; cosv[(size_t)h * n1 + i] = c;
            for (int k = 0; k < 3; ++k) p3d[((size_t)h * n1 + i) * 3 + k] = p[k];
            cnt += v != 0;
        }
        ngood[h] = cnt;
        if (cnt > 0) {
            int k = cnt - 1 < 50 ? cnt - 1 : 50;
            uint32_t prefix = 0, mask = 0;
            for (int bit = 31; bit >= 0; --bit) {
                const uint32_t bb = 1u << bit;
                int c0 = 0;
                for (int i = 0; i < n1; ++i) { const uint32_t key = tv_float_key(cosv[(size_t)h * n1 + i]); c0 += verdict[(size_t)h * n1 + i] != 0 && (key & mask) == prefix && !(key & bb); }
                if (k >= c0) { k -= c0; prefix |= bb; }
                mask |= bb;
            }
            cosk[h] = tv_key_float(prefix);
        }
    }
    int chosen = -1;
    const int status = model == TV_MODEL_NONE ? TV_BOTH_ZERO : tv_decide(model, hdeg != 0, ngood, cosk, ninl, a.min_parallax_cos, a.min_tri, &chosen);
    int ntri = 0;
    for (int i = 0; i < n1; ++i) {
        const size_t kg = (size_t)b * n1 + i;
        int v = 0; float p[3] = {0.0f, 0.0f, 0.0f};
        if (chosen >= 0) { v = verdict[(size_t)chosen * n1 + i]; if (v) for (int k = 0; k < 3; ++k) p[k] = p3d[((size_t)chosen * n1 + i) * 3 + k]; }
        a.tri[kg] = (unsigned char)(v == 2);
        for (int k = 0; k < 3; ++k) a.p3d[3 * kg + k] = p[k];
        a.matches_out[kg] = chosen >= 0 && tv_match_ok(m12[i], n2) && v != 2 ? -1 : m12[i];
        ntri += v == 2;
    }
    for (int k = 0; k < TV_HEADER_INTS; ++k) hdr[k] = 0;
    hdr[TV_H_N] = N; hdr[TV_H_STATUS] = status; hdr[TV_H_MODEL] = model; hdr[TV_H_WIN_H] = winH; hdr[TV_H_WIN_F] = winF;
    for (int h = 0; h < 8; ++h) { hdr[TV_H_NGOOD + h] = ngood[h]; fo[TV_F_COS + h] = cosk[h]; }
    hdr[TV_H_CHOSEN] = chosen; hdr[TV_H_INL_H] = cH; hdr[TV_H_INL_F] = cF; hdr[TV_H_NTRI] = ntri; hdr[TV_H_NHYP] = nhyp; hdr[TV_H_NMATCHES] = chosen >= 0 ? ntri : N;
    if (chosen >= 0) for (int k = 0; k < 12; ++k) fo[TV_F_T21 + k] = motion[chosen * 12 + k];
}
