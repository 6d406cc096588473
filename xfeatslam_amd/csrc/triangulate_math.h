// triangulate_math.h -- the per-pair rule of xfh_triangulate_device, written ONCE for host and device (XFH_HD): the loop body of
// LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:481-710) for a conventional Pinhole keyframe pair, GeometricTools::Triangulate
// (src/GeometricTools.cc:47-66), KeyFrame::UnprojectStereo (src/KeyFrame.cc:755-772) and MapPoint::UpdateNormalAndDepth for a fresh point with
// two observations (src/MapPoint.cc:426-494).  The contract is in include/xfeat_hip.h, line by line; k_triangulate_pairs / k_triangulate_finish
// (triangulate.hip.h), xfh_triangulate_pair (capi_triangulate.cpp) and tests/cpp/asan_triangulate_test.cpp compile these very lines.
// All arithmetic is fp32 in the order written (the library is built with -ffp-contract=off) except where a double is spelled out.
#pragma once
#include "geom_common.h"
#include <math.h>

enum { TRIANG_NO_MATCH = 0, TRIANG_LOW_PARALLAX = 1, TRIANG_STEREO_NO_DEPTH = 2, TRIANG_DEGENERATE = 3, TRIANG_BEHIND1 = 4, TRIANG_BEHIND2 = 5,
       TRIANG_REPROJ1 = 6, TRIANG_REPROJ2 = 7, TRIANG_ZERO_DIST = 8, TRIANG_FAR = 9, TRIANG_SCALE = 10, TRIANG_ACCEPTED = 11, TRIANG_SUPERSEDED = 12 };

struct TriangParams {
    float fx, fy, cx, cy, invfx, invfy, bf, mb;        // invfx = 1.0f / fx (Frame.cc), mb = bf / fx
    float sigma2, ratio_factor, scale_last, far_th;
    int inertial;
};
// one keypoint of a pair with its keyframe: xy = mvKeysUn, raw = mvKeys[i].pt, ur = mvuRight, depth = mvDepth, T = Tcw row-major [R|t], Ow
struct TriangObs { float x, y, xr, yr, ur, depth; const float* T; const float* Ow; };
struct TriangPair { int status, kind; float x3D[3]; double x3Dh[4]; };

XFH_HD float triang_dot3(float a0, float a1, float a2, float b0, float b1, float b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// cos(2 atan2(h, z)) = (z^2 - h^2) / (z^2 + h^2), in double from the floats, rounded once
XFH_HD float triang_cos_stereo(float mb, float depth) {
    const double h = (double)(mb / 2.0f), z = (double)depth;
    return (float)((z * z - h * h) / (z * z + h * h));
}

// one rotation (geo_jacobi_rotation) of the one-sided Jacobi iteration on columns P < Q of U (V accumulates); returns 1 when it rotated
template <int P, int Q>
XFH_HD int triang_jacobi_pair(double (&U)[4][4], double (&V)[4][4]) {
    const double alpha = ((U[0][P] * U[0][P] + U[1][P] * U[1][P]) + U[2][P] * U[2][P]) + U[3][P] * U[3][P];
    const double beta = ((U[0][Q] * U[0][Q] + U[1][Q] * U[1][Q]) + U[2][Q] * U[2][Q]) + U[3][Q] * U[3][Q];
    const double gamma = ((U[0][P] * U[0][Q] + U[1][P] * U[1][Q]) + U[2][P] * U[2][Q]) + U[3][P] * U[3][Q];
    double c, s;
    if (!geo_jacobi_rotation(alpha, beta, gamma, &c, &s)) return 0;         // (a NaN does not rotate)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double up = U[r][P], uq = U[r][Q], vp = V[r][P], vq = V[r][Q];
        U[r][P] = c * up - s * uq; U[r][Q] = s * up + c * uq;
        V[r][P] = c * vp - s * vq; V[r][Q] = s * vp + c * vq;
    }
    return 1;
}

// the right singular vector of the smallest singular value of the float 4x4 A, in fp64: cyclic sweeps (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) until a
// sweep rotates nothing, at most GEO_JACOBI_MAX_SWEEPS; the column of V whose column of U has the least norm, the first such on a tie
XFH_HD void triang_null_vector(const float (&A)[4][4], double* x) {
    double U[4][4], V[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) { U[r][c] = (double)A[r][c]; V[r][c] = r == c ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < GEO_JACOBI_MAX_SWEEPS; ++sweep) {
        int rot = triang_jacobi_pair<0, 1>(U, V);
        rot += triang_jacobi_pair<0, 2>(U, V);
        rot += triang_jacobi_pair<0, 3>(U, V);
        rot += triang_jacobi_pair<1, 2>(U, V);
        rot += triang_jacobi_pair<1, 3>(U, V);
        rot += triang_jacobi_pair<2, 3>(U, V);
        if (rot == 0) break;
    }
    double best = ((U[0][0] * U[0][0] + U[1][0] * U[1][0]) + U[2][0] * U[2][0]) + U[3][0] * U[3][0];
    x[0] = V[0][0]; x[1] = V[1][0]; x[2] = V[2][0]; x[3] = V[3][0];
#pragma unroll
    for (int c = 1; c < 4; ++c) {
        const double n = ((U[0][c] * U[0][c] + U[1][c] * U[1][c]) + U[2][c] * U[2][c]) + U[3][c] * U[3][c];
        if (n < best) { best = n; x[0] = V[0][c]; x[1] = V[1][c]; x[2] = V[2][c]; x[3] = V[3][c]; }
    }
}

// KeyFrame::UnprojectStereo: false when the depth is not > 0
XFH_HD bool triang_unproject_stereo(const TriangParams& p, const TriangObs& o, float* X) {
    const float z = o.depth;
    if (!(z > 0.0f)) return false;
    const float x = (o.xr - p.cx) * z * p.invfx, y = (o.yr - p.cy) * z * p.invfy;
    const float* R = o.T;
#pragma unroll
    for (int k = 0; k < 3; ++k) X[k] = ((R[k] * x + R[4 + k] * y) + R[8 + k] * z) + o.Ow[k];
    return true;
}

// one keyframe's gates on x3D (:613-672): 0 pass, 1 behind, 2 reprojection
XFH_HD int triang_view_gate(const TriangParams& p, const TriangObs& o, bool stereo, const float* X) {
    const float* T = o.T;
    const float z = triang_dot3(T[8], T[9], T[10], X[0], X[1], X[2]) + T[11];
    if (z <= 0.0f) return 1;
    const float x = triang_dot3(T[0], T[1], T[2], X[0], X[1], X[2]) + T[3];
    const float y = triang_dot3(T[4], T[5], T[6], X[0], X[1], X[2]) + T[7];
    if (!stereo) {
        const float ex = (p.fx * x / z + p.cx) - o.x, ey = (p.fy * y / z + p.cy) - o.y;
        if ((double)(ex * ex + ey * ey) > 5.991 * (double)p.sigma2) return 2;
    } else {
        const float invz = (float)(1.0 / (double)z);
        const float u = p.fx * x * invz + p.cx, ur = u - p.bf * invz, v = p.fy * y * invz + p.cy;
        const float ex = u - o.x, ey = v - o.y, er = ur - o.ur;
        if ((double)(ex * ex + ey * ey + er * er) > 7.8 * (double)p.sigma2) return 2;
    }
    return 0;
}

// everything behind the 3-D point: cheirality, the two reprojection gates, the distances and the scale consistency -> status
XFH_HD int triang_gates(const TriangParams& p, const TriangObs& o1, const TriangObs& o2, bool st1, bool st2, const float* X) {
    const int g1 = triang_view_gate(p, o1, st1, X);                        // (the reference tests z1, z2, view 1, view 2: the first failure is the same)
    if (g1 == 1) return TRIANG_BEHIND1;
    const float* T2 = o2.T;
    if (triang_dot3(T2[8], T2[9], T2[10], X[0], X[1], X[2]) + T2[11] <= 0.0f) return TRIANG_BEHIND2;
    if (g1 == 2) return TRIANG_REPROJ1;
    if (triang_view_gate(p, o2, st2, X) == 2) return TRIANG_REPROJ2;
    const float a0 = X[0] - o1.Ow[0], a1 = X[1] - o1.Ow[1], a2 = X[2] - o1.Ow[2];
    const float b0 = X[0] - o2.Ow[0], b1 = X[1] - o2.Ow[1], b2 = X[2] - o2.Ow[2];
    const float dist1 = sqrtf(triang_dot3(a0, a1, a2, a0, a1, a2)), dist2 = sqrtf(triang_dot3(b0, b1, b2, b0, b1, b2));
    if (dist1 == 0.0f || dist2 == 0.0f) return TRIANG_ZERO_DIST;
    if (p.far_th > 0.0f && (dist1 >= p.far_th || dist2 >= p.far_th)) return TRIANG_FAR;
    const float ratioDist = dist2 / dist1;
    if (ratioDist * p.ratio_factor < 1.0f || ratioDist > 1.0f * p.ratio_factor) return TRIANG_SCALE;
    return TRIANG_ACCEPTED;
}

XFH_HD bool triang_is_stereo(float ur) { return ur >= 0.0f; }            // (a NaN is not stereo)

// the whole rule for one matched pair
XFH_HD void triang_pair(const TriangParams& p, const TriangObs& o1, const TriangObs& o2, TriangPair* out) {
    out->kind = 0; out->x3D[0] = out->x3D[1] = out->x3D[2] = 0.0f;
    out->x3Dh[0] = out->x3Dh[1] = out->x3Dh[2] = out->x3Dh[3] = 0.0;
    const bool st1 = triang_is_stereo(o1.ur), st2 = triang_is_stereo(o2.ur);
    const float xn1[2] = {(o1.x - p.cx) / p.fx, (o1.y - p.cy) / p.fy}, xn2[2] = {(o2.x - p.cx) / p.fx, (o2.y - p.cy) / p.fy};
    const float *T1 = o1.T, *T2 = o2.T;
    float r1[3], r2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {                                          // ray = Rwc * xn, Rwc = Rcw^T
        r1[k] = (T1[k] * xn1[0] + T1[4 + k] * xn1[1]) + T1[8 + k] * 1.0f;
        r2[k] = (T2[k] * xn2[0] + T2[4 + k] * xn2[1]) + T2[8 + k] * 1.0f;
    }
    const float n1 = sqrtf(triang_dot3(r1[0], r1[1], r1[2], r1[0], r1[1], r1[2])), n2 = sqrtf(triang_dot3(r2[0], r2[1], r2[2], r2[0], r2[1], r2[2]));
    const float cosRays = triang_dot3(r1[0], r1[1], r1[2], r2[0], r2[1], r2[2]) / (n1 * n2);
    float cos1 = cosRays + 1.0f, cos2 = cosRays + 1.0f;
    if (st1) cos1 = triang_cos_stereo(p.mb, o1.depth);
    else if (st2) cos2 = triang_cos_stereo(p.mb, o2.depth);
    const float cosStereo = cos2 < cos1 ? cos2 : cos1;                     // std::min(cos1, cos2)
    float X[3];
    if (cosRays < cosStereo && cosRays > 0.0f && (st1 || st2 || (double)cosRays < (p.inertial ? 0.9996 : 0.9998))) {
        float A[4][4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            A[0][c] = xn1[0] * T1[8 + c] - T1[c];
            A[1][c] = xn1[1] * T1[8 + c] - T1[4 + c];
            A[2][c] = xn2[0] * T2[8 + c] - T2[c];
            A[3][c] = xn2[1] * T2[8 + c] - T2[4 + c];
        }
        triang_null_vector(A, out->x3Dh);
        const float h[4] = {(float)out->x3Dh[0], (float)out->x3Dh[1], (float)out->x3Dh[2], (float)out->x3Dh[3]};
        if (h[3] == 0.0f) { out->status = TRIANG_DEGENERATE; return; }
        X[0] = h[0] / h[3]; X[1] = h[1] / h[3]; X[2] = h[2] / h[3];
    } else if (st1 && cos1 < cos2) {
        out->kind = 1;
        if (!triang_unproject_stereo(p, o1, X)) { out->status = TRIANG_STEREO_NO_DEPTH; return; }
    } else if (st2 && cos2 < cos1) {
        out->kind = 2;
        if (!triang_unproject_stereo(p, o2, X)) { out->status = TRIANG_STEREO_NO_DEPTH; return; }
    } else {
        out->status = TRIANG_LOW_PARALLAX;
        return;
    }
    out->x3D[0] = X[0]; out->x3D[1] = X[1]; out->x3D[2] = X[2];
    out->status = triang_gates(p, o1, o2, st1, st2, X);
}

// MapPoint::UpdateNormalAndDepth of the fresh point: normal[3] and (0.8f * mfMin, 1.2f * mfMax, mfMax)
XFH_HD void triang_normal_depth(const float* X, const float* Ow1, const float* Ow2, float scale_last, float* normal, float* dist) {
    const float a0 = X[0] - Ow1[0], a1 = X[1] - Ow1[1], a2 = X[2] - Ow1[2];
    const float b0 = X[0] - Ow2[0], b1 = X[1] - Ow2[1], b2 = X[2] - Ow2[2];
    const float na = sqrtf(triang_dot3(a0, a1, a2, a0, a1, a2)), nb = sqrtf(triang_dot3(b0, b1, b2, b0, b1, b2));
    normal[0] = ((0.0f + a0 / na) + b0 / nb) / 2.0f;
    normal[1] = ((0.0f + a1 / na) + b1 / nb) / 2.0f;
    normal[2] = ((0.0f + a2 / na) + b2 / nb) / 2.0f;
    const float mx = na * 1.0f, mn = mx / scale_last;
    dist[0] = 0.8f * mn; dist[1] = 1.2f * mx; dist[2] = mx;
}

// ---- the argument block of the kernels (triangulate.hip.h), filled by capi_triangulate.cpp ----
// per_b: 1 = problem b reads its own block (b * n keypoints in, b * 12 / b * 3 floats in for the pose and the centre), 0 = the shared side 1
struct TriangSide { int n, per_b; const float *xy, *raw, *ur, *depth, *T, *Ow; };
struct TriangArgs {
    int B, claim;
    TriangParams p;
    TriangSide s1, s2;
    const int* match12;
    unsigned char *status, *kind;
    float* xyz;
    int *header, *winner, *new_idx1, *new_b, *new_idx2;
    float *new_xyz, *new_normal, *new_dist;
    int* n_new;
};
enum { TRIANG_H_MATCHED = 0, TRIANG_H_TRI_ATTEMPTS = 1, TRIANG_H_STEREO_ATTEMPTS = 2, TRIANG_H_ACCEPTED = 3, TRIANG_H_NEW = 4, TRIANG_H_NEW_STEREO = 5,
       TRIANG_H_SUPERSEDED = 6 };

// keypoint i of problem b on one side
XFH_HD TriangObs triang_obs(const TriangSide& s, int b, int i) {
    const size_t pb = s.per_b ? (size_t)b : 0, k = pb * (size_t)s.n + (size_t)i;
    TriangObs o;
    o.x = s.xy[2 * k]; o.y = s.xy[2 * k + 1];
    o.xr = s.raw ? s.raw[2 * k] : o.x; o.yr = s.raw ? s.raw[2 * k + 1] : o.y;
    o.ur = s.ur ? s.ur[k] : -1.0f;
    o.depth = s.ur ? s.depth[k] : -1.0f;
    o.T = s.T + pb * 12; o.Ow = s.Ow + pb * 3;
    return o;
}
