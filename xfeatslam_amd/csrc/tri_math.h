// tri_math.h -- the per-pair arithmetic of ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:1092-1331): the stereo-only gate
// (:1192-1196), the epipole radius (:1211-1219) and Pinhole::epipolarConstrain (src/CameraModels/Pinhole.cpp:107-129) with the caller's
// F12, written ONCE for the host entry point (xfh_epipolar_gate; capi_triangulation.cpp) and the kernel (triangulation_search.hip.h),
// and the kernel's argument block.
//
//   a = (x1*F[0] + y1*F[3]) + F[6]; b = (x1*F[1] + y1*F[4]) + F[7]; c = (x1*F[2] + y1*F[5]) + F[8]     F12 row-major: F12(r, c) = F[3r + c] (Pinhole.cpp:115-117)
//   den = a*a + b*b                                                                                    (:121)
//   stereo2 = uright2 >= 0 (a NaN is monocular);  ONLY_STEREO && !stereo2 -> not a candidate
//   !stereo1 && !stereo2:  dx = ep[0] - x2; dy = ep[1] - y2;  dx*dx + dy*dy < epipole_r2 -> rejected   (a NaN sum is not rejected here)
//   !COARSE:  num = (a*x2 + b*y2) + c;  den == 0 -> rejected;  dsqr = (num*num) / den;  !((double)dsqr < 3.84 * (double)unc) -> rejected
//
// The library is built with -ffp-contract=off: every line below is the IEEE operation sequence it spells, on both sides.
#pragma once
#include "projection_math.h"

struct TriLine { float a, b, c, den; };                     // the epipolar line of one KF1 keypoint in KF2

XFH_HD TriLine xfh_tri_line(const float* F, float x1, float y1) {
    TriLine l;
    l.a = (x1 * F[0] + y1 * F[3]) + F[6];
    l.b = (x1 * F[1] + y1 * F[4]) + F[7];
    l.c = (x1 * F[2] + y1 * F[5]) + F[8];
    l.den = l.a * l.a + l.b * l.b;
    return l;
}

// one member of KF2's node that has no map point -> XFH_TRI_GATE_SKIPPED (the stereo-only gate: not a candidate), XFH_TRI_GATE_REJECTED (a
// candidate that fails the epipole or the epipolar test) or XFH_TRI_GATE_PASSED (it reaches DescriptorDistance)
XFH_HD int xfh_tri_member(const TriLine& l, float ex, float ey, float epipole_r2, float unc, int flags, bool stereo1, float x2, float y2, float ur2) {
    const bool stereo2 = ur2 >= 0.0f;
    if ((flags & XFH_TRI_ONLY_STEREO) && !stereo2) return XFH_TRI_GATE_SKIPPED;
    if (!stereo1 && !stereo2) {
        const float dx = ex - x2, dy = ey - y2;
        if (dx * dx + dy * dy < epipole_r2) return XFH_TRI_GATE_REJECTED;
    }
    if (!(flags & XFH_TRI_COARSE)) {
        const float num = (l.a * x2 + l.b * y2) + l.c;
        if (l.den == 0.0f) return XFH_TRI_GATE_REJECTED;
        const float dsqr = (num * num) / l.den;
        if (!((double)dsqr < 3.84 * (double)unc)) return XFH_TRI_GATE_REJECTED;
    }
    return XFH_TRI_GATE_PASSED;
}

// one side of k_triangulation_search (device pointers; problem b's arrays start b * n elements, b * nodes_stride resp. b * desc_stride
// bytes into each; side 1 of a shared call has all three at 0)
struct TriSide {
    int n;
    size_t elem_stride, nodes_stride, desc_stride;
    const char* nodes;
    const float* xy;                 // [.][n][2]
    const float* uright;             // [.][n] or NULL (every keypoint monocular)
    const uint8_t* has;              // [.][n]
    const char* desc;                // [n][64] floats per problem
};
struct TriArgs {
    int flags, th_low;
    float epipole_r2, unc;
    TriSide s1, s2;
    const float* F12;                // [B][9]
    const float* ep;                 // [B][2]
    uint8_t* status; int* match12; int* best_dist; int* n_candidates; int* n_geom;        // [B][n1]
    int* n_matches;                  // [B], zeroed on the stream before the launch
};
