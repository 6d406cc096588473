// sim3_math.h -- the per-point arithmetic of ORBmatcher::SearchBySim3 before the window search (src/ORBmatcher.cc:1691-1722 and its
// mirror image :1771-1802, with KeyFrame::IsInImage, src/KeyFrame.cc:750-753, and MapPoint::PredictScale, src/MapPoint.cc:514-529),
// written ONCE for the host entry point (xfh_sim3_project; capi_loop.cpp) and the kernel (sim3_search.hip.h), and the kernel's
// argument block.
//
//   p1 = Tqw * X          the query side's pose, row-major 3x4 [R|t] in the order of fuse_math.h
//   p2 = M * p1           M = [s*R | t] of S21 (direction 1->2) or S12 (2->1), the same row order (bit equality with Sophus' product is not claimed)
//   p2.z < 0.0f           behind the camera (:1696; the reference compares with the double 0.0, which is the same test); +-0 and NaN go on
//   invz = (float)(1.0 / (double)p2.z)      a DOUBLE division rounded once (:1699) -- not the float one of Fuse (:1393)
//   x = p2.x*invz; y = p2.y*invz; u = fx*x + cx; v = fy*y + cy      (:1700-1704; no Pinhole::project here)
//   IsInImage             half-open, a NaN is out
//   dist3D = sqrtf((p2.x*p2.x + p2.y*p2.y) + p2.z*p2.z)      the norm of the CAMERA-frame point (:1712), not |X - Ow|; outside [min, max] -> out of range
//   level, r              as Fuse: #{ l : predict_distance / dist3D > ratio_max[l] }, th * scale_factors[level]
// There is no viewing-angle test in SearchBySim3.
//
// The library is built with -ffp-contract=off: every line below is the IEEE operation sequence it spells, on both sides.
#pragma once
#include <math.h>
#include "fuse_math.h"

// -> XFH_SIM3_BEHIND (u = v = 0), XFH_SIM3_OUT_OF_IMAGE, XFH_SIM3_OUT_OF_RANGE (u, v as computed; all three with level = -1, r = 0) or
// XFH_SIM3_VISIBLE (level and r set).  dist = (min_distance, max_distance, predict_distance) of the map point.
XFH_HD int xfh_sim3_point(const float* T, const float* M, const xfh_camera& cam, const xfh_grid_bounds& b, float th, const FuseLevels& L,
                          const float* X, const float* dist, float* u, float* v, float* r, int* level) {
    const float x1 = ((T[0] * X[0] + T[1] * X[1]) + T[2] * X[2]) + T[3];
    const float y1 = ((T[4] * X[0] + T[5] * X[1]) + T[6] * X[2]) + T[7];
    const float z1 = ((T[8] * X[0] + T[9] * X[1]) + T[10] * X[2]) + T[11];
    const float x2 = ((M[0] * x1 + M[1] * y1) + M[2] * z1) + M[3];
    const float y2 = ((M[4] * x1 + M[5] * y1) + M[6] * z1) + M[7];
    const float z2 = ((M[8] * x1 + M[9] * y1) + M[10] * z1) + M[11];
    *u = 0.0f; *v = 0.0f; *r = 0.0f; *level = -1;
    if (z2 < 0.0f) return XFH_SIM3_BEHIND;
    const float invz = (float)(1.0 / (double)z2);
    const float x = x2 * invz, y = y2 * invz;
    const float pu = cam.fx * x + cam.cx, pv = cam.fy * y + cam.cy;
    *u = pu; *v = pv;
    if (!(pu >= b.min_x && pu < b.max_x && pv >= b.min_y && pv < b.max_y)) return XFH_SIM3_OUT_OF_IMAGE;
    const float dist3D = sqrtf((x2 * x2 + y2 * y2) + z2 * z2);
    if (dist3D < dist[0] || dist3D > dist[1]) return XFH_SIM3_OUT_OF_RANGE;
    const float ratio = dist[2] / dist3D;
    const int lv = xfh_fuse_level(L, ratio);
    *level = lv; *r = th * L.scale_factors[lv];
    return XFH_SIM3_VISIBLE;
}

// one side of a keyframe pair as k_sim3_search reads and writes it (device pointers).  stride = 1: problem b has its own block of every
// input, b * n elements in; stride = 0: every problem reads problem 0's (side1_shared).  The outputs are always [B][n].
struct Sim3Side {
    int n, stride;
    const char* grids; size_t grid_stride;     // blob of the side's keypoints
    const char* desc; size_t desc_stride;      // keyframe descriptor rows [n][64], problem b's desc_stride bytes * b in
    const float* X;                            // [.][n][3] world position of the map point keypoint i holds
    const float* dist;                         // [.][n][3]: min_distance, max_distance, predict_distance
    const float* mpdesc;                       // [.][n][64] the map point's own descriptor
    const uint8_t* flags;                      // [.][n]
    const float* Tw;                           // [.][12]
    uint8_t* status; int* match; int* best_dist; int* n_window; int* n_tested; int* level;     // [B][n]
    float* proj_out;                           // [B][n][3] or NULL
};
// arguments of k_sim3_search and k_sim3_agree: s[0] = side 1, s[1] = side 2
struct Sim3Args {
    Sim3Side s[2];
    const float* M21; const float* M12;        // [B][12]
    xfh_camera cam; xfh_grid_bounds bounds;
    FuseLevels lv;
    float th; int th_high;
    int nb1;                                   // workgroups of direction 1->2 per problem: (n1 + 3) / 4; the ones behind them run 2->1
    int* match12;                              // [B][n1]
    int* n_found;                              // [B], zeroed on the stream before the launches
};
