// fuse_math.h -- the per-point arithmetic of ORBmatcher::Fuse before the window search (src/ORBmatcher.cc:1383-1429, the Sim3 form
// :1554-1589, with Pinhole::project, src/CameraModels/Pinhole.cpp:43-49, KeyFrame::IsInImage, src/KeyFrame.cc:750-753, and
// MapPoint::PredictScale, src/MapPoint.cc:514-529), written ONCE for the host entry point (xfh_fuse_project; capi_fuse.cpp) and the
// kernel (fuse_search.hip.h), and the kernel's argument block.
//
//   p3Dc = Tcw * p3Dw     row-major 3x4 [R|t] in the order of projection_math.h (bit equality with Sophus' product is not claimed)
//   zc < 0.0f             behind the camera (:1387); zc == +-0 and NaN go on
//   invz = 1.0f / zc      a FLOAT division (:1393) -- not the double one of SearchByProjection (:1893)
//   u = fx*xc/zc + cx     multiply, divide, add (Pinhole.cpp:45-46); v likewise
//   IsInImage             u >= mnMinX && u < mnMaxX && v >= mnMinY && v < mnMaxY: half-open, and a NaN is OUT (the Frame-Frame cull lets it pass)
//   ur = u - bf*invz      (:1404)
//   PO = p3Dw - Ow; dist3D = sqrtf((PO.x*PO.x + PO.y*PO.y) + PO.z*PO.z); outside [min_distance, max_distance] -> out of range (:1412)
//   PO . Pn < 0.5*dist3D  in double, as `0.5 * dist3D` promotes (:1420)
//   ratio = predict_distance / dist3D; level = #{ l : ratio > ratio_max[l] } (xfh_scale_level_thresholds stands for the ceil / log of
//                         MapPoint.cc:522-526); r = th * scale_factors[level] (:1429)
//
// The library is built with -ffp-contract=off: every line below is the IEEE operation sequence it spells, on both sides.
#pragma once
#include <math.h>
#include "projection_math.h"

// mvScaleFactors and the level thresholds, by value (kernel argument)
struct FuseLevels { int nlevels; float scale_factors[XFH_FUSE_MAX_LEVELS]; float ratio_max[XFH_FUSE_MAX_LEVELS]; };

// MapPoint::PredictScale without a logarithm: NaN -> 0, +Inf -> nlevels - 1, ratio <= 0 -> 0
XFH_HD int xfh_fuse_level(const FuseLevels& L, float ratio) {
    int level = 0;
    for (int l = 0; l < L.nlevels - 1; ++l) level += ratio > L.ratio_max[l] ? 1 : 0;
    return level;
}

// -> XFH_FUSE_BEHIND (u = v = ur = 0), XFH_FUSE_OUT_OF_IMAGE, XFH_FUSE_OUT_OF_RANGE, XFH_FUSE_BAD_ANGLE (u, v, ur as computed; all four with
// level = -1, r = 0) or XFH_FUSE_VISIBLE (level and r set).  dist = (min_distance, max_distance, predict_distance) of the map point.
XFH_HD int xfh_fuse_point(const float* T, const float* Ow, const xfh_camera& cam, const xfh_grid_bounds& b, float th, const FuseLevels& L,
                          const float* X, const float* Pn, const float* dist, float* u, float* v, float* ur, float* r, int* level) {
    const float xc = ((T[0] * X[0] + T[1] * X[1]) + T[2] * X[2]) + T[3];
    const float yc = ((T[4] * X[0] + T[5] * X[1]) + T[6] * X[2]) + T[7];
    const float zc = ((T[8] * X[0] + T[9] * X[1]) + T[10] * X[2]) + T[11];
    *u = 0.0f; *v = 0.0f; *ur = 0.0f; *r = 0.0f; *level = -1;
    if (zc < 0.0f) return XFH_FUSE_BEHIND;
    const float invz = 1.0f / zc;
    const float pu = cam.fx * xc / zc + cam.cx, pv = cam.fy * yc / zc + cam.cy;
    *u = pu; *v = pv; *ur = pu - cam.bf * invz;
    if (!(pu >= b.min_x && pu < b.max_x && pv >= b.min_y && pv < b.max_y)) return XFH_FUSE_OUT_OF_IMAGE;
    const float px = X[0] - Ow[0], py = X[1] - Ow[1], pz = X[2] - Ow[2];
    const float dist3D = sqrtf((px * px + py * py) + pz * pz);
    if (dist3D < dist[0] || dist3D > dist[1]) return XFH_FUSE_OUT_OF_RANGE;
    const float dot = (px * Pn[0] + py * Pn[1]) + pz * Pn[2];
    if ((double)dot < 0.5 * (double)dist3D) return XFH_FUSE_BAD_ANGLE;
    const float ratio = dist[2] / dist3D;
    const int lv = xfh_fuse_level(L, ratio);
    *level = lv; *r = th * L.scale_factors[lv];
    return XFH_FUSE_VISIBLE;
}

// the chi-square gate of one candidate (:1457-1481, kpLevel = 0, mvInvLevelSigma2[0] = 1.0f): true = the candidate is skipped
XFH_HD bool xfh_fuse_chi2_skips(float u, float v, float ur, float xk, float yk, float urk) {
    const float ex = u - xk, ey = v - yk;
    if (urk >= 0.0f) {
        const float er = ur - urk;
        const float e2 = (ex * ex + ey * ey) + er * er;
        return (double)e2 > 7.8;
    }
    const float e2 = ex * ex + ey * ey;
    return (double)e2 > 5.99;
}

// arguments of k_fuse_search (device pointers; the query arrays of problem b start at query b * query_stride, query_stride = nq or 0)
struct FuseArgs {
    int nq, nt, flags, init_dist, th_low;
    float th;
    size_t query_stride;
    const float* pts;                // [.][nq][3]
    const float* normals;            // [.][nq][3]
    const float* dist;               // [.][nq][3]: min_distance, max_distance, predict_distance
    const float* qdesc;              // [.][nq][64]
    const uint8_t* qflags;           // [.][nq]
    const float* Tcw;                // [B][12]
    const float* Ow;                 // [B][3]
    xfh_camera cam; xfh_grid_bounds bounds;
    FuseLevels lv;
    const char* grids; size_t grid_stride;
    const char* targets; size_t target_stride;
    const float* uright;             // [B][nt] or NULL (every keypoint monocular)
    uint8_t* status; int* best_idx; int* best_dist; int* n_window; int* n_tested; int* level;     // [B][nq]
    float* proj_out;                 // [B][nq][3] or NULL
    int* n_fused;                    // [B], zeroed on the stream before the launch
};
