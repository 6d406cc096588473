// projection_math.h -- the per-point arithmetic of ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono) before the window
// search (src/ORBmatcher.cc:1888-1909, :1938 with Pinhole::project, src/CameraModels/Pinhole.cpp:43-49), written ONCE for the host
// entry point (xfh_project_points; capi_search.cpp) and the kernel (projection_search.hip.h).
//
//   x3Dc = Tcw * x3Dw     here: row-major 3x4 [R|t], xc = ((T[0]*X + T[1]*Y) + T[2]*Z) + T[3], yc / zc from rows 1 / 2.  The reference
//                         multiplies through Sophus::SE3f (Eigen's quaternion path); bit equality with its x3Dc is not claimed.
//   invzc = 1.0 / zc      a double division rounded to fp32 (:1893); invzc < 0 -> the point is behind the camera (:1895)
//   u = fx*xc/zc + cx     multiply, divide, add (Pinhole.cpp:45-46); v likewise
//   the cull              u < mnMinX || u > mnMaxX || v < mnMinY || v > mnMaxY (:1900-1903): a NaN passes, as in the reference
//   ur = u - bf*invzc     (:1938)
//
// The library is built with -ffp-contract=off: every line below is the IEEE operation sequence it spells, on both sides.
#pragma once
#include <stdint.h>
#include "../../include/xfeat_hip.h"
#include "hd.h"

// -> XFH_PROJ_BEHIND (u = v = ur = 0), XFH_PROJ_OUT_OF_BOUNDS or XFH_PROJ_VISIBLE (both with u, v, ur as computed)
XFH_HD int xfh_project_point(const float* T, const xfh_camera& cam, const xfh_grid_bounds& b, float X, float Y, float Z, float* u, float* v, float* ur) {
    const float xc = ((T[0] * X + T[1] * Y) + T[2] * Z) + T[3];
    const float yc = ((T[4] * X + T[5] * Y) + T[6] * Z) + T[7];
    const float zc = ((T[8] * X + T[9] * Y) + T[10] * Z) + T[11];
    const float invz = (float)(1.0 / (double)zc);
    *u = 0.0f; *v = 0.0f; *ur = 0.0f;
    if (invz < 0.0f) return XFH_PROJ_BEHIND;
    const float pu = cam.fx * xc / zc + cam.cx, pv = cam.fy * yc / zc + cam.cy;
    *u = pu; *v = pv; *ur = pu - cam.bf * invz;
    if (pu < b.min_x || pu > b.max_x || pv < b.min_y || pv > b.max_y) return XFH_PROJ_OUT_OF_BOUNDS;
    return XFH_PROJ_VISIBLE;
}
