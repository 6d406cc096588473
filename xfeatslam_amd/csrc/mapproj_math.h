// mapproj_math.h -- the per-point arithmetic of the three map-point SearchByProjection forms before the window search, written ONCE for
// the host entry point (xfh_map_project; capi_loop.cpp) and the kernel (mapproj_search.hip.h), and the front kernel's argument block:
//   SearchByProjection(KeyFrame*, Sim3f& Scw, vpPoints, vpMatched, th, ratioHamming)                  src/ORBmatcher.cc:640-674   XFH_MAPPROJ_FORM_SIM3
//   SearchByProjection(KeyFrame*, Sim3f& Scw, vpPoints, vpPointsKFs, vpMatched, vpMatchedKF, ...)     :748-787                    XFH_MAPPROJ_FORM_SIM3_KF
//   SearchByProjection(Frame& CurrentFrame, KeyFrame*, sAlreadyFound, th, ORBdist)                    :2098-2122                  XFH_MAPPROJ_FORM_RELOC
// The forms differ in four places, one flag bit each:
//   CULL_BEHIND    zc < 0.0f -> behind (:646, :754); the relocalisation form has no such test
//   PROJECT_INVZ   invz = 1.0f / zc; x = xc*invz; y = yc*invz; u = fx*x + cx (:758-763, a FLOAT division: `1/p3Dc(2)`); otherwise
//                  Pinhole::project, u = fx*xc/zc + cx (:650, :2101)
//   BOUNDS_CLOSED  u < min_x || u > max_x || v < min_y || v > max_y -> out, a NaN passes (:2103-2106); otherwise KeyFrame::IsInImage,
//                  half-open, a NaN is out (:653, :766)
//   CHECK_ANGLE    (double)(PO . Pn) < 0.5 * (double)dist3D -> past 60 degrees (:668, :781); not in the relocalisation form
// Everything else is fuse_math.h's: the row order of Tcw * X, PO = X - Ow and its norm, the range test, the level and the radius.
//
// The library is built with -ffp-contract=off: every line below is the IEEE operation sequence it spells, on both sides.
#pragma once
#include <math.h>
#include "fuse_math.h"
#include "projection_layout.h"

// -> XFH_MAPPROJ_BEHIND (u = v = 0), XFH_MAPPROJ_OUT_OF_IMAGE, XFH_MAPPROJ_OUT_OF_RANGE, XFH_MAPPROJ_BAD_ANGLE (u, v as computed; all four
// with level = -1, r = 0) or XFH_MAPPROJ_VISIBLE (level and r set).  dist = (min_distance, max_distance, predict_distance) of the map point.
XFH_HD int xfh_mapproj_point(const float* T, const float* Ow, const xfh_camera& cam, const xfh_grid_bounds& b, float th, const FuseLevels& L, int form,
                             const float* X, const float* Pn, const float* dist, float* u, float* v, float* r, int* level) {
    const float xc = ((T[0] * X[0] + T[1] * X[1]) + T[2] * X[2]) + T[3];
    const float yc = ((T[4] * X[0] + T[5] * X[1]) + T[6] * X[2]) + T[7];
    const float zc = ((T[8] * X[0] + T[9] * X[1]) + T[10] * X[2]) + T[11];
    *u = 0.0f; *v = 0.0f; *r = 0.0f; *level = -1;
    if ((form & XFH_MAPPROJ_CULL_BEHIND) && zc < 0.0f) return XFH_MAPPROJ_BEHIND;
    float pu, pv;
    if (form & XFH_MAPPROJ_PROJECT_INVZ) {
        const float invz = 1.0f / zc;
        const float x = xc * invz, y = yc * invz;
        pu = cam.fx * x + cam.cx; pv = cam.fy * y + cam.cy;
    } else {
        pu = cam.fx * xc / zc + cam.cx; pv = cam.fy * yc / zc + cam.cy;
    }
    *u = pu; *v = pv;
    if (form & XFH_MAPPROJ_BOUNDS_CLOSED) {
        if (pu < b.min_x || pu > b.max_x || pv < b.min_y || pv > b.max_y) return XFH_MAPPROJ_OUT_OF_IMAGE;
    } else if (!(pu >= b.min_x && pu < b.max_x && pv >= b.min_y && pv < b.max_y)) return XFH_MAPPROJ_OUT_OF_IMAGE;
    const float px = X[0] - Ow[0], py = X[1] - Ow[1], pz = X[2] - Ow[2];
    const float dist3D = sqrtf((px * px + py * py) + pz * pz);
    if (dist3D < dist[0] || dist3D > dist[1]) return XFH_MAPPROJ_OUT_OF_RANGE;
    if (form & XFH_MAPPROJ_CHECK_ANGLE) {
        const float dot = (px * Pn[0] + py * Pn[1]) + pz * Pn[2];
        if ((double)dot < 0.5 * (double)dist3D) return XFH_MAPPROJ_BAD_ANGLE;
    }
    const float ratio = dist[2] / dist3D;
    const int lv = xfh_fuse_level(L, ratio);
    *level = lv; *r = th * L.scale_factors[lv];
    return XFH_MAPPROJ_VISIBLE;
}

// arguments of k_mapproj_candidates (device pointers).  p is what k_proj_resolve and k_proj_count go on with: pts = the world points, skip =
// taken, n_candidates = n_tested, second_dist = scratch in the workspace, grid_stride / target_stride = 0 when the target is shared.
struct MapProjArgs {
    ProjArgs p;
    const float* normals;            // [B][nq][3]
    const float* dist;               // [B][nq][3]: min_distance, max_distance, predict_distance
    const float* Ow;                 // [B][3]
    FuseLevels lv;
    float th; int form;
    int* n_window; int* level;       // [B][nq]
};
