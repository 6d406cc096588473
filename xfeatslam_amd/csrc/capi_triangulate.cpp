// capi_triangulate.cpp -- the entry points of include/xfeat_hip.h behind the triangulation half of LocalMapping::CreateNewMapPoints
// (xfh_triangulate*): the per-pair rule on the host (triangulate_math.h, the kernels' own lines), the device form and the host-pointer form
// (host_stage.h).
#include "host_stage.h"
#include "triangulate_math.h"
#include <math.h>

static bool triang_scalars_ok(int flags, const xfh_camera* cam, float sigma2, float ratio_factor, float scale_last, float far_th) {
    return cam && !(flags & ~(XFH_TRIANG_INERTIAL | XFH_TRIANG_CLAIM)) && isfinite(sigma2) && isfinite(ratio_factor) && isfinite(scale_last) && isfinite(far_th);
}
static TriangParams triang_params(int flags, const xfh_camera* cam, float sigma2, float ratio_factor, float scale_last, float far_th) {
    TriangParams p;
    p.fx = cam->fx; p.fy = cam->fy; p.cx = cam->cx; p.cy = cam->cy; p.invfx = 1.0f / cam->fx; p.invfy = 1.0f / cam->fy; p.bf = cam->bf; p.mb = cam->bf / cam->fx;
    p.sigma2 = sigma2; p.ratio_factor = ratio_factor; p.scale_last = scale_last; p.far_th = far_th;
    p.inertial = (flags & XFH_TRIANG_INERTIAL) ? 1 : 0;
    return p;
}

extern "C" {

int xfh_triangulate_pair(const xfh_camera* cam, int flags, float sigma2, float ratio_factor, float scale_last, float far_th, const float* xy1,
                         const float* xy_raw1, float uright1, float depth1, const float* Tcw1, const float* Ow1, const float* xy2, const float* xy_raw2,
                         float uright2, float depth2, const float* Tcw2, const float* Ow2, int* status, int* kind, float* x3D, float* normal, float* dist,
                         double* x3Dh) {
    if (!triang_scalars_ok(flags & ~XFH_TRIANG_CLAIM, cam, sigma2, ratio_factor, scale_last, far_th) || (flags & XFH_TRIANG_CLAIM)) return XFH_ERR_INVALID_ARG;
    if (!xy1 || !Tcw1 || !Ow1 || !xy2 || !Tcw2 || !Ow2 || !status || !kind || !x3D || !normal || !dist) return XFH_ERR_INVALID_ARG;
    const TriangParams p = triang_params(flags, cam, sigma2, ratio_factor, scale_last, far_th);
    const TriangObs o1 = {xy1[0], xy1[1], xy_raw1 ? xy_raw1[0] : xy1[0], xy_raw1 ? xy_raw1[1] : xy1[1], uright1, depth1, Tcw1, Ow1};
    const TriangObs o2 = {xy2[0], xy2[1], xy_raw2 ? xy_raw2[0] : xy2[0], xy_raw2 ? xy_raw2[1] : xy2[1], uright2, depth2, Tcw2, Ow2};
    TriangPair r;
    triang_pair(p, o1, o2, &r);
    *status = r.status; *kind = r.kind;
    for (int k = 0; k < 3; ++k) { x3D[k] = r.x3D[k]; normal[k] = 0.0f; dist[k] = 0.0f; }
    if (r.status == TRIANG_ACCEPTED) triang_normal_depth(r.x3D, Ow1, Ow2, scale_last, normal, dist);
    if (x3Dh) for (int k = 0; k < 4; ++k) x3Dh[k] = r.x3Dh[k];
    return XFH_OK;
}

int xfh_triangulate_device(xfh_ctx* c, int B, int n1, int n2, int side1_shared, int flags, const xfh_camera* cam, float sigma2, float ratio_factor,
                           float scale_last, float far_th, const float* d_xy1, const float* d_xy_raw1, const float* d_uright1, const float* d_depth1,
                           const float* d_Tcw1, const float* d_Ow1, const float* d_xy2, const float* d_xy_raw2, const float* d_uright2, const float* d_depth2,
                           const float* d_Tcw2, const float* d_Ow2, const int* d_match12, uint8_t* d_status, uint8_t* d_kind, float* d_xyz, int* d_header,
                           int* d_winner, int* d_new_idx1, int* d_new_b, int* d_new_idx2, float* d_new_xyz, float* d_new_normal, float* d_new_dist,
                           int* d_n_new) {
    if (!c || B < 1 || B > 65535 || n1 < 1 || n1 > XFH_GRID_MAX_N || n2 < 1 || n2 > XFH_GRID_MAX_N || (side1_shared != 0 && side1_shared != 1))
        return XFH_ERR_INVALID_ARG;
    if (!triang_scalars_ok(flags, cam, sigma2, ratio_factor, scale_last, far_th)) return XFH_ERR_INVALID_ARG;
    const bool claim = (flags & XFH_TRIANG_CLAIM) != 0;
    if (claim && !side1_shared) return XFH_ERR_INVALID_ARG;
    if (!d_xy1 || !d_Tcw1 || !d_Ow1 || !d_xy2 || !d_Tcw2 || !d_Ow2 || !d_match12 || !d_status || !d_kind || !d_xyz || !d_header) return XFH_ERR_INVALID_ARG;
    if ((d_uright1 && !d_depth1) || (d_uright2 && !d_depth2)) return XFH_ERR_INVALID_ARG;          // a stereo keypoint needs its mvDepth
    if (claim && (!d_winner || !d_new_idx1 || !d_new_b || !d_new_idx2 || !d_new_xyz || !d_new_normal || !d_new_dist || !d_n_new)) return XFH_ERR_INVALID_ARG;
    if (misaligned(3, d_xy1, d_xy_raw1, d_uright1, d_depth1, d_Tcw1, d_Ow1, d_xy2, d_xy_raw2, d_uright2, d_depth2, d_Tcw2, d_Ow2, d_match12, d_xyz, d_header,
                   d_winner, d_new_idx1, d_new_b, d_new_idx2, d_new_xyz, d_new_normal, d_new_dist, d_n_new)) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    TriangArgs a = {};
    a.B = B; a.claim = claim ? 1 : 0;
    a.p = triang_params(flags, cam, sigma2, ratio_factor, scale_last, far_th);
    a.s1 = TriangSide{n1, side1_shared ? 0 : 1, d_xy1, d_xy_raw1, d_uright1, d_depth1, d_Tcw1, d_Ow1};
    a.s2 = TriangSide{n2, 1, d_xy2, d_xy_raw2, d_uright2, d_depth2, d_Tcw2, d_Ow2};
    a.match12 = d_match12; a.status = d_status; a.kind = d_kind; a.xyz = d_xyz; a.header = d_header;
    if (claim) {
        a.winner = d_winner; a.new_idx1 = d_new_idx1; a.new_b = d_new_b; a.new_idx2 = d_new_idx2; a.new_xyz = d_new_xyz; a.new_normal = d_new_normal;
        a.new_dist = d_new_dist; a.n_new = d_n_new;
    }
    HIPCK(c, launch_triangulate(c, a));
    return XFH_OK;
}

int xfh_triangulate(xfh_ctx* c, int B, int n1, int n2, int flags, const xfh_camera* cam, float sigma2, float ratio_factor, float scale_last, float far_th,
                    const float* xy1, const float* xy_raw1, const float* uright1, const float* depth1, const float* Tcw1, const float* Ow1, const float* xy2,
                    const float* xy_raw2, const float* uright2, const float* depth2, const float* Tcw2, const float* Ow2, const int* match12, uint8_t* status,
                    uint8_t* kind, float* xyz, int* header, int* winner, int* new_idx1, int* new_b, int* new_idx2, float* new_xyz, float* new_normal,
                    float* new_dist, int* n_new) {
    if (!c || B < 1 || B > 65535 || n1 < 1 || n1 > XFH_GRID_MAX_N || n2 < 1 || n2 > XFH_GRID_MAX_N) return XFH_ERR_INVALID_ARG;
    if (!triang_scalars_ok(flags, cam, sigma2, ratio_factor, scale_last, far_th)) return XFH_ERR_INVALID_ARG;
    const bool claim = (flags & XFH_TRIANG_CLAIM) != 0;
    if (!xy1 || !Tcw1 || !Ow1 || !xy2 || !Tcw2 || !Ow2 || !match12 || !status || !kind || !xyz || !header) return XFH_ERR_INVALID_ARG;
    if ((uright1 && !depth1) || (uright2 && !depth2)) return XFH_ERR_INVALID_ARG;
    if (claim && (!winner || !new_idx1 || !new_b || !new_idx2 || !new_xyz || !new_normal || !new_dist || !n_new)) return XFH_ERR_INVALID_ARG;
    const size_t N1 = (size_t)n1, N2 = (size_t)B * n2, P = (size_t)B * n1;
    HostStage s{c};
    auto x1 = s.in<float>(xy1, N1 * 8); auto r1 = s.in_opt<float>(xy_raw1, N1 * 8); auto u1 = s.in_opt<float>(uright1, N1 * 4);
    auto z1 = s.in_opt<float>(uright1 ? depth1 : nullptr, N1 * 4); auto T1 = s.in<float>(Tcw1, 48); auto O1 = s.in<float>(Ow1, 12);
    auto x2 = s.in<float>(xy2, N2 * 8); auto r2 = s.in_opt<float>(xy_raw2, N2 * 8); auto u2 = s.in_opt<float>(uright2, N2 * 4);
    auto z2 = s.in_opt<float>(uright2 ? depth2 : nullptr, N2 * 4); auto T2 = s.in<float>(Tcw2, (size_t)B * 48); auto O2 = s.in<float>(Ow2, (size_t)B * 12);
    auto m = s.in<int>(match12, P * 4);
    auto ost = s.out<uint8_t>(status, P); auto okd = s.out<uint8_t>(kind, P); auto oxyz = s.out<float>(xyz, P * 12); auto oh = s.out<int>(header, (size_t)B * 32);
    auto ow = s.out_opt<int>(claim ? winner : nullptr, N1 * 4); auto o1 = s.out_opt<int>(claim ? new_idx1 : nullptr, N1 * 4);
    auto ob = s.out_opt<int>(claim ? new_b : nullptr, N1 * 4); auto o2 = s.out_opt<int>(claim ? new_idx2 : nullptr, N1 * 4);
    auto ox = s.out_opt<float>(claim ? new_xyz : nullptr, N1 * 12); auto on = s.out_opt<float>(claim ? new_normal : nullptr, N1 * 12);
    auto od = s.out_opt<float>(claim ? new_dist : nullptr, N1 * 12); auto onn = s.out_opt<int>(claim ? n_new : nullptr, 4);
    if (const int rc = s.upload(); rc != XFH_OK) return rc;
    const int rc = xfh_triangulate_device(c, B, n1, n2, 1, flags, cam, sigma2, ratio_factor, scale_last, far_th, x1, r1, u1, z1, T1, O1, x2, r2, u2, z2, T2, O2, m,
                                          ost, okd, oxyz, oh, ow, o1, ob, o2, ox, on, od, onn);
    if (rc != XFH_OK) return rc;                                              // (a HIP error: every argument check has passed above)
    return s.download();
}

}  // extern "C"
