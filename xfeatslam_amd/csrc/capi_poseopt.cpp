// capi_poseopt.cpp -- the entry points of include/xfeat_hip.h behind Optimizer::PoseOptimization (xfh_pose_*): the pose, solve and edge lines on the
// host (poseopt_math.h, the kernel's own lines), the device form and the host-pointer form (host_stage.h).
#include "host_stage.h"
#include "poseopt_math.h"
#include <math.h>

static bool pose_args_ok(int B, int nt, int nq, float inv_sigma2) {
    if (B < 1 || B > 65535 || nt < 1 || nt > XFH_GRID_MAX_N || nq < 1 || nq > XFH_GRID_MAX_N) return false;
    return isfinite(inv_sigma2) && inv_sigma2 > 0.0f;
}
static PosePose pose_of(const double* p) { return PosePose{{p[0], p[1], p[2], p[3]}, {p[4], p[5], p[6]}}; }
static void pose_put(const PosePose& P, double* p) { for (int k = 0; k < 4; ++k) p[k] = P.q[k]; for (int k = 0; k < 3; ++k) p[4 + k] = P.t[k]; }
static PoseCam pose_cam(const xfh_camera* cam) { return PoseCam{(double)cam->fx, (double)cam->fy, (double)cam->cx, (double)cam->cy, (double)cam->bf}; }

extern "C" {

int xfh_pose_from_tcw(const float* Tcw, double* pose7) {
    if (!Tcw || !pose7) return XFH_ERR_INVALID_ARG;
    PosePose P;
    pose_from_tcw(Tcw, &P);
    pose_put(P, pose7);
    return XFH_OK;
}

int xfh_pose_to_tcw(const double* pose7, float* Tcw) {
    if (!Tcw || !pose7) return XFH_ERR_INVALID_ARG;
    pose_to_tcw(pose_of(pose7), Tcw);
    return XFH_OK;
}

int xfh_pose_oplus(const double* pose7, const double* update6, double* pose7_out) {
    if (!pose7 || !update6 || !pose7_out) return XFH_ERR_INVALID_ARG;
    PosePose o;
    pose_oplus(update6, pose_of(pose7), &o);
    pose_put(o, pose7_out);
    return XFH_OK;
}

int xfh_pose_solve(const double* H21, double lambda, const double* b6, double* x6) {
    if (!H21 || !b6 || !x6) return 0;
    return pose_ldlt_solve(H21, lambda, b6, x6) ? 1 : 0;
}

int xfh_pose_edge(const double* pose7, const xfh_camera* cam, const float* point3, const float* xy, float uright, float inv_sigma2, int robust,
                  double* error3, double* chi2, double* jacobian18, double* rho1) {
    if (!pose7 || !cam || !point3 || !xy) return XFH_ERR_INVALID_ARG;
    const bool stereo = !(uright < 0.0f);
    const PoseCam pc = pose_cam(cam);
    const double X[3] = {(double)point3[0], (double)point3[1], (double)point3[2]}, obs[3] = {(double)xy[0], (double)xy[1], (double)uright};
    double p[3], e[3], J[18], r0, r1 = 1.0;
    const double c = pose_edge_error(pose_of(pose7), pc, X, obs, stereo, (double)inv_sigma2, p, e);
    pose_edge_jacobian(pc, p, stereo, J);
    if (robust) pose_huber(c, pose_delta(stereo), &r0, &r1);
    if (error3) for (int k = 0; k < 3; ++k) error3[k] = e[k];
    if (chi2) *chi2 = c;
    if (jacobian18) for (int k = 0; k < 18; ++k) jacobian18[k] = J[k];
    if (rho1) *rho1 = r1;
    return XFH_OK;
}

size_t xfh_pose_optimize_workspace_bytes(int nt, int B) {
    if (nt < 1 || nt > XFH_GRID_MAX_N || B < 1 || B > 65535) return 0;
    return pose_ws_bytes(nt) * (size_t)B;
}

int xfh_pose_optimize_device(xfh_ctx* c, int B, int nt, int nq, const float* d_Tcw, const xfh_camera* cam, const float* d_xy_un, const float* d_uright,
                             const int* d_assigned, const float* d_points, float inv_sigma2, void* d_ws, float* d_Tcw_out, uint8_t* d_outlier,
                             float* d_chi2, int* d_header, double* d_final_chi2) {
    if (!c || !pose_args_ok(B, nt, nq, inv_sigma2)) return XFH_ERR_INVALID_ARG;
    if (!d_Tcw || !cam || !d_xy_un || !d_assigned || !d_points || !d_ws || !d_Tcw_out || !d_outlier || !d_chi2 || !d_header || !d_final_chi2)
        return XFH_ERR_INVALID_ARG;
    if (misaligned(15, d_ws) || misaligned(7, d_final_chi2) || misaligned(3, d_Tcw, d_xy_un, d_uright, d_assigned, d_points, d_Tcw_out, d_chi2, d_header))
        return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    PoseArgs a = {};
    a.nt = nt; a.nq = nq; a.Tcw = d_Tcw; a.cam = pose_cam(cam); a.xy_un = d_xy_un; a.uright = d_uright; a.assigned = d_assigned; a.points = d_points;
    a.w = (double)inv_sigma2;
    a.ws = (char*)d_ws; a.ws_stride = pose_ws_bytes(nt);
    a.Tcw_out = d_Tcw_out; a.outlier = d_outlier; a.chi2 = d_chi2; a.header = d_header; a.final_chi2 = d_final_chi2;
    HIPCK(c, launch_pose_optimize(c, a, B));
    return XFH_OK;
}

int xfh_pose_optimize(xfh_ctx* c, int nt, int nq, const float* Tcw, const xfh_camera* cam, const float* xy_un, const float* uright, const int* assigned,
                      const float* points, float inv_sigma2, float* Tcw_out, uint8_t* outlier, float* chi2, int* header, double* final_chi2) {
    if (!c || !pose_args_ok(1, nt, nq, inv_sigma2)) return XFH_ERR_INVALID_ARG;
    if (!Tcw || !cam || !xy_un || !assigned || !points || !Tcw_out || !outlier || !chi2 || !header || !final_chi2) return XFH_ERR_INVALID_ARG;
    HostStage s{c};
    auto dT = s.in<float>(Tcw, 48), dxy = s.in<float>(xy_un, (size_t)nt * 8);
    auto dur = s.in_opt<float>(uright, (size_t)nt * 4);
    auto das = s.in<int>(assigned, (size_t)nt * 4);
    auto dp = s.in<float>(points, (size_t)nq * 12);
    auto dws = s.tmp<char>(xfh_pose_optimize_workspace_bytes(nt, 1));
    auto dTo = s.out<float>(Tcw_out, 48);
    auto dol = s.out<uint8_t>(outlier, (size_t)nt);
    auto dch = s.out<float>(chi2, (size_t)nt * 4);
    auto dh = s.out<int>(header, 32);
    auto dfc = s.out<double>(final_chi2, 8);
    if (const int rc = s.upload(); rc != XFH_OK) return rc;
    const int rc = xfh_pose_optimize_device(c, 1, nt, nq, dT, cam, dxy, dur, das, dp, inv_sigma2, dws, dTo, dol, dch, dh, dfc);
    if (rc != XFH_OK) return rc;                                              // (a HIP error: every argument check has passed above)
    return s.download();
}

}  // extern "C"
