// capi_optsim3.cpp -- the entry points of include/xfeat_hip.h behind Optimizer::OptimizeSim3 (xfh_sim3_optimize*, xfh_sim3_state_*, _oplus, _map,
// _inverse_map, _solve7, _edge): the pieces of the rule on the host (optsim3_math.h, the kernel's own lines), the whole rule on one host thread, the
// device form and the host-pointer form (host_stage.h).
#include "host_stage.h"
#include "optsim3_math.h"
#include <math.h>

static_assert(XFH_OS3_NO_EDGE == XFH_SIM3_OPT_NO_EDGE && XFH_OS3_BAD_FIRST == XFH_SIM3_OPT_BAD_FIRST && XFH_OS3_BAD_FINAL == XFH_SIM3_OPT_BAD_FINAL &&
              XFH_OS3_INLIER == XFH_SIM3_OPT_INLIER && XFH_OS3_HEADER_INTS == XFH_SIM3_OPT_HEADER_INTS && XFH_OS3_S12_FLOATS == XFH_SIM3_OPT_S12_FLOATS,
              "optsim3_math.h and include/xfeat_hip.h name the same values");

struct Os3In {                                                              // the arrays of one call, device or host pointers
    const float *T1w, *xy_un1; const int* point1; const float* points1; const int* assigned; const float* points2; const uint8_t* flags2; const int* index2;
    const float *xy_un2, *T2w, *S12; size_t S12_stride; const float* Tmw;
};
struct Os3Out {
    int* assigned_out; uint8_t* status; float* chi2; double* state; float* S12_out; size_t S12_out_stride; float *Tcw, *Ow; int* header; double* final_chi2;
};

static bool os3_scalars_ok(int B, int n1, int M1, int nq, int n2, int side1_shared, const xfh_camera* cam1, const xfh_camera* cam2, float th2, int fix_scale,
                           int all_points, float w1, float w2) {
    if (B < 1 || B > 65535 || n1 < 1 || n1 > XFH_GRID_MAX_N || M1 < 1 || M1 > XFH_GRID_MAX_N || nq < 1 || nq > XFH_GRID_MAX_N || n2 < 1 || n2 > XFH_GRID_MAX_N)
        return false;
    if (!cam1 || !cam2 || side1_shared < 0 || side1_shared > 1 || fix_scale < 0 || fix_scale > 1 || all_points < 0 || all_points > 1) return false;
    return isfinite(th2) && th2 > 0.0f && isfinite(w1) && w1 > 0.0f && isfinite(w2) && w2 > 0.0f;
}
static bool os3_pointers_ok(const Os3In& i, const Os3Out& o, const void* ws) {
    if (!i.T1w || !i.xy_un1 || !i.point1 || !i.points1 || !i.assigned || !i.points2 || !i.flags2 || !i.index2 || !i.xy_un2 || !i.T2w || !i.S12 || !ws) return false;
    if (!o.assigned_out || !o.status || !o.chi2 || !o.state || !o.S12_out || !o.header || !o.final_chi2 || (i.Tmw && (!o.Tcw || !o.Ow))) return false;
    if (i.S12_stride < XFH_OS3_S12_FLOATS || o.S12_out_stride < XFH_OS3_S12_FLOATS) return false;
    return !misaligned(15, ws) && !misaligned(7, o.state, o.final_chi2) &&
           !misaligned(3, i.T1w, i.xy_un1, i.point1, i.points1, i.assigned, i.points2, i.index2, i.xy_un2, i.T2w, i.S12, i.Tmw, o.assigned_out, o.chi2, o.S12_out,
                       o.Tcw, o.Ow, o.header);
}
static Os3Cam os3_cam(const xfh_camera* c) { return Os3Cam{(double)c->fx, (double)c->fy, (double)c->cx, (double)c->cy}; }
static Os3Args os3_args(int n1, int M1, int nq, int n2, int side1_shared, const Os3In& i, const xfh_camera* cam1, const xfh_camera* cam2, float th2, int fix_scale,
                        int all_points, float w1, float w2, void* ws, const Os3Out& o) {
    Os3Args a = {};
    a.n1 = n1; a.M1 = M1; a.nq = nq; a.n2 = n2; a.side1_shared = side1_shared; a.fix_scale = fix_scale; a.all_points = all_points;
    a.T1w = i.T1w; a.xy_un1 = i.xy_un1; a.points1 = i.points1; a.point1 = i.point1; a.assigned = i.assigned; a.points2 = i.points2; a.flags2 = i.flags2;
    a.index2 = i.index2; a.xy_un2 = i.xy_un2; a.T2w = i.T2w; a.S12 = i.S12; a.S12_stride = i.S12_stride; a.Tmw = i.Tmw;
    a.cam1 = os3_cam(cam1); a.cam2 = os3_cam(cam2); a.th2 = (double)th2; a.w1 = (double)w1; a.w2 = (double)w2; a.delta = (double)sqrtf(th2);
    a.ws = (char*)ws; a.ws_stride = os3_ws_bytes(n1);
    a.assigned_out = o.assigned_out; a.status = o.status; a.chi2 = o.chi2; a.state = o.state; a.S12_out = o.S12_out; a.S12_out_stride = o.S12_out_stride;
    a.Tcw = o.Tcw; a.Ow = o.Ow; a.header = o.header; a.final_chi2 = o.final_chi2;
    return a;
}
static Os3Sim os3_of(const double* p) { return Os3Sim{{p[0], p[1], p[2], p[3]}, {p[4], p[5], p[6]}, p[7]}; }
static void os3_put(const Os3Sim& S, double* p) { for (int k = 0; k < 4; ++k) p[k] = S.q[k]; for (int k = 0; k < 3; ++k) p[4 + k] = S.t[k]; p[7] = S.s; }

extern "C" {

int xfh_sim3_state_from(const float* S13, double* state8) {
    if (!S13 || !state8) return XFH_ERR_INVALID_ARG;
    Os3Sim S;
    os3_from_floats(S13, &S);
    os3_put(S, state8);
    return XFH_OK;
}

int xfh_sim3_state_to(const double* state8, float* S13) {
    if (!S13 || !state8) return XFH_ERR_INVALID_ARG;
    os3_to_floats(os3_of(state8), S13);
    return XFH_OK;
}

int xfh_sim3_oplus(const double* state8, const double* update7, int fix_scale, double* state8_out) {
    if (!state8 || !update7 || !state8_out) return XFH_ERR_INVALID_ARG;
    Os3Sim o;
    os3_oplus(update7, os3_of(state8), fix_scale, &o);
    os3_put(o, state8_out);
    return XFH_OK;
}

int xfh_sim3_map(const double* state8, const double* point3, double* out3) {
    if (!state8 || !point3 || !out3) return XFH_ERR_INVALID_ARG;
    os3_map(os3_of(state8), point3, out3);
    return XFH_OK;
}

int xfh_sim3_inverse_map(const double* state8, const double* point3, double* out3) {
    if (!state8 || !point3 || !out3) return XFH_ERR_INVALID_ARG;
    Os3Sim inv;
    os3_inverse(os3_of(state8), &inv);
    os3_map(inv, point3, out3);
    return XFH_OK;
}

int xfh_sim3_solve7(const double* H28, double lambda, const double* b7, double* x7) {
    if (!H28 || !b7 || !x7) return 0;
    return geo_ldlt_solve<7>(H28, lambda, b7, x7) ? 1 : 0;
}

int xfh_sim3_edge(const double* state8, const xfh_camera* cam1, const xfh_camera* cam2, const float* P3D1c, const float* P3D2c, const float* obs1, const float* obs2,
                  float inv_sigma2_1, float inv_sigma2_2, float th2, int fix_scale, int robust, double* error4, double* chi2_2, double* jacobian28, double* rho1_2) {
    if (!state8 || !cam1 || !cam2 || !P3D1c || !P3D2c || !obs1 || !obs2) return XFH_ERR_INVALID_ARG;
    const Os3Sim est = os3_of(state8);
    Os3Sims S;
    for (int j = 0; j < 15; ++j) os3_sims_piece(est, fix_scale, j, &S);
    const Os3Cam k1 = os3_cam(cam1), k2 = os3_cam(cam2);
    const double X1[3] = {(double)P3D1c[0], (double)P3D1c[1], (double)P3D1c[2]}, X2[3] = {(double)P3D2c[0], (double)P3D2c[1], (double)P3D2c[2]};
    const double o1[2] = {(double)obs1[0], (double)obs1[1]}, o2[2] = {(double)obs2[0], (double)obs2[1]};
    double e[4], c[2], J[28], r0, r1[2] = {1.0, 1.0};
    c[0] = os3_edge_error(S.est, k1, X2, o1, (double)inv_sigma2_1, e);
    c[1] = os3_edge_error(S.inv, k2, X1, o2, (double)inv_sigma2_2, e + 2);
    os3_edge_jacobian(S.pert, k1, X2, o1, J);
    os3_edge_jacobian(S.pinv, k2, X1, o2, J + 14);
    if (robust) { pose_huber(c[0], (double)sqrtf(th2), &r0, &r1[0]); pose_huber(c[1], (double)sqrtf(th2), &r0, &r1[1]); }
    if (error4) for (int k = 0; k < 4; ++k) error4[k] = e[k];
    if (chi2_2) { chi2_2[0] = c[0]; chi2_2[1] = c[1]; }
    if (jacobian28) for (int k = 0; k < 28; ++k) jacobian28[k] = J[k];
    if (rho1_2) { rho1_2[0] = r1[0]; rho1_2[1] = r1[1]; }
    return XFH_OK;
}

size_t xfh_sim3_optimize_workspace_bytes(int n1, int B) {
    if (n1 < 1 || n1 > XFH_GRID_MAX_N || B < 1 || B > 65535) return 0;
    return os3_ws_bytes(n1) * (size_t)B;
}

int xfh_sim3_optimize_host(int B, int n1, int M1, int nq, int n2, int side1_shared, const float* T1w, const float* xy_un1, const int* point1, const float* points1,
                           const int* assigned, const float* points2, const uint8_t* flags2, const int* index2, const float* xy_un2, const float* T2w,
                           const float* S12, size_t S12_problem_stride, const float* Tmw_or_null, const xfh_camera* cam1, const xfh_camera* cam2, float th2,
                           int fix_scale, int all_points, float inv_sigma2_1, float inv_sigma2_2, void* workspace, int* assigned_out, uint8_t* pair_status,
                           float* chi2, double* state, float* S12_out, size_t S12_out_problem_stride, float* Tcw, float* Ow, int* header, double* final_chi2) {
    const Os3In in{T1w, xy_un1, point1, points1, assigned, points2, flags2, index2, xy_un2, T2w, S12, S12_problem_stride, Tmw_or_null};
    const Os3Out out{assigned_out, pair_status, chi2, state, S12_out, S12_out_problem_stride, Tcw, Ow, header, final_chi2};
    if (!os3_scalars_ok(B, n1, M1, nq, n2, side1_shared, cam1, cam2, th2, fix_scale, all_points, inv_sigma2_1, inv_sigma2_2) || !os3_pointers_ok(in, out, workspace))
        return XFH_ERR_INVALID_ARG;
    const Os3Args a = os3_args(n1, M1, nq, n2, side1_shared, in, cam1, cam2, th2, fix_scale, all_points, inv_sigma2_1, inv_sigma2_2, workspace, out);
    for (int b = 0; b < B; ++b) os3_host_problem(a, b);
    return XFH_OK;
}

int xfh_sim3_optimize_device(xfh_ctx* c, int B, int n1, int M1, int nq, int n2, int side1_shared, const float* d_T1w, const float* d_xy_un1, const int* d_point1,
                             const float* d_points1, const int* d_assigned, const float* d_points2, const uint8_t* d_flags2, const int* d_index2,
                             const float* d_xy_un2, const float* d_T2w, const float* d_S12, size_t S12_problem_stride, const float* d_Tmw_or_null,
                             const xfh_camera* cam1, const xfh_camera* cam2, float th2, int fix_scale, int all_points, float inv_sigma2_1, float inv_sigma2_2,
                             void* d_workspace, int* d_assigned_out, uint8_t* d_pair_status, float* d_chi2, double* d_state, float* d_S12_out,
                             size_t S12_out_problem_stride, float* d_Tcw, float* d_Ow, int* d_header, double* d_final_chi2) {
    const Os3In in{d_T1w, d_xy_un1, d_point1, d_points1, d_assigned, d_points2, d_flags2, d_index2, d_xy_un2, d_T2w, d_S12, S12_problem_stride, d_Tmw_or_null};
    const Os3Out out{d_assigned_out, d_pair_status, d_chi2, d_state, d_S12_out, S12_out_problem_stride, d_Tcw, d_Ow, d_header, d_final_chi2};
    if (!c || !os3_scalars_ok(B, n1, M1, nq, n2, side1_shared, cam1, cam2, th2, fix_scale, all_points, inv_sigma2_1, inv_sigma2_2) ||
        !os3_pointers_ok(in, out, d_workspace)) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    const Os3Args a = os3_args(n1, M1, nq, n2, side1_shared, in, cam1, cam2, th2, fix_scale, all_points, inv_sigma2_1, inv_sigma2_2, d_workspace, out);
    HIPCK(c, launch_sim3_optimize(c, a, B));
    return XFH_OK;
}

int xfh_sim3_optimize(xfh_ctx* c, int n1, int M1, int nq, int n2, const float* T1w, const float* xy_un1, const int* point1, const float* points1,
                      const int* assigned, const float* points2, const uint8_t* flags2, const int* index2, const float* xy_un2, const float* T2w, const float* S12,
                      const float* Tmw_or_null, const xfh_camera* cam1, const xfh_camera* cam2, float th2, int fix_scale, int all_points, float inv_sigma2_1,
                      float inv_sigma2_2, int* assigned_out, uint8_t* pair_status, float* chi2, double* state, float* S12_out, float* Tcw, float* Ow, int* header,
                      double* final_chi2) {
    if (!c || !os3_scalars_ok(1, n1, M1, nq, n2, 0, cam1, cam2, th2, fix_scale, all_points, inv_sigma2_1, inv_sigma2_2)) return XFH_ERR_INVALID_ARG;
    if (!T1w || !xy_un1 || !point1 || !points1 || !assigned || !points2 || !flags2 || !index2 || !xy_un2 || !T2w || !S12 || !assigned_out || !pair_status || !chi2 ||
        !state || !S12_out || !header || !final_chi2 || (Tmw_or_null && (!Tcw || !Ow))) return XFH_ERR_INVALID_ARG;
    const size_t N1 = (size_t)n1, NQ = (size_t)nq;
    HostStage s{c};
    auto t1 = s.in<float>(T1w, 48); auto k1 = s.in<float>(xy_un1, N1 * 8); auto p1 = s.in<int>(point1, N1 * 4); auto x1 = s.in<float>(points1, (size_t)M1 * 12);
    auto as = s.in<int>(assigned, N1 * 4); auto x2 = s.in<float>(points2, NQ * 12); auto f2 = s.in<uint8_t>(flags2, NQ); auto i2 = s.in<int>(index2, NQ * 4);
    auto k2 = s.in<float>(xy_un2, (size_t)n2 * 8); auto t2 = s.in<float>(T2w, 48); auto s12 = s.in<float>(S12, XFH_OS3_S12_FLOATS * 4);
    auto tm = s.in_opt<float>(Tmw_or_null, 48);
    auto ws = s.tmp<char>(xfh_sim3_optimize_workspace_bytes(n1, 1));
    auto oa = s.out<int>(assigned_out, N1 * 4); auto os = s.out<uint8_t>(pair_status, N1); auto oc = s.out<float>(chi2, N1 * 8); auto ost = s.out<double>(state, 64);
    auto o12 = s.out<float>(S12_out, XFH_OS3_S12_FLOATS * 4);
    auto oT = s.out_opt<float>(Tmw_or_null ? Tcw : nullptr, 48); auto oO = s.out_opt<float>(Tmw_or_null ? Ow : nullptr, 12);
    auto oh = s.out<int>(header, XFH_OS3_HEADER_INTS * 4); auto of = s.out<double>(final_chi2, 8);
    if (const int rc = s.upload(); rc != XFH_OK) return rc;
    const int rc = xfh_sim3_optimize_device(c, 1, n1, M1, nq, n2, 0, t1, k1, p1, x1, as, x2, f2, i2, k2, t2, s12, XFH_OS3_S12_FLOATS, tm, cam1, cam2, th2, fix_scale,
                                            all_points, inv_sigma2_1, inv_sigma2_2, (char*)ws, oa, os, oc, ost, o12, XFH_OS3_S12_FLOATS, oT, oO, oh, of);
    if (rc != XFH_OK) return rc;                                              // (a HIP error: every argument check has passed above)
    return s.download();
}

}  // extern "C"
