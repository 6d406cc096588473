// capi_lba.cpp -- the entry points of include/xfeat_hip.h behind Optimizer::LocalBundleAdjustment (xfh_local_ba*, xfh_lba_edge, _point_block, _solve) and xfh_debug_lba_solve of
// include/xfeat_hip_bench.h: the
// pieces of the rule on the host (lba_math.h, the kernels' own lines), the whole rule on one host thread, the device form and the host-pointer form.
#include "host_stage.h"
#include "lba_math.h"
#include <math.h>
#include <string.h>

static_assert(XFH_LBA_MAX_FREE_KF == XFH_LBA_MAX_FREE && XFH_LBA_HDR_INTS == XFH_LBA_HEADER_INTS && LBA_OK == XFH_LBA_OK && LBA_ABORTED == XFH_LBA_ABORTED &&
              LBA_NOTHING_FREE == XFH_LBA_NOTHING_FREE && LBA_FREE_MISMATCH == XFH_LBA_FREE_MISMATCH && XFH_LBA_ITERATIONS_MAX == XFH_LBA_MAX_ITERATIONS,
              "lba_math.h and include/xfeat_hip.h name the same values");

static bool lba_scalars_ok(int nK, int n_free, int nP, int nE, int pose_rows, int point_rows, const xfh_camera* cam, float inv_sigma2, int max_iterations, int write_back) {
    if (nK < 1 || nK > XFH_LBA_MAX_KF || nP < 1 || nP > XFH_LBA_MAX_POINTS || nE < 1 || nE > XFH_LBA_MAX_EDGES || pose_rows < 1 || point_rows < 1) return false;
    if (n_free < 0 || n_free > nK || n_free > XFH_LBA_MAX_FREE_KF || !cam || max_iterations < 1 || max_iterations > XFH_LBA_ITERATIONS_MAX) return false;
    return write_back >= 0 && write_back <= 1 && isfinite(inv_sigma2) && inv_sigma2 > 0.0f;
}
static bool lba_pointers_ok(const LbaArgs& a) {
    if (!a.pose_table || !a.point_table || !a.kf_row || !a.kf_fixed || !a.point_row || !a.edge_begin || !a.edge_kf || !a.edge_obs || !a.ws) return false;
    if (!a.Tcw_out || !a.points_out || !a.erase || !a.chi2 || !a.header || !a.final_chi2) return false;
    return !misaligned(15, a.ws) && !misaligned(7, a.final_chi2) &&
           !misaligned(3, a.pose_table, a.point_table, a.kf_row, a.point_row, a.edge_begin, a.edge_kf, a.edge_obs, a.Tcw_out, a.points_out, a.chi2, a.header);
}
static LbaArgs lba_args(int nK, int n_free, int nP, int nE, float* pose_table, int pose_rows, float* point_table, int point_rows, const int* kf_row,
                        const uint8_t* kf_fixed, const int* point_row, const int* edge_begin, const int* edge_kf, const float* edge_obs, const xfh_camera* cam,
                        float inv_sigma2, int max_iterations, int write_back, void* ws, float* Tcw_out, float* points_out, uint8_t* erase, float* chi2, int* header,
                        double* final_chi2) {
    LbaArgs a = {};
    a.nK = nK; a.nP = nP; a.nE = nE; a.n_free = n_free; a.pose_rows = pose_rows; a.point_rows = point_rows; a.max_it = max_iterations; a.write_back = write_back;
    a.pose_table = pose_table; a.point_table = point_table; a.kf_row = kf_row; a.kf_fixed = kf_fixed; a.point_row = point_row; a.edge_begin = edge_begin;
    a.edge_kf = edge_kf; a.edge_obs = edge_obs;
    if (cam) a.cam = PoseCam{(double)cam->fx, (double)cam->fy, (double)cam->cx, (double)cam->cy, (double)cam->bf};
    a.w = (double)inv_sigma2;
    a.Tcw_out = Tcw_out; a.points_out = points_out; a.erase = erase; a.chi2 = chi2; a.header = header; a.final_chi2 = final_chi2; a.ws = (char*)ws;
    return a;
}

// the workspace image up, k_lba_solve once, the workspace image back (xfh_debug_lba_solve)
static int lba_solve_staged(xfh_ctx* c, LbaArgs a, char* host, size_t bytes) {
    HostStage s{c};
    auto ws = s.add<char>(bytes, host, host, false);
    if (const int rc = s.upload(); rc != XFH_OK) return rc;
    a.ws = (char*)ws;
    HIPCK(c, launch_lba_solve_alone(c, a));
    return s.download();
}

extern "C" {

int xfh_lba_edge(const double* pose7, const double* point3, const xfh_camera* cam, const float* obs3, float inv_sigma2, double* error3, double* chi2,
                 double* jacobian_pose18, double* jacobian_point9, double* rho1) {
    if (!pose7 || !point3 || !cam || !obs3) return XFH_ERR_INVALID_ARG;
    const PosePose P = lba_pose_get(pose7);
    const PoseCam k{(double)cam->fx, (double)cam->fy, (double)cam->cx, (double)cam->cy, (double)cam->bf};
    const double obs[3] = {(double)obs3[0], (double)obs3[1], (double)obs3[2]};
    LbaLin L;
    lba_edge_linearize(P, k, point3, obs, !(obs3[2] < 0.0f), (double)inv_sigma2, &L);
    if (error3) for (int n = 0; n < 3; ++n) error3[n] = L.e[n];
    if (chi2) *chi2 = L.chi2;
    if (jacobian_pose18) for (int n = 0; n < 18; ++n) jacobian_pose18[n] = L.Jp[n];
    if (jacobian_point9) for (int n = 0; n < 9; ++n) jacobian_point9[n] = L.Jl[n];
    if (rho1) *rho1 = L.rho1;
    return XFH_OK;
}

int xfh_lba_point_block(const double* H6, double lambda, double* Dinv9) {
    if (!H6 || !Dinv9) return XFH_ERR_INVALID_ARG;
    lba_point_block(H6, lambda, Dinv9);
    return XFH_OK;
}

int xfh_lba_solve(int n, double* S, const double* b, double* x) {
    if (n < 1 || n > 6 * XFH_LBA_MAX_FREE_KF || !S || !b || !x) return 0;
    double y[6 * XFH_LBA_MAX_FREE_KF];
    return lba_ldlt_solve_host(S, n, b, x, y) ? 1 : 0;
}

size_t xfh_local_ba_workspace_bytes(int nK, int nP, int nE, int n_free) {
    if (nK < 1 || nK > XFH_LBA_MAX_KF || nP < 1 || nP > XFH_LBA_MAX_POINTS || nE < 1 || nE > XFH_LBA_MAX_EDGES || n_free < 0 || n_free > nK ||
        n_free > XFH_LBA_MAX_FREE_KF) return 0;
    return lba_ws(nullptr, nK, nP, nE, n_free).bytes;
}

int xfh_local_ba_host(int nK, int n_free, int nP, int nE, float* pose_table, int pose_rows, float* point_table, int point_rows, const int* kf_row,
                      const uint8_t* kf_fixed, const int* point_row, const int* edge_begin, const int* edge_kf, const float* edge_obs, const xfh_camera* cam,
                      float inv_sigma2, int max_iterations, int write_back, void* workspace, float* Tcw_out, float* points_out, uint8_t* erase, float* chi2,
                      int* header, double* final_chi2) {
    const LbaArgs a = lba_args(nK, n_free, nP, nE, pose_table, pose_rows, point_table, point_rows, kf_row, kf_fixed, point_row, edge_begin, edge_kf, edge_obs, cam,
                               inv_sigma2, max_iterations, write_back, workspace, Tcw_out, points_out, erase, chi2, header, final_chi2);
    if (!lba_scalars_ok(nK, n_free, nP, nE, pose_rows, point_rows, cam, inv_sigma2, max_iterations, write_back) || !lba_pointers_ok(a)) return XFH_ERR_INVALID_ARG;
    lba_host_run(a);
    return XFH_OK;
}

int xfh_local_ba_device(xfh_ctx* c, int nK, int n_free, int nP, int nE, float* d_pose_table, int pose_rows, float* d_point_table, int point_rows,
                        const int* d_kf_row, const uint8_t* d_kf_fixed, const int* d_point_row, const int* d_edge_begin, const int* d_edge_kf,
                        const float* d_edge_obs, const xfh_camera* cam, float inv_sigma2, int max_iterations, int write_back, void* d_workspace, float* d_Tcw_out,
                        float* d_points_out, uint8_t* d_erase, float* d_chi2, int* d_header, double* d_final_chi2) {
    const LbaArgs a = lba_args(nK, n_free, nP, nE, d_pose_table, pose_rows, d_point_table, point_rows, d_kf_row, d_kf_fixed, d_point_row, d_edge_begin, d_edge_kf,
                               d_edge_obs, cam, inv_sigma2, max_iterations, write_back, d_workspace, d_Tcw_out, d_points_out, d_erase, d_chi2, d_header, d_final_chi2);
    if (!c || !lba_scalars_ok(nK, n_free, nP, nE, pose_rows, point_rows, cam, inv_sigma2, max_iterations, write_back) || !lba_pointers_ok(a)) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, launch_local_ba(c, a));
    return XFH_OK;
}

int xfh_local_ba(xfh_ctx* c, int nK, int n_free, int nP, int nE, float* pose_table, int pose_rows, float* point_table, int point_rows, const int* kf_row,
                 const uint8_t* kf_fixed, const int* point_row, const int* edge_begin, const int* edge_kf, const float* edge_obs, const xfh_camera* cam, float inv_sigma2,
                 int max_iterations, int write_back, float* Tcw_out, float* points_out, uint8_t* erase, float* chi2, int* header, double* final_chi2) {
    if (!c || !lba_scalars_ok(nK, n_free, nP, nE, pose_rows, point_rows, cam, inv_sigma2, max_iterations, write_back)) return XFH_ERR_INVALID_ARG;
    if (!pose_table || !point_table || !kf_row || !kf_fixed || !point_row || !edge_begin || !edge_kf || !edge_obs || !Tcw_out || !points_out || !erase || !chi2 ||
        !header || !final_chi2) return XFH_ERR_INVALID_ARG;
    const size_t K = (size_t)nK, P = (size_t)nP, E = (size_t)nE;
    HostStage s{c};
    auto tp = s.add<float>((size_t)pose_rows * 48, pose_table, write_back ? pose_table : nullptr, false);      // the two tables go up, and come back when written
    auto tx = s.add<float>((size_t)point_rows * 12, point_table, write_back ? point_table : nullptr, false);
    auto kr = s.in<int>(kf_row, K * 4); auto kf = s.in<uint8_t>(kf_fixed, K); auto pr = s.in<int>(point_row, P * 4); auto eb = s.in<int>(edge_begin, (P + 1) * 4);
    auto ek = s.in<int>(edge_kf, E * 4); auto eo = s.in<float>(edge_obs, E * 12);
    auto ws = s.tmp<char>(xfh_local_ba_workspace_bytes(nK, nP, nE, n_free));
    auto oT = s.out<float>(Tcw_out, K * 48); auto oX = s.out<float>(points_out, P * 12); auto oe = s.out<uint8_t>(erase, E); auto oc = s.out<float>(chi2, E * 4);
    auto oh = s.out<int>(header, XFH_LBA_HDR_INTS * 4); auto of = s.out<double>(final_chi2, 8);
    if (const int rc = s.upload(); rc != XFH_OK) return rc;
    const int rc = xfh_local_ba_device(c, nK, n_free, nP, nE, tp, pose_rows, tx, point_rows, kr, kf, pr, eb, ek, eo, cam, inv_sigma2, max_iterations, write_back, (char*)ws,
                                       oT, oX, oe, oc, oh, of);
    if (rc != XFH_OK) return rc;
    return s.download();
}

// include/xfeat_hip_bench.h: k_lba_solve alone.  The workspace of a problem of one keyframe slot, one point and one edge with n / 6 free keyframes is made on
// the host -- every byte ws_fill, then the control block at the TRIAL step of iteration 0 and S, b and x where lba_ws puts them -- and travels both ways whole.
int xfh_debug_lba_solve(xfh_ctx* c, int n, double* S, const double* b, double* x, int ws_fill, int* solved) {
    if (!c || n < 6 || n > 6 * XFH_LBA_MAX_FREE_KF || n % 6 != 0 || !S || !b || !x || !solved) return XFH_ERR_INVALID_ARG;
    LbaArgs a = {};
    a.nK = 1; a.nP = 1; a.nE = 1; a.n_free = n / 6; a.max_it = 1;
    const size_t bytes = lba_ws(nullptr, a.nK, a.nP, a.nE, a.n_free).bytes, N = (size_t)n;
    char* host = (char*)malloc(bytes);
    if (!host) return XFH_ERR_OUT_OF_MEMORY;
    memset(host, ws_fill & 255, bytes);
    const LbaWs w = lba_ws(host, a.nK, a.nP, a.nE, a.n_free);
    LbaCtl ctl = {};
    ctl.act = LBA_TRIAL; ctl.iter = 0; ctl.max_it = 1; ctl.ni = 2.0; ctl.solved = -1;
    *w.ctl = ctl;
    memcpy(w.S, S, N * N * 8); memcpy(w.bS, b, N * 8); memcpy(w.xp, x, N * 8);
    const int rc = lba_solve_staged(c, a, host, bytes);
    if (rc == XFH_OK) {
        memcpy(S, w.S, N * N * 8); memcpy(x, w.xp, N * 8);
        *solved = w.ctl->solved;
    }
    free(host);
    return rc;
}

}  // extern "C"
