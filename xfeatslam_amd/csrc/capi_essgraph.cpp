// capi_essgraph.cpp -- the entry points of include/xfeat_hip.h behind Optimizer::OptimizeEssentialGraph (xfh_essential_graph*, xfh_sim3_log, xfh_eg_edge,
// xfh_eg_solve) and xfh_debug_eg_solve of include/xfeat_hip_bench.h: the pieces of the rule on the host (essgraph_math.h, the kernels' own lines), the whole
// rule on one host thread, the device form with its read-back loop and the host-pointer form.
#include "host_stage.h"
#include "essgraph_math.h"
#include <math.h>
#include <string.h>

static_assert(XFH_EG_MAX_FREE_V == XFH_EG_MAX_FREE && XFH_EG_HDR_INTS == XFH_EG_HEADER_INTS && EG_OK == XFH_EG_OK && EG_NOTHING_FREE == XFH_EG_NOTHING_FREE &&
              EG_FREE_MISMATCH == XFH_EG_FREE_MISMATCH && EG_NO_EDGES == XFH_EG_NO_EDGES && XFH_EG_ITERATIONS_MAX == XFH_EG_MAX_ITERATIONS,
              "essgraph_math.h and include/xfeat_hip.h name the same values");

static bool eg_scalars_ok(int nV, int n_free, int nE, int nP, int nS, int pose_rows, int point_rows, int fix_scale, int max_iterations, int write_back) {
    if (nV < 1 || nV > XFH_EG_MAX_V || nP < 1 || nP > XFH_EG_MAX_POINTS || nE < 1 || nE > XFH_EG_MAX_EDGES || nS < 1 || nS > XFH_EG_MAX_SIM3) return false;
    if (pose_rows < 1 || point_rows < 1 || n_free < 0 || n_free > nV || n_free > XFH_EG_MAX_FREE_V) return false;
    return max_iterations >= 1 && max_iterations <= XFH_EG_ITERATIONS_MAX && write_back >= 0 && write_back <= 1 && fix_scale >= 0 && fix_scale <= 1;
}
static bool eg_pointers_ok(const EgArgs& a) {
    if (!a.pose_table || !a.point_table || !a.kf_row || !a.kf_fixed || !a.corrected_index || !a.noncorrected_index || !a.sim3 || !a.edge_i || !a.edge_j ||
        !a.edge_kind || !a.point_row || !a.point_ref || !a.ws) return false;
    if (!a.Sim3_out || !a.Tcw_out || !a.points_out || !a.chi2 || !a.header || !a.final_chi2) return false;
    return !misaligned(15, a.ws) && !misaligned(7, a.sim3, a.Sim3_out, a.final_chi2) &&
           !misaligned(3, a.pose_table, a.point_table, a.kf_row, a.corrected_index, a.noncorrected_index, a.edge_i, a.edge_j, a.edge_kind, a.point_row, a.point_ref,
                       a.Tcw_out, a.points_out, a.chi2, a.header);
}
static EgArgs eg_args(int nV, int n_free, int nE, int nP, int nS, float* pose_table, int pose_rows, float* point_table, int point_rows, const int* kf_row,
                      const uint8_t* kf_fixed, const int* corrected_index, const int* noncorrected_index, const double* sim3, const int* edge_i, const int* edge_j,
                      const int* edge_kind, const int* point_row, const int* point_ref, int fix_scale, int max_iterations, int write_back, void* ws,
                      double* Sim3_out, float* Tcw_out, float* points_out, float* chi2, int* header, double* final_chi2) {
    EgArgs a = {};
    a.nV = nV; a.nP = nP; a.nE = nE; a.nS = nS; a.n_free = n_free; a.pose_rows = pose_rows; a.point_rows = point_rows; a.max_it = max_iterations;
    a.write_back = write_back; a.fix_scale = fix_scale;
    a.pose_table = pose_table; a.point_table = point_table; a.kf_row = kf_row; a.kf_fixed = kf_fixed; a.corrected_index = corrected_index;
    a.noncorrected_index = noncorrected_index; a.sim3 = sim3; a.edge_i = edge_i; a.edge_j = edge_j; a.edge_kind = edge_kind; a.point_row = point_row;
    a.point_ref = point_ref;
    a.Sim3_out = Sim3_out; a.Tcw_out = Tcw_out; a.points_out = points_out; a.chi2 = chi2; a.header = header; a.final_chi2 = final_chi2; a.ws = (char*)ws;
    return a;
}

extern "C" {

int xfh_sim3_log(const double* sim8, double* log7) {
    if (!sim8 || !log7) return XFH_ERR_INVALID_ARG;
    eg_sim3_log(eg_sim_get(sim8), log7);
    return XFH_OK;
}

int xfh_eg_edge(const double* meas8, const double* Si8, const double* Sj8, int free_i, int free_j, int fix_scale, double* error7, double* chi2,
                double* jacobian_i49, double* jacobian_j49) {
    if (!meas8 || !Si8 || !Sj8) return XFH_ERR_INVALID_ARG;
    const Os3Sim Si = eg_sim_get(Si8), Sj = eg_sim_get(Sj8);
    double perti[14 * 8], pinvj[14 * 8], e[7], Ji[49], Jj[49];
    Os3Sims si, sj;
    for (int k = 0; k < 15; ++k) { os3_sims_piece(Si, fix_scale ? 1 : 0, k, &si); os3_sims_piece(Sj, fix_scale ? 1 : 0, k, &sj); }
    for (int k = 0; k < 14; ++k) { eg_sim_put(si.pert[k], perti + 8 * k); eg_sim_put(sj.pinv[k], pinvj + 8 * k); }
    const double c = eg_edge_linearize(eg_sim_get(meas8), Si, sj.inv, perti, pinvj, free_i != 0, free_j != 0, e, Ji, Jj);
    if (error7) for (int n = 0; n < 7; ++n) error7[n] = e[n];
    if (chi2) *chi2 = c;
    if (jacobian_i49) for (int n = 0; n < 49; ++n) jacobian_i49[n] = Ji[n];
    if (jacobian_j49) for (int n = 0; n < 49; ++n) jacobian_j49[n] = Jj[n];
    return XFH_OK;
}

int xfh_eg_solve(int n, double* S, const double* b, double* x) {
    if (n < 1 || n > 7 * XFH_EG_MAX_FREE_V || !S || !b || !x) return 0;
    double* y = (double*)malloc(sizeof(double) * (size_t)n);
    if (!y) return 0;
    const bool ok = lba_ldlt_solve_host(S, n, b, x, y);
    free(y);
    return ok ? 1 : 0;
}

size_t xfh_essential_graph_workspace_bytes(int nV, int nE, int n_free) {
    if (nV < 1 || nV > XFH_EG_MAX_V || nE < 1 || nE > XFH_EG_MAX_EDGES || n_free < 0 || n_free > nV || n_free > XFH_EG_MAX_FREE_V) return 0;
    return eg_ws(nullptr, nV, nE, n_free).bytes;
}

int xfh_essential_graph_host(int nV, int n_free, int nE, int nP, int nS, float* pose_table, int pose_rows, float* point_table, int point_rows, const int* kf_row,
                             const uint8_t* kf_fixed, const int* corrected_index, const int* noncorrected_index, const double* sim3, const int* edge_i,
                             const int* edge_j, const int* edge_kind, const int* point_row, const int* point_ref, int fix_scale, int max_iterations, int write_back,
                             void* workspace, double* Sim3_out, float* Tcw_out, float* points_out, float* chi2, int* header, double* final_chi2) {
    const EgArgs a = eg_args(nV, n_free, nE, nP, nS, pose_table, pose_rows, point_table, point_rows, kf_row, kf_fixed, corrected_index, noncorrected_index, sim3,
                             edge_i, edge_j, edge_kind, point_row, point_ref, fix_scale, max_iterations, write_back, workspace, Sim3_out, Tcw_out, points_out, chi2,
                             header, final_chi2);
    if (!eg_scalars_ok(nV, n_free, nE, nP, nS, pose_rows, point_rows, fix_scale, max_iterations, write_back) || !eg_pointers_ok(a)) return XFH_ERR_INVALID_ARG;
    eg_host_run(a);
    return XFH_OK;
}

// the plan, then one step at a time with the control record read back after every trial: at most max_iterations x 10 reads.  A HIP error at any read ends
// the loop and is returned.
int xfh_essential_graph_device(xfh_ctx* c, int nV, int n_free, int nE, int nP, int nS, float* d_pose_table, int pose_rows, float* d_point_table, int point_rows,
                               const int* d_kf_row, const uint8_t* d_kf_fixed, const int* d_corrected_index, const int* d_noncorrected_index, const double* d_sim3,
                               const int* d_edge_i, const int* d_edge_j, const int* d_edge_kind, const int* d_point_row, const int* d_point_ref, int fix_scale,
                               int max_iterations, int write_back, void* d_workspace, double* d_Sim3_out, float* d_Tcw_out, float* d_points_out, float* d_chi2,
                               int* d_header, double* d_final_chi2) {
    const EgArgs a = eg_args(nV, n_free, nE, nP, nS, d_pose_table, pose_rows, d_point_table, point_rows, d_kf_row, d_kf_fixed, d_corrected_index,
                             d_noncorrected_index, d_sim3, d_edge_i, d_edge_j, d_edge_kind, d_point_row, d_point_ref, fix_scale, max_iterations, write_back,
                             d_workspace, d_Sim3_out, d_Tcw_out, d_points_out, d_chi2, d_header, d_final_chi2);
    if (!c || !eg_scalars_ok(nV, n_free, nE, nP, nS, pose_rows, point_rows, fix_scale, max_iterations, write_back) || !eg_pointers_ok(a)) return XFH_ERR_INVALID_ARG;
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, launch_eg_plan(c, a));
    const EgWs w = eg_ws(a.ws, nV, nE, n_free);
    int act = EG_BUILD;
    for (int reads = 0; reads < max_iterations * GEO_LM_MAX_TRIALS && act != EG_DONE; ++reads) {
        if (act == EG_BUILD) HIPCK(c, launch_eg_build(c, a));
        HIPCK(c, launch_eg_trial(c, a));
        EgCtl ctl;
        HIPCK(c, hipMemcpyAsync(&ctl, w.ctl, sizeof(EgCtl), hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));
        act = ctl.act;
    }
    HIPCK(c, launch_eg_finish(c, a));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return XFH_OK;
}

int xfh_essential_graph(xfh_ctx* c, int nV, int n_free, int nE, int nP, int nS, float* pose_table, int pose_rows, float* point_table, int point_rows,
                        const int* kf_row, const uint8_t* kf_fixed, const int* corrected_index, const int* noncorrected_index, const double* sim3, const int* edge_i,
                        const int* edge_j, const int* edge_kind, const int* point_row, const int* point_ref, int fix_scale, int max_iterations, int write_back,
                        double* Sim3_out, float* Tcw_out, float* points_out, float* chi2, int* header, double* final_chi2) {
    if (!c || !eg_scalars_ok(nV, n_free, nE, nP, nS, pose_rows, point_rows, fix_scale, max_iterations, write_back)) return XFH_ERR_INVALID_ARG;
    if (!pose_table || !point_table || !kf_row || !kf_fixed || !corrected_index || !noncorrected_index || !sim3 || !edge_i || !edge_j || !edge_kind || !point_row ||
        !point_ref || !Sim3_out || !Tcw_out || !points_out || !chi2 || !header || !final_chi2) return XFH_ERR_INVALID_ARG;
    const size_t V = (size_t)nV, P = (size_t)nP, E = (size_t)nE;
    HostStage s{c};
    auto tp = s.add<float>((size_t)pose_rows * 48, pose_table, write_back ? pose_table : nullptr, false);      // the two tables go up, and come back when written
    auto tx = s.add<float>((size_t)point_rows * 12, point_table, write_back ? point_table : nullptr, false);
    auto kr = s.in<int>(kf_row, V * 4); auto kf = s.in<uint8_t>(kf_fixed, V); auto ci = s.in<int>(corrected_index, V * 4);
    auto ni = s.in<int>(noncorrected_index, V * 4); auto sm = s.in<double>(sim3, (size_t)nS * 64);
    auto ei = s.in<int>(edge_i, E * 4); auto ej = s.in<int>(edge_j, E * 4); auto ek = s.in<int>(edge_kind, E * 4);
    auto pr = s.in<int>(point_row, P * 4); auto pf = s.in<int>(point_ref, P * 4);
    auto ws = s.tmp<char>(xfh_essential_graph_workspace_bytes(nV, nE, n_free));
    auto oS = s.out<double>(Sim3_out, V * 64); auto oT = s.out<float>(Tcw_out, V * 48); auto oX = s.out<float>(points_out, P * 12); auto oc = s.out<float>(chi2, E * 4);
    auto oh = s.out<int>(header, XFH_EG_HDR_INTS * 4); auto of = s.out<double>(final_chi2, 8);
    if (const int rc = s.upload(); rc != XFH_OK) return rc;
    const int rc = xfh_essential_graph_device(c, nV, n_free, nE, nP, nS, tp, pose_rows, tx, point_rows, kr, kf, ci, ni, sm, ei, ej, ek, pr, pf, fix_scale, max_iterations,
                                              write_back, (char*)ws, oS, oT, oX, oc, oh, of);
    if (rc != XFH_OK) return rc;
    return s.download();
}

// include/xfeat_hip_bench.h: the blocked factorisation and the substitutions alone, the kernels the call launches and no copy of them
int xfh_debug_eg_solve(xfh_ctx* c, int n, double* S, const double* b, double* x, int* solved) {
    if (!c || n < 1 || n > 7 * XFH_EG_MAX_FREE_V || !S || !b || !x || !solved) return XFH_ERR_INVALID_ARG;
    const size_t N = (size_t)n;
    int flag = 1;
    HostStage s{c};
    auto dS = s.add<double>(N * N * 8, S, S, false); auto db = s.in<double>(b, N * 8); auto dx = s.add<double>(N * 8, x, x, false);
    auto dk = s.add<int>(4, &flag, solved, false);
    if (const int rc = s.upload(); rc != XFH_OK) return rc;
    HIPCK(c, launch_eg_solve_alone(c, dS, db, dx, dk, n));
    return s.download();
}

}  // extern "C"
