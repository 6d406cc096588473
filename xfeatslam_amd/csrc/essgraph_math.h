// essgraph_math.h -- the arithmetic of Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:1532-1779: the Sim3 vertices, the EdgeSim3 pose graph,
// optimize(20) of OptimizationAlgorithmLevenberg over BlockSolver_7_3 with setUserLambdaInit(1e-16), the recovered poses and the corrected points), written
// ONCE for the kernels of essgraph.hip.h, the host form xfh_essential_graph_host and the piece entry points of capi_essgraph.cpp.  The Sim3 state with
// its exponential, product, inverse and oplus is optsim3_math.h's; here are Sim3::log (sim3.h:148-229), the EdgeSim3 error with g2o's numeric Jacobians, an
// edge's share of the blocks of H and b, the steps of the schedule as functions of one work item (one vertex, one edge, one lane of a fold), the Levenberg
// decisions for a system that is no small struct (EgCtl, beside lba_lm_after_trial) and the dense LDL^T in its column form.  The 256-lane fold and
// lba_ldlt_solve_host are lba_math.h's.  IEEE double throughout, every product and sum in the order written; tests/ref_essential_graph.py restates these lines.
#pragma once
#include "lba_math.h"
#include "optsim3_math.h"

#define XFH_EG_MAX_FREE_V 192             /* H is at most 1344 x 1344: the largest system the device solver has been run on */
#define XFH_EG_ITERATIONS_MAX 20          /* optimize(20) */
#define XFH_EG_HDR_INTS 9
#define XFH_EG_THREADS 256
#define XFH_EG_TILE 64                    /* the tile of the blocked LDL^T */
#define XFH_EG_REC 106                    /* doubles per edge: error [7], chi2, Ji [7][7], Jj [7][7] (row-major, a fixed vertex's zero) */
#define XFH_EG_NSUM 36                    /* 28 upper entries of a diagonal block (row-major, r <= c), 7 of b, the vertex's share of chi2 */
#define XFH_EG_SIMS 29                    /* per vertex: pert [14], their inverses [14], the inverse of the estimate */
#define XFH_EG_MAX_V 65535
#define XFH_EG_MAX_POINTS (1 << 22)
#define XFH_EG_MAX_EDGES (1 << 20)
#define XFH_EG_MAX_SIM3 (1 << 17)
#define XFH_EG_LAMBDA_INIT 1e-16          /* setUserLambdaInit(1e-16) */
enum { EG_OK = 0, EG_NOTHING_FREE = 1, EG_FREE_MISMATCH = 2, EG_NO_EDGES = 3 };
enum { EG_H_STATUS = 0, EG_H_FREE = 1, EG_H_EDGES = 2, EG_H_LOOP = 3, EG_H_ITERATIONS = 4, EG_H_TRIALS = 5, EG_H_REJECTED = 6, EG_H_LDLT_FAILURES = 7,
       EG_H_POINTS = 8 };
enum { EG_BUILD = 0, EG_TRIAL = 1, EG_DONE = 2 };

// the control record in device memory: every kernel of a step reads it first, the host reads it back after every trial.  cur: which of the two estimate
// buffers holds the estimate (a trial writes the other one, an accepted trial flips cur).  solved: 1 from the start of a trial's factorisation until a
// pivot fails.
struct EgCtl {
    double lambda, ni, currentChi, iniChi;
    int act, iter, qmax, nbad_lm, solved, cur, max_it, n_points;
    int hdr[XFH_EG_HDR_INTS];
    int reserved;
};

struct EgArgs {
    int nV, nP, nE, nS, n_free, pose_rows, point_rows, max_it, write_back, fix_scale;
    float* pose_table; float* point_table;
    const int* kf_row; const unsigned char* kf_fixed; const int* corrected_index; const int* noncorrected_index; const double* sim3;
    const int* edge_i; const int* edge_j; const int* edge_kind; const int* point_row; const int* point_ref;
    double* Sim3_out; float* Tcw_out; float* points_out; float* chi2; int* header; double* final_chi2;
    char* ws;
};

// ---- the workspace: every array on a 256-byte boundary, in this order; S last -----------------------------------------------------------------------
struct EgWs {
    EgCtl* ctl;
    int *v_free, *free_v, *v_cnt, *v_lead, *v_loop, *v_begin, *v_edges, *edge_ok;
    double *vScw, *Smw, *est, *sims, *meas, *rec, *v_sum, *v_chi, *b, *x, *S;
    size_t bytes;
};
XFH_HD EgWs eg_ws(char* base, int nV, int nE, int n_free) {
    EgWs w;
    size_t o = 0;
    const size_t V = (size_t)nV, E = (size_t)nE, n = (size_t)7 * (size_t)(n_free < 1 ? 1 : n_free);
#define EG_WS_TAKE(field, type, count) w.field = base ? (type*)(base + o) : nullptr; o += lba_al(sizeof(type) * (count))     /* (base NULL: the size alone) */
    EG_WS_TAKE(ctl, EgCtl, 1);
    EG_WS_TAKE(v_free, int, V); EG_WS_TAKE(free_v, int, XFH_EG_MAX_FREE_V); EG_WS_TAKE(v_cnt, int, V); EG_WS_TAKE(v_lead, int, V);
    EG_WS_TAKE(v_loop, int, V); EG_WS_TAKE(v_begin, int, V + 1);
    EG_WS_TAKE(v_edges, int, 2 * E); EG_WS_TAKE(edge_ok, int, E);
    EG_WS_TAKE(vScw, double, 8 * V); EG_WS_TAKE(Smw, double, 8 * V); EG_WS_TAKE(est, double, 2 * 8 * V); EG_WS_TAKE(sims, double, XFH_EG_SIMS * 8 * V);
    EG_WS_TAKE(meas, double, 8 * E); EG_WS_TAKE(rec, double, XFH_EG_REC * E); EG_WS_TAKE(v_sum, double, XFH_EG_NSUM * V); EG_WS_TAKE(v_chi, double, V);
    EG_WS_TAKE(b, double, n); EG_WS_TAKE(x, double, n); EG_WS_TAKE(S, double, n * n);
#undef EG_WS_TAKE
    w.bytes = o;
    return w;
}
XFH_HD Os3Sim eg_sim_get(const double* p) { return Os3Sim{{p[0], p[1], p[2], p[3]}, {p[4], p[5], p[6]}, p[7]}; }
XFH_HD void eg_sim_put(const Os3Sim& S, double* p) { p[0] = S.q[0]; p[1] = S.q[1]; p[2] = S.q[2]; p[3] = S.q[3]; p[4] = S.t[0]; p[5] = S.t[1]; p[6] = S.t[2]; p[7] = S.s; }

// ---- Sim3::log (sim3.h:148-229), branch for branch ------------------------------------------------------------------------------------------------------
// W.lu().solve(t): partial-pivot LU of a 3 x 3 in a fixed order.  Column k: the row r >= k with the largest |M[r][k]| (a later row only when strictly
// larger; a NaN never wins), swapped up; the rows below divided by the pivot and reduced.  Then the unit-lower forward and the upper backward substitution.
XFH_HD void eg_lu3_solve(double* M, double* t, double* x) {
    _Pragma("unroll")
    for (int k = 0; k < 3; ++k) {
        int p = k;
        _Pragma("unroll")
        for (int r = k + 1; r < 3; ++r) if (fabs(M[3 * r + k]) > fabs(M[3 * p + k])) p = r;
        _Pragma("unroll")
        for (int r = k + 1; r < 3; ++r)
            if (p == r) {
                _Pragma("unroll")
                for (int c = 0; c < 3; ++c) { const double s = M[3 * k + c]; M[3 * k + c] = M[3 * r + c]; M[3 * r + c] = s; }
                const double s = t[k]; t[k] = t[r]; t[r] = s;
            }
        _Pragma("unroll")
        for (int r = k + 1; r < 3; ++r) {
            M[3 * r + k] = M[3 * r + k] / M[3 * k + k];
            _Pragma("unroll")
            for (int c = k + 1; c < 3; ++c) M[3 * r + c] = M[3 * r + c] - M[3 * r + k] * M[3 * k + c];
        }
    }
    const double y0 = t[0], y1 = t[1] - M[3] * y0, y2 = (t[2] - M[6] * y0) - M[7] * y1;
    x[2] = y2 / M[8];
    x[1] = (y1 - M[5] * x[2]) / M[4];
    x[0] = ((y0 - M[1] * x[1]) - M[2] * x[2]) / M[0];
}
XFH_HD void eg_sim3_log(const Os3Sim& S, double* res) {
    const double s = S.s, sigma = log(s), eps = 0.00001;
    double R[9];
    pose_matrix_from_quat(S.q, R);
    const double d = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};            // deltaR
    double om[3], A, B, C;
    const bool near = d > 1.0 - eps;
    double theta = 0.0;
    if (near) { om[0] = 0.5 * dR[0]; om[1] = 0.5 * dR[1]; om[2] = 0.5 * dR[2]; }
    else {
        theta = acos(d);
        const double f = theta / (2.0 * sqrt(1.0 - d * d));
        om[0] = f * dR[0]; om[1] = f * dR[1]; om[2] = f * dR[2];
    }
    if (fabs(sigma) < eps) {
        C = 1.0;
        if (near) { A = 1.0 / 2.0; B = 1.0 / 6.0; }
        else {
            const double theta2 = theta * theta;
            A = (1.0 - cos(theta)) / theta2;
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (s - 1.0) / sigma;
        if (near) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1.0) * s + 1.0) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1.0) * s) / (sigma2 * sigma);
        } else {
            const double theta2 = theta * theta, a = s * sin(theta), b = s * cos(theta), c = theta2 + sigma * sigma;
            A = (a * sigma + (1.0 - b) * theta) / (theta * c);
            B = (C - ((b - 1.0) * sigma + a * theta) / c) * 1.0 / theta2;
        }
    }
    const double O[9] = {0.0, -om[2], om[1], om[2], 0.0, -om[0], -om[1], om[0], 0.0};
    double O2[9], W[9];
    _Pragma("unroll")
    for (int r = 0; r < 3; ++r)
        _Pragma("unroll")
        for (int c = 0; c < 3; ++c) O2[3 * r + c] = (O[3 * r] * O[c] + O[3 * r + 1] * O[3 + c]) + O[3 * r + 2] * O[6 + c];
    _Pragma("unroll")
    for (int k = 0; k < 9; ++k) W[k] = (A * O[k] + B * O2[k]) + C * (k % 4 == 0 ? 1.0 : 0.0);
    double t[3] = {S.t[0], S.t[1], S.t[2]}, up[3];
    eg_lu3_solve(W, t, up);
    res[0] = om[0]; res[1] = om[1]; res[2] = om[2]; res[3] = up[0]; res[4] = up[1]; res[5] = up[2]; res[6] = sigma;
}

// ---- EdgeSim3 (types_seven_dof_expmap.h:106-114) ----------------------------------------------------------------------------------------------------------
// computeError with the product C * v1 already formed: error = ((C * v1) * v2^-1).log(); chi2 = e . e, the terms added in index order
XFH_HD double eg_edge_error(const Os3Sim& CSi, const Os3Sim& Sj_inv, double* e) {
    Os3Sim T;
    os3_mul(CSi, Sj_inv, &T);
    eg_sim3_log(T, e);
    return (((((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) + e[3] * e[3]) + e[4] * e[4]) + e[5] * e[5]) + e[6] * e[6];
}
// one column pair of the numeric linearizeOplus (base_binary_edge.hpp:130-205): column d of J [7][7] row-major = (e(+) - e(-)) * (1 / (2 delta))
XFH_HD void eg_jacobian_column(const double* ep, const double* em, int d, double* J) {
    const double scalar = 1.0 / (2 * XFH_OS3_DELTA);
    _Pragma("unroll")
    for (int r = 0; r < 7; ++r) J[7 * r + d] = scalar * (ep[r] - em[r]);
}
// the whole edge at (Si, Sj) with measurement C: error, chi2 and, where wanted, the two Jacobians.  free_i / free_j: a fixed vertex has no Jacobian (zeros).
// perti / pinvj: the 14 perturbed estimates of vertex i and the inverses of the 14 perturbed estimates of vertex j (os3_sims_piece's pieces).
XFH_HD double eg_edge_linearize(const Os3Sim& C, const Os3Sim& Si, const Os3Sim& Sj_inv, const double* perti, const double* pinvj, bool free_i, bool free_j,
                                double* e, double* Ji, double* Jj) {
    Os3Sim CSi;
    os3_mul(C, Si, &CSi);
    const double chi2 = eg_edge_error(CSi, Sj_inv, e);
    _Pragma("clang loop unroll(disable)")
    for (int d = 0; d < 7; ++d) {
        double ep[7], em[7];
        if (free_i) {
            Os3Sim T;
            os3_mul(C, eg_sim_get(perti + 8 * (2 * d)), &T); eg_edge_error(T, Sj_inv, ep);
            os3_mul(C, eg_sim_get(perti + 8 * (2 * d + 1)), &T); eg_edge_error(T, Sj_inv, em);
            eg_jacobian_column(ep, em, d, Ji);
        } else for (int r = 0; r < 7; ++r) Ji[7 * r + d] = 0.0;
        if (free_j) {
            eg_edge_error(CSi, eg_sim_get(pinvj + 8 * (2 * d)), ep);
            eg_edge_error(CSi, eg_sim_get(pinvj + 8 * (2 * d + 1)), em);
            eg_jacobian_column(ep, em, d, Jj);
        } else for (int r = 0; r < 7; ++r) Jj[7 * r + d] = 0.0;
    }
    return chi2;
}
// constructQuadraticForm with the identity information, one vertex's side: acc[0 .. 27] += J^T J (upper, row-major), acc[28 .. 34] -= J^T e; every entry
// is summed over the 7 rows first, in row order
XFH_HD void eg_accumulate(double* acc, const double* J, const double* e) {
    int n = 0;
    _Pragma("unroll")
    for (int a = 0; a < 7; ++a)
        _Pragma("unroll")
        for (int b = a; b < 7; ++b, ++n) {
            double c = J[a] * J[b];
            _Pragma("unroll")
            for (int r = 1; r < 7; ++r) c = c + J[7 * r + a] * J[7 * r + b];
            acc[n] += c;
        }
    _Pragma("unroll")
    for (int a = 0; a < 7; ++a) {
        double c = J[a] * e[0];
        _Pragma("unroll")
        for (int r = 1; r < 7; ++r) c = c + J[7 * r + a] * e[r];
        acc[28 + a] -= c;
    }
}

// ---- the plan ---------------------------------------------------------------------------------------------------------------------------------------
XFH_HD bool eg_vertex_row_ok(const EgArgs& a, int v) { return lba_row_ok(a.kf_row[v], a.pose_rows); }
// vScw and Smw of vertex v (:1551-1554, :1616-1637) and the estimate in both buffers
XFH_HD void eg_vertex_init(const EgArgs& a, const EgWs& w, int v) {
    Os3Sim S{{0.0, 0.0, 0.0, 1.0}, {0.0, 0.0, 0.0}, 1.0};
    const int ci = a.corrected_index[v], ni = a.noncorrected_index[v];
    if (ci >= 0 && ci < a.nS) S = eg_sim_get(a.sim3 + 8 * (size_t)ci);
    else if (eg_vertex_row_ok(a, v)) {
        const float* T = a.pose_table + 12 * (size_t)a.kf_row[v];
        pose_quat_from_entries((double)T[0], (double)T[1], (double)T[2], (double)T[4], (double)T[5], (double)T[6], (double)T[8], (double)T[9], (double)T[10], S.q);
        S.t[0] = (double)T[3]; S.t[1] = (double)T[7]; S.t[2] = (double)T[11]; S.s = 1.0;
    }
    Os3Sim M = S;
    if (ni >= 0 && ni < a.nS) M = eg_sim_get(a.sim3 + 8 * (size_t)ni);
    eg_sim_put(S, w.vScw + 8 * (size_t)v); eg_sim_put(M, w.Smw + 8 * (size_t)v);
    eg_sim_put(S, w.est + 8 * (size_t)v); eg_sim_put(S, w.est + 8 * ((size_t)a.nV + v));
}
// an edge is an edge iff both indices are inside [0, nV), they differ and both vertices name a row of the pose table
XFH_HD int eg_edge_plan(const EgArgs& a, int e) {
    const int i = a.edge_i[e], j = a.edge_j[e];
    if (i < 0 || i >= a.nV || j < 0 || j >= a.nV || i == j) return 0;
    return (eg_vertex_row_ok(a, i) && eg_vertex_row_ok(a, j)) ? 1 : 0;
}
// the measurement: Sjw * Swi, of vScw for a loop connection (kind 0), of Smw for every other kind
XFH_HD void eg_edge_meas(const EgArgs& a, const EgWs& w, int e) {
    Os3Sim C{{0.0, 0.0, 0.0, 1.0}, {0.0, 0.0, 0.0}, 1.0};
    if (w.edge_ok[e]) {
        const double* tab = a.edge_kind[e] == 0 ? w.vScw : w.Smw;
        Os3Sim Swi;
        os3_inverse(eg_sim_get(tab + 8 * (size_t)a.edge_i[e]), &Swi);
        os3_mul(eg_sim_get(tab + 8 * (size_t)a.edge_j[e]), Swi, &C);
    }
    eg_sim_put(C, w.meas + 8 * (size_t)e);
    double* rec = w.rec + (size_t)XFH_EG_REC * e;
    for (int n = 0; n < 8; ++n) rec[n] = 0.0;
}
XFH_HD bool eg_incident(const EgArgs& a, const EgWs& w, int e, int v) { return w.edge_ok[e] && (a.edge_i[e] == v || a.edge_j[e] == v); }
// what edge e adds to vertex v's counts: bit 0 it is incident, bit 1 v is its vertex 0, bit 2 v is its vertex 0 and it is a loop connection
XFH_HD int eg_count_bits(const EgArgs& a, const EgWs& w, int e, int v) {
    if (!eg_incident(a, w, e, v)) return 0;
    return 1 | (a.edge_i[e] == v ? 2 : 0) | ((a.edge_i[e] == v && a.edge_kind[e] == 0) ? 4 : 0);
}
// after the per-vertex counts: free indices in vertex order, the vertex-major offsets, the header's counts and the early statuses.  One thread.
XFH_HD void eg_plan_scan(const EgArgs& a, const EgWs& w) {
    EgCtl& c = *w.ctl;
    int nf = 0, off = 0, edges = 0, loop = 0;
    for (int v = 0; v < a.nV; ++v) {
        const bool fixed = a.kf_fixed[v] != 0;
        w.v_free[v] = -1;
        if (!fixed) { if (nf < XFH_EG_MAX_FREE_V && nf < a.n_free) { w.v_free[v] = nf; w.free_v[nf] = v; } ++nf; }
        w.v_begin[v] = off; off += w.v_cnt[v];
        edges += w.v_lead[v]; loop += w.v_loop[v];
    }
    w.v_begin[a.nV] = off;
    c.lambda = 0.0; c.ni = 2.0; c.currentChi = 0.0; c.iniChi = 0.0;
    c.iter = 0; c.qmax = 0; c.nbad_lm = 0; c.solved = 0; c.cur = 0; c.max_it = a.max_it; c.n_points = 0; c.reserved = 0;
    for (int k = 0; k < XFH_EG_HDR_INTS; ++k) c.hdr[k] = 0;
    c.hdr[EG_H_FREE] = nf; c.hdr[EG_H_EDGES] = edges; c.hdr[EG_H_LOOP] = loop;
    int st = EG_OK;
    if (nf != a.n_free) st = EG_FREE_MISMATCH;
    else if (nf == 0) st = EG_NOTHING_FREE;
    else if (edges == 0) st = EG_NO_EDGES;
    c.hdr[EG_H_STATUS] = st;
    c.act = st == EG_OK ? EG_BUILD : EG_DONE;
    for (int j = 0; j < 7 * a.n_free; ++j) w.x[j] = 0.0;                     // the solver's x: a failed factorisation leaves the previous solve's there
}

// ---- the steps, one work item's share each ----------------------------------------------------------------------------------------------------------------
// piece j of vertex v's similarities at the estimate in buffer `buf`: j < 14 the perturbed estimate and its inverse (free vertices only), 14 the inverse
XFH_HD void eg_sims_piece(const EgArgs& a, const EgWs& w, int v, int j, int buf) {
    const Os3Sim est = eg_sim_get(w.est + 8 * ((size_t)buf * a.nV + v));
    double* out = w.sims + (size_t)XFH_EG_SIMS * 8 * v;
    Os3Sim p, pi;
    if (j == 14) { os3_inverse(est, &pi); eg_sim_put(pi, out + 8 * 28); return; }
    if (w.v_free[v] < 0) return;
    const int d = j >> 1;
    const double dv = (j & 1) ? -XFH_OS3_DELTA : XFH_OS3_DELTA;
    double u[7];
    _Pragma("unroll")
    for (int k = 0; k < 7; ++k) u[k] = k == d ? dv : 0.0;
    os3_oplus(u, est, a.fix_scale, &p);
    os3_inverse(p, &pi);
    eg_sim_put(p, out + 8 * j); eg_sim_put(pi, out + 8 * (14 + j));
}
// LINEARIZE / EVALUATE, edge e at the estimate in buffer `buf` (whose similarities eg_sims_piece left): the record
XFH_HD void eg_edge_step(const EgArgs& a, const EgWs& w, int e, int buf, bool build) {
    if (!w.edge_ok[e]) return;
    const int i = a.edge_i[e], j = a.edge_j[e];
    double* rec = w.rec + (size_t)XFH_EG_REC * e;
    const Os3Sim C = eg_sim_get(w.meas + 8 * (size_t)e), Si = eg_sim_get(w.est + 8 * ((size_t)buf * a.nV + i));
    const double* sj = w.sims + (size_t)XFH_EG_SIMS * 8 * j;
    const Os3Sim Sj_inv = eg_sim_get(sj + 8 * 28);
    double er[7];
    if (build) {
        rec[7] = eg_edge_linearize(C, Si, Sj_inv, w.sims + (size_t)XFH_EG_SIMS * 8 * i, sj + 8 * 14, w.v_free[i] >= 0, w.v_free[j] >= 0, er, rec + 8, rec + 57);
    } else {
        Os3Sim CSi;
        os3_mul(C, Si, &CSi);
        rec[7] = eg_edge_error(CSi, Sj_inv, er);
    }
    for (int r = 0; r < 7; ++r) rec[r] = er[r];
}
// vertex v, lane l: its incident edges l, l + 256, ... of the vertex-major list.  build: a free vertex's share of its diagonal block and b
// (acc[0 .. 34]); always its share of chi2 (acc[35]): the edges whose vertex 0 it is.
XFH_HD void eg_vertex_lane(const EgArgs& a, const EgWs& w, int v, int lane, bool build, double* acc) {
    const bool free_v = w.v_free[v] >= 0;
    const int b = w.v_begin[v], n = w.v_cnt[v];
    for (int t = lane; t < n; t += XFH_EG_THREADS) {
        const int e = w.v_edges[b + t];
        const double* rec = w.rec + (size_t)XFH_EG_REC * e;
        const bool first = a.edge_i[e] == v;
        if (build && free_v) eg_accumulate(acc, rec + (first ? 8 : 57), rec);
        if (first) acc[35] += rec[7];
    }
}
// the diagonal block of free vertex f with lambda, and its b: the lower triangle of S (row stride n = 7 n_free)
XFH_HD void eg_diag_store(const EgArgs& a, const EgWs& w, int f) {
    const size_t n = (size_t)7 * a.n_free;
    const double* Hs = w.v_sum + (size_t)XFH_EG_NSUM * w.free_v[f];
    const double lambda = w.ctl->lambda;
    int m = 0;
    for (int r = 0; r < 7; ++r)
        for (int c = r; c < 7; ++c, ++m) w.S[(7 * (size_t)f + c) * n + 7 * (size_t)f + r] = (r == c) ? Hs[m] + lambda : Hs[m];
    for (int r = 0; r < 7; ++r) w.b[7 * (size_t)f + r] = Hs[28 + r];
}
// the off-diagonal block of the pair of free vertices that edge e joins, when e is the FIRST edge of that pair: J_lo^T J_hi summed over the pair's edges in
// edge order (lo: the vertex that comes first in vertex order), each entry of an edge's term summed over the 7 rows first
XFH_HD void eg_pair_store(const EgArgs& a, const EgWs& w, int e) {
    if (!w.edge_ok[e]) return;
    const int i = a.edge_i[e], j = a.edge_j[e], lo = i < j ? i : j, hi = i < j ? j : i;
    const int flo = w.v_free[lo], fhi = w.v_free[hi];
    if (flo < 0 || fhi < 0) return;
    const size_t n = (size_t)7 * a.n_free;
    double blk[49];
    for (int k = 0; k < 49; ++k) blk[k] = 0.0;
    const int b = w.v_begin[lo], cnt = w.v_cnt[lo];
    bool seen = false;
    for (int t = 0; t < cnt; ++t) {
        const int f = w.v_edges[b + t];
        const int fi = a.edge_i[f], fj = a.edge_j[f];
        if (!((fi == lo && fj == hi) || (fi == hi && fj == lo))) continue;
        if (!seen && f != e) return;                                        // an earlier edge of the pair does the sum
        seen = true;
        const double* rec = w.rec + (size_t)XFH_EG_REC * f;
        const double *Jl = rec + (fi == lo ? 8 : 57), *Jh = rec + (fi == lo ? 57 : 8);
        for (int r = 0; r < 7; ++r)
            for (int c = 0; c < 7; ++c) {
                double s = Jl[r] * Jh[c];
                for (int k = 1; k < 7; ++k) s = s + Jl[7 * k + r] * Jh[7 * k + c];
                blk[7 * r + c] += s;
            }
    }
    for (int r = 0; r < 7; ++r)
        for (int c = 0; c < 7; ++c) w.S[(7 * (size_t)fhi + c) * n + 7 * (size_t)flo + r] = blk[7 * r + c];
}
// the term j of computeScale, j = 0 .. 7 n_free - 1
XFH_HD double eg_scale_term(const EgWs& w, int j) { const double x = w.x[j]; return x * (w.ctl->lambda * x + w.b[j]); }
// UPDATE: oplusImpl of free vertex v into the other buffer
XFH_HD void eg_vertex_update(const EgArgs& a, const EgWs& w, int v) {
    const int f = w.v_free[v];
    if (f < 0) return;
    const int cur = w.ctl->cur;
    Os3Sim n;
    os3_oplus(w.x + 7 * (size_t)f, eg_sim_get(w.est + 8 * ((size_t)cur * a.nV + v)), a.fix_scale, &n);
    eg_sim_put(n, w.est + 8 * ((size_t)(1 - cur) * a.nV + v));
}

// ---- the Levenberg decisions (optimization_algorithm_levenberg.cpp:61-194) with the sums handed in, as lba_lm_after_build / lba_lm_after_trial ------------
XFH_HD void eg_lm_after_build(EgCtl& S, double chi) {
    S.currentChi = chi; S.iniChi = chi;
    if (S.iter == 0) { S.lambda = XFH_EG_LAMBDA_INIT; S.ni = 2.0; S.nbad_lm = 0; }   // computeLambdaInit: the user value
    S.qmax = 0;
    ++S.hdr[EG_H_ITERATIONS];
    S.act = EG_TRIAL;
}
XFH_HD void eg_lm_after_trial(EgCtl& S, double chi, double scale) {
    ++S.hdr[EG_H_TRIALS];
    if (!S.solved) ++S.hdr[EG_H_LDLT_FAILURES];
    const double tempChi = S.solved ? chi : DBL_MAX;
    double rho = S.currentChi - tempChi;
    scale += 1e-3;
    rho /= scale;
    if (rho > 0.0 && isfinite(tempChi)) {
        const double t = 2.0 * rho - 1.0;
        double alpha = 1.0 - t * t * t;
        alpha = (2.0 / 3.0 < alpha) ? 2.0 / 3.0 : alpha;
        const double f = (1.0 / 3.0 < alpha) ? alpha : 1.0 / 3.0;
        S.lambda *= f; S.ni = 2.0; S.currentChi = tempChi;
        S.cur = 1 - S.cur;
    } else {
        S.lambda *= S.ni; S.ni *= 2.0;
        ++S.hdr[EG_H_REJECTED];
    }
    ++S.qmax;
    if (rho < 0.0 && S.qmax < GEO_LM_MAX_TRIALS) { S.act = EG_TRIAL; return; }
    if (S.qmax == GEO_LM_MAX_TRIALS || rho == 0.0) { S.act = EG_DONE; return; }
    if ((S.iniChi - S.currentChi) * 1e3 < S.iniChi) ++S.nbad_lm; else S.nbad_lm = 0;
    if (S.nbad_lm >= 3) { S.act = EG_DONE; return; }
    S.act = ++S.iter < S.max_it ? EG_BUILD : EG_DONE;
}

// ---- the outputs ------------------------------------------------------------------------------------------------------------------------------------
// Sim3_out and Tcw_out = [R | t / s], R of the normalised quaternion, rounded once (:1736-1749)
XFH_HD void eg_finish_vertex(const EgArgs& a, const EgWs& w, int v) {
    const Os3Sim E = eg_sim_get(w.est + 8 * ((size_t)w.ctl->cur * a.nV + v));
    eg_sim_put(E, a.Sim3_out + 8 * (size_t)v);
    const double nq = sqrt(((E.q[0] * E.q[0] + E.q[1] * E.q[1]) + E.q[2] * E.q[2]) + E.q[3] * E.q[3]);
    const double q[4] = {E.q[0] / nq, E.q[1] / nq, E.q[2] / nq, E.q[3] / nq};
    double R[9];
    pose_matrix_from_quat(q, R);
    float* out = a.Tcw_out + 12 * (size_t)v;
    for (int r = 0; r < 3; ++r) { out[4 * r] = (float)R[3 * r]; out[4 * r + 1] = (float)R[3 * r + 1]; out[4 * r + 2] = (float)R[3 * r + 2]; out[4 * r + 3] = (float)(E.t[r] / E.s); }
    if (a.write_back && w.ctl->hdr[EG_H_STATUS] != EG_FREE_MISMATCH && eg_vertex_row_ok(a, v))
        for (int n = 0; n < 12; ++n) a.pose_table[12 * (size_t)a.kf_row[v] + n] = out[n];
}
// correctedSwr.map(Srw.map(P)) (:1771-1776); returns 1 for a corrected point
XFH_HD int eg_finish_point(const EgArgs& a, const EgWs& w, int p) {
    const int row = a.point_row[p], ref = a.point_ref[p];
    float* out = a.points_out + 3 * (size_t)p;
    if (!lba_row_ok(row, a.point_rows)) { out[0] = 0.0f; out[1] = 0.0f; out[2] = 0.0f; return 0; }
    const float* X = a.point_table + 3 * (size_t)row;
    if (ref < 0 || ref >= a.nV) { out[0] = X[0]; out[1] = X[1]; out[2] = X[2]; return 0; }
    const double P[3] = {(double)X[0], (double)X[1], (double)X[2]};
    double c[3], o[3];
    Os3Sim Swr;
    os3_inverse(eg_sim_get(w.est + 8 * ((size_t)w.ctl->cur * a.nV + ref)), &Swr);
    os3_map(eg_sim_get(w.vScw + 8 * (size_t)ref), P, c);
    os3_map(Swr, c, o);
    out[0] = (float)o[0]; out[1] = (float)o[1]; out[2] = (float)o[2];
    if (a.write_back && w.ctl->hdr[EG_H_STATUS] != EG_FREE_MISMATCH)
        for (int n = 0; n < 3; ++n) a.point_table[3 * (size_t)row + n] = out[n];
    return 1;
}
// chi2 of the error the last computeActiveErrors left (the stale-error rule); 0 for an edge that is no edge and for a call without an iteration
XFH_HD void eg_finish_edge(const EgArgs& a, const EgWs& w, int e) {
    a.chi2[e] = (w.edge_ok[e] && w.ctl->hdr[EG_H_ITERATIONS] > 0) ? (float)w.rec[(size_t)XFH_EG_REC * e + 7] : 0.0f;
}
XFH_HD void eg_finish_header(const EgArgs& a, const EgWs& w) {
    for (int k = 0; k < XFH_EG_HDR_INTS; ++k) a.header[k] = w.ctl->hdr[k];
    a.header[EG_H_POINTS] = w.ctl->n_points;
    *a.final_chi2 = w.ctl->currentChi;
}

// ---- the whole rule on ONE host thread: the kernels' steps in the order the device call launches them, every fold as the 256 lanes make it -----------------
inline void eg_host_vertex_pass(const EgArgs& a, const EgWs& w, bool build) {
    static thread_local double part[XFH_EG_THREADS][XFH_EG_NSUM];
    for (int v = 0; v < a.nV; ++v) {
        for (int l = 0; l < XFH_EG_THREADS; ++l) {
            for (int n = 0; n < XFH_EG_NSUM; ++n) part[l][n] = 0.0;
            eg_vertex_lane(a, w, v, l, build, part[l]);
        }
        if (build) for (int n = 0; n < XFH_EG_NSUM; ++n) w.v_sum[(size_t)XFH_EG_NSUM * v + n] = lba_host_fold(&part[0][n], XFH_EG_NSUM);
        else w.v_chi[v] = lba_host_fold(&part[0][35], XFH_EG_NSUM);
    }
}
inline void eg_host_run(const EgArgs& a) {
    const EgWs w = eg_ws(a.ws, a.nV, a.nE, a.n_free);
    EgCtl& c = *w.ctl;
    for (int v = 0; v < a.nV; ++v) eg_vertex_init(a, w, v);
    for (int e = 0; e < a.nE; ++e) { w.edge_ok[e] = eg_edge_plan(a, e); eg_edge_meas(a, w, e); }
    for (int v = 0; v < a.nV; ++v) {
        int n = 0, n0 = 0, l0 = 0;
        for (int e = 0; e < a.nE; ++e) { const int bits = eg_count_bits(a, w, e, v); n += bits & 1; n0 += (bits >> 1) & 1; l0 += (bits >> 2) & 1; }
        w.v_cnt[v] = n; w.v_lead[v] = n0; w.v_loop[v] = l0;
    }
    eg_plan_scan(a, w);
    for (int v = 0; v < a.nV; ++v) { int n = w.v_begin[v]; for (int e = 0; e < a.nE; ++e) if (eg_incident(a, w, e, v)) w.v_edges[n++] = e; }
    const int n = 7 * a.n_free;
    const size_t N = (size_t)n;
    double* y = n > 0 ? new double[n] : nullptr;
    for (int step = 0; step < a.max_it * (GEO_LM_MAX_TRIALS + 1) && c.act != EG_DONE; ++step) {
        if (c.act == EG_BUILD) {
            for (int v = 0; v < a.nV; ++v) for (int j = 0; j < 15; ++j) eg_sims_piece(a, w, v, j, c.cur);
            for (int e = 0; e < a.nE; ++e) eg_edge_step(a, w, e, c.cur, true);
            eg_host_vertex_pass(a, w, true);
            eg_lm_after_build(c, lba_host_fold_terms(a.nV, [&](int v) { return w.v_sum[(size_t)XFH_EG_NSUM * v + 35]; }));
            continue;
        }
        for (size_t k = 0; k < N * N; ++k) w.S[k] = 0.0;
        for (int f = 0; f < a.n_free; ++f) eg_diag_store(a, w, f);
        for (int e = 0; e < a.nE; ++e) eg_pair_store(a, w, e);
        c.solved = lba_ldlt_solve_host(w.S, n, w.b, w.x, y) ? 1 : 0;
        for (int v = 0; v < a.nV; ++v) eg_vertex_update(a, w, v);
        for (int v = 0; v < a.nV; ++v) eg_sims_piece(a, w, v, 14, 1 - c.cur);
        for (int e = 0; e < a.nE; ++e) eg_edge_step(a, w, e, 1 - c.cur, false);
        eg_host_vertex_pass(a, w, false);
        const double chi = lba_host_fold_terms(a.nV, [&](int v) { return w.v_chi[v]; });
        const double scale = lba_host_fold_terms(n, [&](int j) { return eg_scale_term(w, j); });
        eg_lm_after_trial(c, chi, scale);
    }
    delete[] y;
    for (int v = 0; v < a.nV; ++v) eg_finish_vertex(a, w, v);
    for (int p = 0; p < a.nP; ++p) c.n_points += eg_finish_point(a, w, p);
    for (int e = 0; e < a.nE; ++e) eg_finish_edge(a, w, e);
    eg_finish_header(a, w);
}
