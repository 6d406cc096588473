// lba_math.h -- the arithmetic of Optimizer::LocalBundleAdjustment (src/Optimizer.cc:1188-1460: the graph, optimize(10) of OptimizationAlgorithmLevenberg over
// BlockSolver_6_3 with the Schur complement, the three loops that fill vToErase), written ONCE for the kernels of lba.hip.h, the host form
// xfh_local_ba_host and the piece entry points of capi_lba.cpp.  The SE3 state, pose_oplus, the edge error, the pose Jacobian, the Huber kernel and an edge's
// share of a pose block are poseopt_math.h's; here are what a binary edge adds (the point Jacobian, the cross block, the point block and its closed-form
// inverse), the steps of the distributed schedule as functions of one work item (one keyframe, one point, one pair of free keyframes, one lane of a fold)
// and the Levenberg decisions restated for a machine whose sums arrive from other kernels (LbaCtl; geo_lm_* of geom_common.h keeps the dense N x N form).
// IEEE double throughout, every product and sum in the order written; tests/ref_local_ba.py restates these lines.
#pragma once
#include "poseopt_math.h"

#define XFH_LBA_MAX_FREE_KF 128          /* S is at most 768 x 768 */
#define XFH_LBA_ITERATIONS_MAX 10         /* optimize(10): the schedule is laid out for at most this many */
#define XFH_LBA_HDR_INTS 10
#define XFH_LBA_THREADS 256
#define XFH_LBA_SOLVE_THREADS 1024
#define XFH_LBA_REC 28                    /* doubles per edge: Hll share [6], bl share [3], W [6][3], the chi2 of the last computeError */
#define XFH_LBA_MAX_KF 65535
#define XFH_LBA_MAX_POINTS (1 << 22)
#define XFH_LBA_MAX_EDGES (1 << 24)
enum { LBA_OK = 0, LBA_ABORTED = 1, LBA_NOTHING_FREE = 2, LBA_FREE_MISMATCH = 3 };
enum { LBA_H_STATUS = 0, LBA_H_FREE = 1, LBA_H_FIXED_EDGE = 2, LBA_H_MONO = 3, LBA_H_STEREO = 4, LBA_H_ITERATIONS = 5, LBA_H_TRIALS = 6, LBA_H_REJECTED = 7,
       LBA_H_LDLT_FAILURES = 8, LBA_H_ERASE = 9 };
enum { LBA_BUILD = 0, LBA_TRIAL = 1, LBA_DONE = 2 };

// the control block in device memory: every kernel of the schedule reads it first.  cur: which of the two estimate buffers holds the estimate; a
// trial writes the other one and an accepted trial flips cur, so push() / pop() copy nothing.
struct LbaCtl {
    double lambda, ni, currentChi, iniChi;
    int act, iter, qmax, nbad_lm, solved, cur, max_it, n_erase;
    int hdr[XFH_LBA_HDR_INTS];
};

struct LbaArgs {
    int nK, nP, nE, n_free, pose_rows, point_rows, max_it, write_back;
    float* pose_table; float* point_table;
    const int* kf_row; const unsigned char* kf_fixed; const int* point_row; const int* edge_begin; const int* edge_kf; const float* edge_obs;
    PoseCam cam; double w;
    float* Tcw_out; float* points_out; unsigned char* erase; float* chi2; int* header; double* final_chi2;
    char* ws;
};

// ---- the workspace: every array on a 256-byte boundary, in this order -----------------------------------------------------------------------------
struct LbaWs {
    LbaCtl* ctl;
    int *kf_free, *free_kf, *kf_cnt, *kf_mono, *kf_stereo, *kf_begin, *kf_edges, *edge_pt, *pt_edges;
    double *pose, *pt, *rec, *kf_sum, *kf_chi, *Hll, *bl, *xl, *pscale, *xp, *bS, *S;
    size_t bytes;
};
XFH_HD size_t lba_al(size_t x) { return (x + 255) & ~(size_t)255; }
XFH_HD LbaWs lba_ws(char* base, int nK, int nP, int nE, int n_free) {
    LbaWs w;
    size_t o = 0;
    const size_t K = (size_t)nK, P = (size_t)nP, E = (size_t)nE, n = (size_t)6 * (size_t)(n_free < 1 ? 1 : n_free);
#define LBA_WS_TAKE(field, type, count) w.field = base ? (type*)(base + o) : nullptr; o += lba_al(sizeof(type) * (count))     /* (base NULL: the size alone) */
    LBA_WS_TAKE(ctl, LbaCtl, 1);
    LBA_WS_TAKE(kf_free, int, K); LBA_WS_TAKE(free_kf, int, XFH_LBA_MAX_FREE_KF); LBA_WS_TAKE(kf_cnt, int, K); LBA_WS_TAKE(kf_mono, int, K);
    LBA_WS_TAKE(kf_stereo, int, K); LBA_WS_TAKE(kf_begin, int, K + 1); LBA_WS_TAKE(kf_edges, int, E); LBA_WS_TAKE(edge_pt, int, E); LBA_WS_TAKE(pt_edges, int, P);
    LBA_WS_TAKE(pose, double, 2 * 8 * K); LBA_WS_TAKE(pt, double, 2 * 3 * P); LBA_WS_TAKE(rec, double, XFH_LBA_REC * E); LBA_WS_TAKE(kf_sum, double, XFH_POSE_NSUM * K);
    LBA_WS_TAKE(kf_chi, double, K); LBA_WS_TAKE(Hll, double, 6 * P); LBA_WS_TAKE(bl, double, 3 * P); LBA_WS_TAKE(xl, double, 3 * P); LBA_WS_TAKE(pscale, double, P);
    LBA_WS_TAKE(xp, double, n); LBA_WS_TAKE(bS, double, n); LBA_WS_TAKE(S, double, n * n);
#undef LBA_WS_TAKE
    w.bytes = o;
    return w;
}
XFH_HD PosePose lba_pose_get(const double* p) { return PosePose{{p[0], p[1], p[2], p[3]}, {p[4], p[5], p[6]}}; }
XFH_HD void lba_pose_put(const PosePose& P, double* p) { p[0] = P.q[0]; p[1] = P.q[1]; p[2] = P.q[2]; p[3] = P.q[3]; p[4] = P.t[0]; p[5] = P.t[1]; p[6] = P.t[2]; p[7] = 0.0; }

// ---- the binary edge ------------------------------------------------------------------------------------------------------------------------------
// _jacobianOplusXi at the camera-frame point pc, R = the pose's rotation matrix (row-major): Jl [3][3] row-major, the third row zero for a mono edge.
// Mono (OptimizableTypes.cpp:139-152): -projectJac(pc) * R with the structural zeros of projectJac left out; stereo: types_six_dof_expmap.cpp:242-252.
XFH_HD void lba_point_jacobian(const PoseCam& cam, const double* R, const double* pc, bool stereo, double* Jl) {
    const double x = pc[0], y = pc[1], z = pc[2];
    if (!stereo) {
        const double a = cam.fx / z, c = -cam.fx * x / (z * z), b = cam.fy / z, d = -cam.fy * y / (z * z);
        _Pragma("unroll")
        for (int k = 0; k < 3; ++k) { Jl[k] = -(a * R[k] + c * R[6 + k]); Jl[3 + k] = -(b * R[3 + k] + d * R[6 + k]); Jl[6 + k] = 0.0; }
        return;
    }
    const double z_2 = z * z;
    _Pragma("unroll")
    for (int k = 0; k < 3; ++k) {
        Jl[k] = -cam.fx * R[k] / z + cam.fx * x * R[6 + k] / z_2;
        Jl[3 + k] = -cam.fy * R[3 + k] / z + cam.fy * y * R[6 + k] / z_2;
        Jl[6 + k] = Jl[k] - cam.bf * R[6 + k] / z_2;
    }
}
// one edge linearised at (P, X): error, chi2, rho, both Jacobians (computeError, robustify, linearizeOplus)
struct LbaLin { double e[3], chi2, rho0, rho1, Jp[18], Jl[9]; };
XFH_HD void lba_edge_linearize(const PosePose& P, const PoseCam& cam, const double* X, const double* obs, bool stereo, double w, LbaLin* L) {
    double pc[3], R[9];
    L->chi2 = pose_edge_error(P, cam, X, obs, stereo, w, pc, L->e);
    pose_huber(L->chi2, pose_delta(stereo), &L->rho0, &L->rho1);
    pose_edge_jacobian(cam, pc, stereo, L->Jp);
    pose_matrix_from_quat(P.q, R);
    lba_point_jacobian(cam, R, pc, stereo, L->Jl);
}
// constructQuadraticForm of a binary edge (base_binary_edge.hpp), the part that involves the point: rec[0..5] = Jl^T (rho1 w) Jl (upper, row-major),
// rec[6..8] = -rho1 Jl^T (w e), rec[9..26] = W = Jp^T (rho1 w) Jl as [6][3] (zero for a fixed keyframe: it has no pose block), rec[27] = chi2.
// Each entry is summed over the edge's rows first, as pose_accumulate does.
XFH_HD void lba_edge_record(const LbaLin& L, bool stereo, double w, bool free_kf, double* rec) {
    const double ww = L.rho1 * w;
    int n = 0;
    _Pragma("unroll")
    for (int a = 0; a < 3; ++a)
        _Pragma("unroll")
        for (int b = a; b < 3; ++b, ++n) {
            double c = L.Jl[a] * (ww * L.Jl[b]) + L.Jl[3 + a] * (ww * L.Jl[3 + b]);
            if (stereo) c = c + L.Jl[6 + a] * (ww * L.Jl[6 + b]);
            rec[n] = c;
        }
    _Pragma("unroll")
    for (int a = 0; a < 3; ++a) {
        double c = L.Jl[a] * (w * L.e[0]) + L.Jl[3 + a] * (w * L.e[1]);
        if (stereo) c = c + L.Jl[6 + a] * (w * L.e[2]);
        rec[6 + a] = -(L.rho1 * c);
    }
    _Pragma("unroll")
    for (int i = 0; i < 6; ++i)
        _Pragma("unroll")
        for (int a = 0; a < 3; ++a) {
            double c = L.Jp[i] * (ww * L.Jl[a]) + L.Jp[6 + i] * (ww * L.Jl[3 + a]);
            if (stereo) c = c + L.Jp[12 + i] * (ww * L.Jl[6 + a]);
            rec[9 + 3 * i + a] = free_kf ? c : 0.0;
        }
    rec[27] = L.chi2;
}

// (Hll + lambda I)^-1 of one point, closed form: Eigen's fixed-size 3 x 3 inverse is by cofactors (the determinant from the first column's), and a
// singular block makes what it makes.  H6 = the upper triangle row by row; D = the full 3 x 3 row-major.
XFH_HD void lba_point_block(const double* H6, double lambda, double* D) {
    const double m00 = H6[0] + lambda, m01 = H6[1], m02 = H6[2], m11 = H6[3] + lambda, m12 = H6[4], m22 = H6[5] + lambda;
    const double c00 = m11 * m22 - m12 * m12, c10 = m02 * m12 - m01 * m22, c20 = m01 * m12 - m02 * m11;
    const double det = (c00 * m00 + c10 * m01) + c20 * m02, inv = 1.0 / det;
    D[0] = c00 * inv; D[1] = c10 * inv; D[2] = c20 * inv;
    D[3] = D[1]; D[4] = (m00 * m22 - m02 * m02) * inv; D[5] = (m01 * m02 - m00 * m12) * inv;
    D[6] = D[2]; D[7] = D[5]; D[8] = (m00 * m11 - m01 * m01) * inv;
}

// ---- the plan ---------------------------------------------------------------------------------------------------------------------------------------
// the point an edge belongs to: the first p with edge_begin[p + 1] > e, provided edge_begin[p] <= e; -1 where the CSR names none.  A fixed number of
// steps whatever the array holds, and only edge_begin[0 .. nP] is read.
XFH_HD int lba_edge_point(const int* edge_begin, int nP, int e) {
    int lo = 0, hi = nP;
    for (int s = 0; s < 32; ++s) {
        if (lo >= hi) break;
        const int mid = lo + (hi - lo) / 2;
        if (edge_begin[mid + 1] > e) hi = mid; else lo = mid + 1;
    }
    return (lo < nP && edge_begin[lo] <= e) ? lo : -1;
}
XFH_HD bool lba_row_ok(int row, int rows) { return row >= 0 && row < rows; }
// an edge is an edge iff its keyframe index is inside [0, nK), the CSR names its point, and both name a row of their table
XFH_HD int lba_edge_plan(const LbaArgs& a, int e) {
    const int k = a.edge_kf[e];
    if (k < 0 || k >= a.nK || !lba_row_ok(a.kf_row[k], a.pose_rows)) return -1;
    const int p = lba_edge_point(a.edge_begin, a.nP, e);
    if (p < 0 || !lba_row_ok(a.point_row[p], a.point_rows)) return -1;
    return p;
}
XFH_HD bool lba_stereo(const LbaArgs& a, int e) { return !(a.edge_obs[3 * (size_t)e + 2] < 0.0f); }   // `mvuRight < 0` decides: a NaN is stereo
XFH_HD void lba_obs(const LbaArgs& a, int e, double* obs) {
    obs[0] = (double)a.edge_obs[3 * (size_t)e]; obs[1] = (double)a.edge_obs[3 * (size_t)e + 1]; obs[2] = (double)a.edge_obs[3 * (size_t)e + 2];
}
XFH_HD int lba_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// the edges of point p: [b, e) of the CSR clamped into [0, nE]; the caller skips an entry whose edge_pt is not p
XFH_HD void lba_point_range(const LbaArgs& a, int p, int* b, int* e) {
    *b = lba_clamp(a.edge_begin[p], 0, a.nE);
    *e = lba_clamp(a.edge_begin[p + 1], *b, a.nE);
}
XFH_HD void lba_point_init(const LbaArgs& a, const LbaWs& w, int p) {
    const int row = a.point_row[p];
    int n = 0, b, e;
    lba_point_range(a, p, &b, &e);
    for (int k = b; k < e; ++k) n += w.edge_pt[k] == p ? 1 : 0;
    w.pt_edges[p] = n;
    for (int c = 0; c < 3; ++c) {
        const double v = lba_row_ok(row, a.point_rows) ? (double)a.point_table[3 * (size_t)row + c] : 0.0;
        w.pt[3 * (size_t)p + c] = v; w.pt[3 * ((size_t)a.nP + p) + c] = v; w.xl[3 * (size_t)p + c] = 0.0;
    }
    w.pscale[p] = 0.0;
}
XFH_HD void lba_kf_init(const LbaArgs& a, const LbaWs& w, int k) {
    PosePose P{{0.0, 0.0, 0.0, 1.0}, {0.0, 0.0, 0.0}};
    if (lba_row_ok(a.kf_row[k], a.pose_rows)) pose_from_tcw(a.pose_table + 12 * (size_t)a.kf_row[k], &P);
    lba_pose_put(P, w.pose + 8 * (size_t)k); lba_pose_put(P, w.pose + 8 * ((size_t)a.nK + k));
}
// after the per-keyframe counts: free indices in keyframe order, the keyframe-major offsets, the header's counts and the early statuses.  One thread.
XFH_HD void lba_plan_scan(const LbaArgs& a, const LbaWs& w) {
    LbaCtl& c = *w.ctl;
    int nf = 0, fixed_edge = 0, mono = 0, stereo = 0, off = 0;
    for (int k = 0; k < a.nK; ++k) {
        const bool fixed = a.kf_fixed[k] != 0 || !lba_row_ok(a.kf_row[k], a.pose_rows);
        w.kf_free[k] = -1;
        if (!fixed) { if (nf < XFH_LBA_MAX_FREE_KF && nf < a.n_free) { w.kf_free[k] = nf; w.free_kf[nf] = k; } ++nf; }
        else if (w.kf_cnt[k] > 0) ++fixed_edge;
        mono += w.kf_mono[k]; stereo += w.kf_stereo[k];
        w.kf_begin[k] = off; off += w.kf_cnt[k];
    }
    w.kf_begin[a.nK] = off;
    c.lambda = 0.0; c.ni = 2.0; c.currentChi = 0.0; c.iniChi = 0.0;
    c.iter = 0; c.qmax = 0; c.nbad_lm = 0; c.solved = 0; c.cur = 0; c.max_it = a.max_it; c.n_erase = 0;
    for (int k = 0; k < XFH_LBA_HDR_INTS; ++k) c.hdr[k] = 0;
    c.hdr[LBA_H_FREE] = nf; c.hdr[LBA_H_FIXED_EDGE] = fixed_edge; c.hdr[LBA_H_MONO] = mono; c.hdr[LBA_H_STEREO] = stereo;
    int st = LBA_OK;
    if (nf != a.n_free) st = LBA_FREE_MISMATCH;
    else if (fixed_edge == 0) st = LBA_ABORTED;                             // `if (num_fixedKF == 0) return`
    else if (nf == 0) st = LBA_NOTHING_FREE;
    c.hdr[LBA_H_STATUS] = st;
    c.act = st == LBA_OK ? LBA_BUILD : LBA_DONE;
    for (int j = 0; j < 6 * a.n_free; ++j) w.xp[j] = 0.0;                    // the solver's x: a failed factorisation leaves the previous solve's there
}

// ---- the folds ----------------------------------------------------------------------------------------------------------------------------------------
// Every sum over many terms is the 256-lane fold of xfh_pose_optimize_device: lane l adds the terms l, l + 256, ... in that order to 0, the xor butterfly
// 32, 16, .. 1 inside each wave of 64, the four waves in order.  On the host the lanes are an array.
inline double lba_host_fold(const double* part, int stride) {              // part[l * stride], l = 0 .. 255
    double wv[4];
    for (int v = 0; v < 4; ++v) {
        double x[64], y[64];
        for (int l = 0; l < 64; ++l) x[l] = part[(size_t)(v * 64 + l) * stride];
        for (int m = 32; m >= 1; m >>= 1) {
            for (int l = 0; l < 64; ++l) y[l] = x[l] + x[l ^ m];
            for (int l = 0; l < 64; ++l) x[l] = y[l];
        }
        wv[v] = x[0];
    }
    return ((wv[0] + wv[1]) + wv[2]) + wv[3];
}

// ---- the steps, one lane's share each ---------------------------------------------------------------------------------------------------------------
// LINEARIZE / EVALUATE, keyframe k, lane l: its edges l, l + 256, ... of the keyframe-major list at the estimate in buffer `buf`.  build: the edge's
// record and, for a free keyframe, its share of Hpp and bp (acc[0 .. 26]); always the robust chi2 (acc[27]) and the chi2 computeError left (rec[27]).
XFH_HD void lba_kf_lane(const LbaArgs& a, const LbaWs& w, int k, int lane, int buf, bool build, double* acc) {
    const PosePose P = lba_pose_get(w.pose + 8 * ((size_t)buf * a.nK + k));
    const bool free_kf = w.kf_free[k] >= 0;
    const int b = w.kf_begin[k], n = w.kf_cnt[k];
    for (int i = lane; i < n; i += XFH_LBA_THREADS) {
        const int e = w.kf_edges[b + i], p = w.edge_pt[e];
        const double* Xp = w.pt + 3 * ((size_t)buf * a.nP + p);
        const double X[3] = {Xp[0], Xp[1], Xp[2]};
        double obs[3];
        lba_obs(a, e, obs);
        const bool stereo = lba_stereo(a, e);
        double* rec = w.rec + (size_t)XFH_LBA_REC * e;
        if (build) {
            LbaLin L;
            lba_edge_linearize(P, a.cam, X, obs, stereo, a.w, &L);
            lba_edge_record(L, stereo, a.w, free_kf, rec);
            if (free_kf) pose_accumulate(acc, L.Jp, L.e, stereo, a.w, L.rho1);
            acc[27] += L.rho0;
        } else {
            double pc[3], er[3], r0, r1;
            const double chi2 = pose_edge_error(P, a.cam, X, obs, stereo, a.w, pc, er);
            pose_huber(chi2, pose_delta(stereo), &r0, &r1);
            rec[27] = chi2;
            acc[27] += r0;
        }
    }
}
// POINT BUILD, point p: Hll and bl, the shares of its edges added to 0 in edge order (g2o's own order)
XFH_HD void lba_point_build(const LbaArgs& a, const LbaWs& w, int p) {
    double H[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, bl[3] = {0.0, 0.0, 0.0};
    int b, e;
    lba_point_range(a, p, &b, &e);
    for (int k = b; k < e; ++k) {
        if (w.edge_pt[k] != p) continue;
        const double* rec = w.rec + (size_t)XFH_LBA_REC * k;
        for (int n = 0; n < 6; ++n) H[n] += rec[n];
        for (int n = 0; n < 3; ++n) bl[n] += rec[6 + n];
    }
    for (int n = 0; n < 6; ++n) w.Hll[6 * (size_t)p + n] = H[n];
    for (int n = 0; n < 3; ++n) w.bl[3 * (size_t)p + n] = bl[n];
}
// computeLambdaInit over the diagonal entries j = 0 .. 6 nF + 3 nP - 1 (free keyframes in index order, then the points): entry j
XFH_HD double lba_diag_entry(const LbaArgs& a, const LbaWs& w, int j) {
    const int np = 6 * a.n_free;
    if (j < np) {
        const int c = j % 6, n = c * 6 - c * (c - 1) / 2;                   // the index of (c, c) in the upper triangle row by row
        return fabs(w.kf_sum[(size_t)XFH_POSE_NSUM * w.free_kf[j / 6] + n]);
    }
    const int p = (j - np) / 3, c = (j - np) % 3;
    return fabs(w.Hll[6 * (size_t)p + (c == 0 ? 0 : (c == 1 ? 3 : 5))]);
}
// std::max(fabs(H_jj), m) over a run of entries: a NaN entry replaces m and is replaced by the next one.  (m, seen a NaN) of a run combine in order.
XFH_HD void lba_max_step(double a, double* m, int* nan) { if (a != a) *nan = 1; *m = (a < *m) ? *m : a; }
XFH_HD void lba_max_join(double rm, int rnan, double* m, int* nan) {
    if (rnan) { *m = rm; *nan = 1; } else *m = (rm < *m) ? *m : rm;
}
// the term j of computeScale, j = 0 .. 6 nF + nP - 1: x_j (lambda x_j + b_j) of a pose unknown, then each point's three terms added to 0 (UPDATE left them)
XFH_HD double lba_scale_term(const LbaArgs& a, const LbaWs& w, int j) {
    const int np = 6 * a.n_free;
    if (j >= np) return w.pscale[j - np];
    const double x = w.xp[j];
    return x * (w.ctl->lambda * x + w.kf_sum[(size_t)XFH_POSE_NSUM * w.free_kf[j / 6] + 21 + j % 6]);
}
// SCHUR, the pair of free keyframes (i, j), i <= j, lane l: the edges l, l + 256, ... of keyframe i; Y = W_e Dinv_p; acc[6 a + b] += sum_c Y[a][c]
// W_e'[b][c] for every edge e' of the same point at keyframe j, in edge order; i == j: acc[36 + a] += sum_c Y[a][c] bl_p[c]
XFH_HD void lba_schur_lane(const LbaArgs& a, const LbaWs& w, int i, int j, int lane, double* acc) {
    const int ki = w.free_kf[i], kj = w.free_kf[j], b = w.kf_begin[ki], n = w.kf_cnt[ki];
    const double lambda = w.ctl->lambda;
    for (int t = lane; t < n; t += XFH_LBA_THREADS) {
        const int e = w.kf_edges[b + t], p = w.edge_pt[e];
        double D[9], Y[18];
        lba_point_block(w.Hll + 6 * (size_t)p, lambda, D);
        const double* W = w.rec + (size_t)XFH_LBA_REC * e + 9;
        _Pragma("unroll")
        for (int r = 0; r < 6; ++r)
            _Pragma("unroll")
            for (int c = 0; c < 3; ++c) Y[3 * r + c] = (W[3 * r] * D[c] + W[3 * r + 1] * D[3 + c]) + W[3 * r + 2] * D[6 + c];
        if (i == j) {
            const double* bl = w.bl + 3 * (size_t)p;
            _Pragma("unroll")
            for (int r = 0; r < 6; ++r) acc[36 + r] += (Y[3 * r] * bl[0] + Y[3 * r + 1] * bl[1]) + Y[3 * r + 2] * bl[2];
        }
        int pb, pe;
        lba_point_range(a, p, &pb, &pe);
        for (int k = pb; k < pe; ++k) {
            if (w.edge_pt[k] != p || a.edge_kf[k] != kj) continue;
            const double* V = w.rec + (size_t)XFH_LBA_REC * k + 9;
            _Pragma("unroll")
            for (int r = 0; r < 6; ++r)
                _Pragma("unroll")
                for (int c = 0; c < 6; ++c) acc[6 * r + c] += (Y[3 * r] * V[3 * c] + Y[3 * r + 1] * V[3 * c + 1]) + Y[3 * r + 2] * V[3 * c + 2];
        }
    }
}
// the folded sums of the pair -> the lower triangle of S (row stride n = 6 nF) and, i == j, b_S
XFH_HD void lba_schur_store(const LbaArgs& a, const LbaWs& w, int i, int j, const double* sum) {
    const size_t n = (size_t)6 * a.n_free;
    const double lambda = w.ctl->lambda;
    if (i == j) {
        const double* Hs = w.kf_sum + (size_t)XFH_POSE_NSUM * w.free_kf[i];
        int m = 0;
        for (int r = 0; r < 6; ++r)
            for (int c = r; c < 6; ++c, ++m) w.S[(6 * (size_t)i + c) * n + 6 * (size_t)i + r] = ((r == c) ? Hs[m] + lambda : Hs[m]) - sum[6 * r + c];
        for (int r = 0; r < 6; ++r) w.bS[6 * (size_t)i + r] = Hs[21 + r] - sum[36 + r];
    } else {
        for (int r = 0; r < 6; ++r)
            for (int c = 0; c < 6; ++c) w.S[(6 * (size_t)j + c) * n + 6 * (size_t)i + r] = -sum[6 * r + c];
    }
}
// UPDATE, point p: the step by back-substitution (when the factorisation held; the previous step otherwise), the trial estimate, its computeScale terms
XFH_HD void lba_point_update(const LbaArgs& a, const LbaWs& w, int p) {
    const LbaCtl& c = *w.ctl;
    const double* X = w.pt + 3 * ((size_t)c.cur * a.nP + p);
    double* Xn = w.pt + 3 * ((size_t)(1 - c.cur) * a.nP + p);
    double* xl = w.xl + 3 * (size_t)p;
    if (w.pt_edges[p] == 0) { Xn[0] = X[0]; Xn[1] = X[1]; Xn[2] = X[2]; w.pscale[p] = 0.0; return; }   // not a vertex of the graph
    const double* bl = w.bl + 3 * (size_t)p;
    if (c.solved) {
        double t[3] = {bl[0], bl[1], bl[2]}, D[9];
        int b, e;
        lba_point_range(a, p, &b, &e);
        for (int k = b; k < e; ++k) {
            if (w.edge_pt[k] != p) continue;
            const int f = w.kf_free[a.edge_kf[k]];
            if (f < 0) continue;
            const double* W = w.rec + (size_t)XFH_LBA_REC * k + 9;
            const double* x = w.xp + 6 * (size_t)f;
            for (int r = 0; r < 6; ++r) { t[0] = t[0] - W[3 * r] * x[r]; t[1] = t[1] - W[3 * r + 1] * x[r]; t[2] = t[2] - W[3 * r + 2] * x[r]; }
        }
        lba_point_block(w.Hll + 6 * (size_t)p, c.lambda, D);
        for (int r = 0; r < 3; ++r) xl[r] = (D[3 * r] * t[0] + D[3 * r + 1] * t[1]) + D[3 * r + 2] * t[2];
    }
    double s = 0.0;
    for (int r = 0; r < 3; ++r) { Xn[r] = X[r] + xl[r]; s += xl[r] * (c.lambda * xl[r] + bl[r]); }
    w.pscale[p] = s;
}
XFH_HD void lba_kf_update(const LbaArgs& a, const LbaWs& w, int k) {
    const int f = w.kf_free[k];
    if (f < 0) return;                                                       // a fixed keyframe's pose is the same in both buffers
    const LbaCtl& c = *w.ctl;
    PosePose n;
    pose_oplus(w.xp + 6 * (size_t)f, lba_pose_get(w.pose + 8 * ((size_t)c.cur * a.nK + k)), &n);
    lba_pose_put(n, w.pose + 8 * ((size_t)(1 - c.cur) * a.nK + k));
}

// ---- the Levenberg decisions (optimization_algorithm_levenberg.cpp:61-194), the same as geo_lm_after_build / geo_lm_after_trial with the sums handed in ---
XFH_HD void lba_lm_after_build(LbaCtl& S, double chi, double max_diag) {
    S.currentChi = chi; S.iniChi = chi;
    if (S.iter == 0) { S.lambda = 1e-5 * max_diag; S.ni = 2.0; S.nbad_lm = 0; }
    S.qmax = 0;
    ++S.hdr[LBA_H_ITERATIONS];
    S.act = LBA_TRIAL;
}
// chi: the robust chi2 at the trial estimate; scale: the folded computeScale sum before its 1e-3
XFH_HD void lba_lm_after_trial(LbaCtl& S, double chi, double scale) {
    ++S.hdr[LBA_H_TRIALS];
    if (!S.solved) ++S.hdr[LBA_H_LDLT_FAILURES];
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
        S.cur = 1 - S.cur;                                                  // the trial estimate becomes the estimate
    } else {
        S.lambda *= S.ni; S.ni *= 2.0;                                      // pop(): the other buffer is simply not taken; the edges keep its errors
        ++S.hdr[LBA_H_REJECTED];
    }
    ++S.qmax;
    if (rho < 0.0 && S.qmax < GEO_LM_MAX_TRIALS) { S.act = LBA_TRIAL; return; }
    if (S.qmax == GEO_LM_MAX_TRIALS || rho == 0.0) { S.act = LBA_DONE; return; }
    if ((S.iniChi - S.currentChi) * 1e3 < S.iniChi) ++S.nbad_lm; else S.nbad_lm = 0;
    if (S.nbad_lm >= 3) { S.act = LBA_DONE; return; }
    S.act = ++S.iter < S.max_it ? LBA_BUILD : LBA_DONE;
}

// ---- the dense LDL^T of S, n = 6 nF: the lower triangle of S (row stride n) becomes L, its diagonal d.  Unpivoted; false at the first pivot that is not
// > 0 (a NaN included), with x untouched.  Right-looking: after column k, S[i][j] -= L[i][k] * L[j][k] * d[k] for k < j <= i, so every entry receives
// its terms in ascending k -- the order of geo_ldlt_solve.  Forward substitution takes its terms in ascending k, back-substitution in DESCENDING k
// (the order in which a column-parallel solve has them).  This is the host's loop; k_lba_solve spreads the same operations over one workgroup.
inline bool lba_ldlt_solve_host(double* S, int n, const double* b, double* x, double* y) {
    const size_t N = (size_t)n;
    for (int k = 0; k < n; ++k) {
        const double dk = S[k * N + k];
        if (!(dk > 0.0)) return false;
        for (int i = k + 1; i < n; ++i) S[i * N + k] = S[i * N + k] / dk;
        for (int i = k + 1; i < n; ++i)
            for (int j = k + 1; j <= i; ++j) S[i * N + j] = S[i * N + j] - S[i * N + k] * S[j * N + k] * dk;
    }
    for (int i = 0; i < n; ++i) y[i] = b[i];
    for (int k = 0; k < n; ++k)
        for (int i = k + 1; i < n; ++i) y[i] = y[i] - S[i * N + k] * y[k];
    for (int i = 0; i < n; ++i) y[i] = y[i] / S[i * N + i];
    for (int k = n - 1; k >= 0; --k)
        for (int i = 0; i < k; ++i) y[i] = y[i] - S[k * N + i] * y[k];
    for (int i = 0; i < n; ++i) x[i] = y[i];
    return true;
}

// ---- the outputs ------------------------------------------------------------------------------------------------------------------------------------
XFH_HD void lba_finish_kf(const LbaArgs& a, const LbaWs& w, int k) {
    const int row = a.kf_row[k];
    float* out = a.Tcw_out + 12 * (size_t)k;
    const bool ok = lba_row_ok(row, a.pose_rows);
    if (w.kf_free[k] < 0 || w.ctl->hdr[LBA_H_STATUS] != LBA_OK) {           // a fixed keyframe, or a call that optimised nothing: the input's bits
        for (int n = 0; n < 12; ++n) out[n] = ok ? a.pose_table[12 * (size_t)row + n] : 0.0f;
        return;
    }
    pose_to_tcw(lba_pose_get(w.pose + 8 * ((size_t)w.ctl->cur * a.nK + k)), out);
    if (a.write_back) for (int n = 0; n < 12; ++n) a.pose_table[12 * (size_t)row + n] = out[n];
}
XFH_HD void lba_finish_point(const LbaArgs& a, const LbaWs& w, int p) {
    const int row = a.point_row[p];
    float* out = a.points_out + 3 * (size_t)p;
    const bool ok = lba_row_ok(row, a.point_rows);
    if (w.pt_edges[p] == 0 || w.ctl->hdr[LBA_H_STATUS] != LBA_OK) {
        for (int n = 0; n < 3; ++n) out[n] = ok ? a.point_table[3 * (size_t)row + n] : 0.0f;
        return;
    }
    for (int n = 0; n < 3; ++n) out[n] = (float)w.pt[3 * ((size_t)w.ctl->cur * a.nP + p) + n];
    if (a.write_back) for (int n = 0; n < 3; ++n) a.point_table[3 * (size_t)row + n] = out[n];
}
// `e->chi2() > 5.991 || !e->isDepthPositive()` (7.815 for a stereo edge): chi2 of the error the last computeError left, the depth afresh at the final
// estimate.  Returns the flag; an edge that is no edge has flag 0 and chi2 0.
XFH_HD int lba_finish_edge(const LbaArgs& a, const LbaWs& w, int e) {
    const int p = w.edge_pt[e];
    int flag = 0;
    float chi = 0.0f;
    if (p >= 0 && w.ctl->hdr[LBA_H_STATUS] == LBA_OK && w.ctl->hdr[LBA_H_ITERATIONS] > 0) {
        const int cur = w.ctl->cur;
        const PosePose P = lba_pose_get(w.pose + 8 * ((size_t)cur * a.nK + a.edge_kf[e]));
        const double* X = w.pt + 3 * ((size_t)cur * a.nP + p);
        const double Xv[3] = {X[0], X[1], X[2]};
        double r[3];
        pose_rotate(P.q, Xv, r);
        const double c2 = w.rec[(size_t)XFH_LBA_REC * e + 27];
        flag = (c2 > (lba_stereo(a, e) ? 7.815 : 5.991) || !(r[2] + P.t[2] > 0.0)) ? 1 : 0;
        chi = (float)c2;
    }
    a.erase[e] = (unsigned char)flag; a.chi2[e] = chi;
    return flag;
}
XFH_HD void lba_finish_header(const LbaArgs& a, const LbaWs& w) {
    for (int k = 0; k < XFH_LBA_HDR_INTS; ++k) a.header[k] = w.ctl->hdr[k];
    a.header[LBA_H_ERASE] = w.ctl->n_erase;
    *a.final_chi2 = w.ctl->currentChi;
}

// ---- the whole rule on ONE host thread: the kernels' steps in the schedule's order, every fold as the 256 lanes make it ------------------------------
inline void lba_host_kf_pass(const LbaArgs& a, const LbaWs& w, int buf, bool build) {
    static thread_local double part[XFH_LBA_THREADS][XFH_POSE_NSUM];
    for (int k = 0; k < a.nK; ++k) {
        for (int l = 0; l < XFH_LBA_THREADS; ++l) {
            for (int n = 0; n < XFH_POSE_NSUM; ++n) part[l][n] = 0.0;
            lba_kf_lane(a, w, k, l, buf, build, part[l]);
        }
        if (build) for (int n = 0; n < XFH_POSE_NSUM; ++n) w.kf_sum[(size_t)XFH_POSE_NSUM * k + n] = lba_host_fold(&part[0][n], XFH_POSE_NSUM);
        else w.kf_chi[k] = lba_host_fold(&part[0][27], XFH_POSE_NSUM);
    }
}
template <class Term>
inline double lba_host_fold_terms(int count, Term term) {
    double part[XFH_LBA_THREADS];
    for (int l = 0; l < XFH_LBA_THREADS; ++l) { double s = 0.0; for (int j = l; j < count; j += XFH_LBA_THREADS) s += term(j); part[l] = s; }
    return lba_host_fold(part, 1);
}
// chi_hook (tests only): what the decision sees in place of the robust chi2 of trial number `trial` (0, 1, ..)
inline void lba_host_run(const LbaArgs& a, double (*chi_hook)(int trial, double chi) = nullptr) {
    const LbaWs w = lba_ws(a.ws, a.nK, a.nP, a.nE, a.n_free);
    LbaCtl& c = *w.ctl;
    for (int e = 0; e < a.nE; ++e) w.edge_pt[e] = lba_edge_plan(a, e);
    for (int k = 0; k < a.nK; ++k) {
        int n = 0, m = 0, s = 0;
        for (int e = 0; e < a.nE; ++e)
            if (w.edge_pt[e] >= 0 && a.edge_kf[e] == k) { ++n; if (lba_stereo(a, e)) ++s; else ++m; }
        w.kf_cnt[k] = n; w.kf_mono[k] = m; w.kf_stereo[k] = s;
        lba_kf_init(a, w, k);
    }
    for (int p = 0; p < a.nP; ++p) lba_point_init(a, w, p);
    lba_plan_scan(a, w);
    for (int k = 0; k < a.nK; ++k) {
        int n = w.kf_begin[k];
        for (int e = 0; e < a.nE; ++e) if (w.edge_pt[e] >= 0 && a.edge_kf[e] == k) w.kf_edges[n++] = e;
    }
    const int nF = a.n_free, n = 6 * nF;
    double* y = n > 0 ? new double[n] : nullptr;
    for (int step = 0; step < a.max_it * (GEO_LM_MAX_TRIALS + 1) && c.act != LBA_DONE; ++step) {
        if (c.act == LBA_BUILD) {
            lba_host_kf_pass(a, w, c.cur, true);
            for (int p = 0; p < a.nP; ++p) lba_point_build(a, w, p);
            const double chi = lba_host_fold_terms(a.nK, [&](int k) { return w.kf_sum[(size_t)XFH_POSE_NSUM * k + 27]; });
            double m = 0.0;
            int nan = 0;
            for (int j = 0; j < n + 3 * a.nP; ++j) lba_max_step(lba_diag_entry(a, w, j), &m, &nan);
            lba_lm_after_build(c, chi, m);
            continue;
        }
        for (int i = 0; i < nF; ++i)
            for (int j = i; j < nF; ++j) {
                static thread_local double part[XFH_LBA_THREADS][42];
                double sum[42];
                for (int l = 0; l < XFH_LBA_THREADS; ++l) { for (int t = 0; t < 42; ++t) part[l][t] = 0.0; lba_schur_lane(a, w, i, j, l, part[l]); }
                for (int t = 0; t < 42; ++t) sum[t] = lba_host_fold(&part[0][t], 42);
                lba_schur_store(a, w, i, j, sum);
            }
        c.solved = lba_ldlt_solve_host(w.S, n, w.bS, w.xp, y) ? 1 : 0;
        for (int p = 0; p < a.nP; ++p) lba_point_update(a, w, p);
        for (int k = 0; k < a.nK; ++k) lba_kf_update(a, w, k);
        lba_host_kf_pass(a, w, 1 - c.cur, false);
        double chi = lba_host_fold_terms(a.nK, [&](int k) { return w.kf_chi[k]; });
        if (chi_hook) chi = chi_hook(c.hdr[LBA_H_TRIALS], chi);
        const double scale = lba_host_fold_terms(n + a.nP, [&](int j) { return lba_scale_term(a, w, j); });
        lba_lm_after_trial(c, chi, scale);
    }
    delete[] y;
    for (int k = 0; k < a.nK; ++k) lba_finish_kf(a, w, k);
    for (int p = 0; p < a.nP; ++p) lba_finish_point(a, w, p);
    for (int e = 0; e < a.nE; ++e) c.n_erase += lba_finish_edge(a, w, e);
    lba_finish_header(a, w);
}
