// optsim3_math.h -- the arithmetic of Optimizer::OptimizeSim3 (src/Optimizer.cc:2100-2381) as LoopClosing drives it between its two Sim3 projection
// searches, written ONCE for k_sim3_optimize (optsim3.hip.h), the host form xfh_sim3_optimize_host, the single-piece entry points of
// capi_optsim3.cpp and the sanitizer program tests/cpp/asan_optsim3_test.cpp: the g2o::Sim3 state (thirdparty/g2o/g2o/types/sim3.h) with its
// exponential, product and inverse, the two projection edges of OptimizableTypes.h:175-215 with g2o's NUMERIC Jacobian
// (base_binary_edge.hpp:130-205), one edge's share of H and b, and the two rounds around the Levenberg machine of geom_common.h, which one lane or
// one host thread drives.  The quaternion rules, the quaternion product, the rotation of a vector and the Huber kernel are
// poseopt_math.h's.  IEEE double throughout, every product and sum in the order written here (the library is built without contraction);
// tests/ref_optsim3.py restates these lines.
#pragma once
#include "poseopt_math.h"

#define XFH_OS3_THREADS 256
#define XFH_OS3_NSUM 36                   /* 28 upper entries of H (row-major, i <= j), 7 of b, the robust chi2 */
#define XFH_OS3_ITERS_FIRST 5             /* optimize(5) */
#define XFH_OS3_ITERS_MORE 5              /* nMoreIterations without a bad pair, */
#define XFH_OS3_ITERS_MORE_BAD 10         /* and with one */
#define XFH_OS3_MIN_PAIRS 10              /* `if (nCorrespondences - nBad < 10) return 0` */
#define XFH_OS3_MAX_PASSES ((XFH_OS3_ITERS_FIRST + XFH_OS3_ITERS_MORE_BAD) * (1 + GEO_LM_MAX_TRIALS) + 2)
#define XFH_OS3_DELTA 1e-9                /* base_binary_edge.hpp:147 */
#define XFH_OS3_HEADER_INTS 16
#define XFH_OS3_S12_FLOATS 13

// a pair's state word: bit 0 it has its two edges, bit 1 its point is in KF2, bit 2 bad in the first classification, bit 3 bad in the final one
enum { OS3_EDGE = 1, OS3_IN_KF2 = 2, OS3_BAD_FIRST = 4, OS3_BAD_FINAL = 8 };
enum { XFH_OS3_NO_EDGE = 0, XFH_OS3_BAD_FIRST = 1, XFH_OS3_BAD_FINAL = 2, XFH_OS3_INLIER = 3 };
enum { XFH_OS3_H_CORR = 0, XFH_OS3_H_IN_KF2 = 1, XFH_OS3_H_OUT_KF2 = 2, XFH_OS3_H_BAD = 3, XFH_OS3_H_BAD_OUT_KF2 = 4, XFH_OS3_H_MORE = 5, XFH_OS3_H_RETURN = 6,
       XFH_OS3_H_ROUNDS = 7, XFH_OS3_H_ITERATIONS = 8, XFH_OS3_H_TRIALS = 9, XFH_OS3_H_REJECTED = 10, XFH_OS3_H_LDLT_FAILURES = 11 };

struct Os3Sim { double q[4]; double t[3]; double s; };                    // g2o::Sim3: quaternion (x, y, z, w), NOT normalised, translation, scale
struct Os3Cam { double fx, fy, cx, cy; };
// est, its inverse, and the 14 + 14 similarities of one linearisation: pert[2 d] = exp(+delta e_d) * est, pert[2 d + 1] = exp(-delta e_d) * est
struct Os3Sims { Os3Sim est, inv; Os3Sim pert[14], pinv[14]; };
struct Os3Pair { float P1[3], P2[3], o1[2], o2[2]; };                     // P3D1c, P3D2c, obs1, obs2
// the arguments of k_sim3_optimize: device pointers as xfh_sim3_optimize_device takes them; w = (double)inv_sigma2, delta = (double)sqrtf(th2)
struct Os3Args {
    int n1, M1, nq, n2, side1_shared, fix_scale, all_points;
    const float *T1w, *xy_un1, *points1; const int* point1;
    const int* assigned; const float* points2; const unsigned char* flags2; const int* index2; const float *xy_un2, *T2w;
    const float* S12; size_t S12_stride; const float* Tmw;
    Os3Cam cam1, cam2; double th2, w1, w2, delta;
    char* ws; size_t ws_stride;
    int* assigned_out; unsigned char* status; float* chi2; double* state; float* S12_out; size_t S12_out_stride; float *Tcw, *Ow; int* header;
    double* final_chi2;
};

// the workspace of one problem: double last[n1][2], int st[n1].  The kernel instance for n1 <= 1024 keeps both in registers and does not touch it.
XFH_HD size_t os3_ws_last_bytes(int n1) { return ((size_t)n1 * 16 + 255) & ~(size_t)255; }
XFH_HD size_t os3_ws_bytes(int n1) { return os3_ws_last_bytes(n1) + (((size_t)n1 * 4 + 255) & ~(size_t)255); }

// ---- g2o::Sim3 -------------------------------------------------------------------------------------------------------------------------------------
// Sim3(Matrix3d R, t, s) of 13 floats (R row-major 9, t 3, s): Quaterniond(R) and nothing else, and back through toRotationMatrix
XFH_HD void os3_from_floats(const float* S, Os3Sim* o) {
    pose_quat_from_entries((double)S[0], (double)S[1], (double)S[2], (double)S[3], (double)S[4], (double)S[5], (double)S[6], (double)S[7], (double)S[8], o->q);
    o->t[0] = (double)S[9]; o->t[1] = (double)S[10]; o->t[2] = (double)S[11]; o->s = (double)S[12];
}
XFH_HD void os3_to_floats(const Os3Sim& S, float* o) {
    double R[9];
    pose_matrix_from_quat(S.q, R);
    _Pragma("unroll")
    for (int k = 0; k < 9; ++k) o[k] = (float)R[k];
    o[9] = (float)S.t[0]; o[10] = (float)S.t[1]; o[11] = (float)S.t[2]; o[12] = (float)S.s;
}
// map: s * (r * X) + t
XFH_HD void os3_map(const Os3Sim& S, const double* X, double* o) {
    double r[3];
    pose_rotate(S.q, X, r);
    o[0] = S.s * r[0] + S.t[0]; o[1] = S.s * r[1] + S.t[1]; o[2] = S.s * r[2] + S.t[2];
}
// inverse: (r*, r* * ((-1 / s) * t), 1 / s)
XFH_HD void os3_inverse(const Os3Sim& S, Os3Sim* o) {
    o->q[0] = -S.q[0]; o->q[1] = -S.q[1]; o->q[2] = -S.q[2]; o->q[3] = S.q[3];
    const double m = -1.0 / S.s;
    const double v[3] = {m * S.t[0], m * S.t[1], m * S.t[2]};
    pose_rotate(o->q, v, o->t);
    o->s = 1.0 / S.s;
}
// operator*: r = a.r * b.r, t = a.s * (a.r * b.t) + a.t, s = a.s * b.s; nothing is normalised
XFH_HD void os3_mul(const Os3Sim& A, const Os3Sim& B, Os3Sim* o) {
    double rt[3];
    pose_rotate(A.q, B.t, rt);
    pose_quat_mul(A.q, B.q, o->q);
    o->t[0] = A.s * rt[0] + A.t[0]; o->t[1] = A.s * rt[1] + A.t[1]; o->t[2] = A.s * rt[2] + A.t[2];
    o->s = A.s * B.s;
}
// Sim3(Vector7d update), sim3.h:70-142: u = (omega, upsilon, sigma), all four branches of (|sigma| < 1e-5, theta < 1e-5)
XFH_HD void os3_exp(const double* u, Os3Sim* e) {
    const double wx = u[0], wy = u[1], wz = u[2], sigma = u[6];
    const double theta = sqrt((wx * wx + wy * wy) + wz * wz);
    const double O[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
    double O2[9], R[9];
    _Pragma("unroll")
    for (int r = 0; r < 3; ++r)
        _Pragma("unroll")
        for (int c = 0; c < 3; ++c) O2[3 * r + c] = (O[3 * r] * O[c] + O[3 * r + 1] * O[3 + c]) + O[3 * r + 2] * O[6 + c];
    const double s = exp(sigma), eps = 0.00001;
    const bool small = theta < eps;
    double A, B, C;
    if (fabs(sigma) < eps) {
        C = 1.0;
        if (small) { A = 1.0 / 2.0; B = 1.0 / 6.0; }
        else {
            const double theta2 = theta * theta;
            A = (1.0 - cos(theta)) / theta2;
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (s - 1.0) / sigma;
        if (small) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1.0) * s + 1.0) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1.0) * s) / (sigma2 * sigma);
        } else {
            const double a = s * sin(theta), b = s * cos(theta), theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1.0 - b) * theta) / (theta * c);
            B = (C - ((b - 1.0) * sigma + a * theta) / c) * 1.0 / theta2;
        }
    }
    if (small) {
        _Pragma("unroll")
        for (int k = 0; k < 9; ++k) R[k] = ((k % 4 == 0 ? 1.0 : 0.0) + O[k]) + O2[k];
    } else {
        const double ra = sin(theta) / theta, rb = (1.0 - cos(theta)) / (theta * theta);
        _Pragma("unroll")
        for (int k = 0; k < 9; ++k) R[k] = ((k % 4 == 0 ? 1.0 : 0.0) + ra * O[k]) + rb * O2[k];
    }
    pose_quat_from_matrix(R, e->q);
    double W[9];
    _Pragma("unroll")
    for (int k = 0; k < 9; ++k) W[k] = (A * O[k] + B * O2[k]) + C * (k % 4 == 0 ? 1.0 : 0.0);
    _Pragma("unroll")
    for (int r = 0; r < 3; ++r) e->t[r] = (W[3 * r] * u[3] + W[3 * r + 1] * u[4]) + W[3 * r + 2] * u[5];
    e->s = s;
}
// VertexSim3Expmap::oplusImpl (OptimizableTypes.h:158-167): update[6] = 0 under _fix_scale, then Sim3(update) * estimate
XFH_HD void os3_oplus(const double* u, const Os3Sim& est, int fix_scale, Os3Sim* out) {
    const double v[7] = {u[0], u[1], u[2], u[3], u[4], u[5], fix_scale ? 0.0 : u[6]};
    Os3Sim e;
    os3_exp(v, &e);
    os3_mul(e, est, out);
}
// piece j of the similarities of one pass at `est`: j < 14 the perturbed one (d = j / 2, sign + for even j) and its inverse, j == 14 est and its inverse
XFH_HD void os3_sims_piece(const Os3Sim& est, int fix_scale, int j, Os3Sims* S) {
    if (j == 14) { S->est = est; os3_inverse(est, &S->inv); return; }
    const int d = j >> 1;
    const double v = (j & 1) ? -XFH_OS3_DELTA : XFH_OS3_DELTA;
    double u[7];
    _Pragma("unroll")
    for (int k = 0; k < 7; ++k) u[k] = k == d ? v : 0.0;
    Os3Sim p;
    os3_oplus(u, est, fix_scale, &p);
    S->pert[j] = p;
    os3_inverse(p, &S->pinv[j]);
}

// ---- the edges -------------------------------------------------------------------------------------------------------------------------------------
// computeError + chi2 of one edge through the similarity T (S12 for e12, its inverse for e21): e = obs - project(T.map(X)), Pinhole::project in double
XFH_HD double os3_edge_error(const Os3Sim& T, const Os3Cam& cam, const double* X, const double* obs, double w, double* e) {
    double p[3];
    os3_map(T, X, p);
    e[0] = obs[0] - (cam.fx * p[0] / p[2] + cam.cx);
    e[1] = obs[1] - (cam.fy * p[1] / p[2] + cam.cy);
    return e[0] * (w * e[0]) + e[1] * (w * e[1]);
}
// the numeric linearizeOplus: column d = (e(pert[2 d]) - e(pert[2 d + 1])) * (1 / (2 delta)); J is [2][7] row-major
XFH_HD void os3_edge_jacobian(const Os3Sim* pert, const Os3Cam& cam, const double* X, const double* obs, double* J) {
    const double scalar = 1.0 / (2 * XFH_OS3_DELTA);
    _Pragma("unroll")
    for (int k = 0; k < 14; ++k) J[k] = 0.0;
    // d stays a run-time loop, and column d reaches J through selects: unrolled, the 14 similarities of an edge (112 doubles) are loop invariants
    // that the compiler keeps in registers across the slots, which spills; J itself is indexed at compile time only
    _Pragma("clang loop unroll(disable)")
    for (int d = 0; d < 7; ++d) {
        double ep[2], em[2];
        const Os3Sim Tp = pert[2 * d], Tm = pert[2 * d + 1];
        os3_edge_error(Tp, cam, X, obs, 1.0, ep);
        os3_edge_error(Tm, cam, X, obs, 1.0, em);
        const double c0 = scalar * (ep[0] - em[0]), c1 = scalar * (ep[1] - em[1]);
        _Pragma("unroll")
        for (int k = 0; k < 7; ++k) { J[k] = k == d ? c0 : J[k]; J[7 + k] = k == d ? c1 : J[7 + k]; }
    }
}
// constructQuadraticForm of one edge (base_binary_edge.hpp:56-120) added to a lane's partial sums: H += B^T (rho1 w) B, b -= rho1 B^T (w e)
XFH_HD void os3_accumulate(double* acc, const double* J, const double* e, double w, double rho1) {
    const double ww = rho1 * w;
    int n = 0;
    _Pragma("unroll")
    for (int i = 0; i < 7; ++i)
        _Pragma("unroll")
        for (int j = i; j < 7; ++j, ++n) acc[n] += J[i] * (ww * J[j]) + J[7 + i] * (ww * J[7 + j]);
    _Pragma("unroll")
    for (int i = 0; i < 7; ++i) acc[28 + i] -= rho1 * (J[i] * (w * e[0]) + J[7 + i] * (w * e[1]));
}

// keypoint i of problem pb: the state word of its pair (0: no edge), and P3D1c, P3D2c, obs1, obs2 when it has one (:2167-2304)
XFH_HD int os3_pair_load(const Os3Args& a, int pb, int i, Os3Pair* p) {
    const size_t s1 = a.side1_shared ? 0 : (size_t)pb;
    const int q = a.assigned[(size_t)pb * a.n1 + i];
    if (q < 0 || q >= a.nq) return 0;                                      // !vpMatches1[i]
    const size_t qg = (size_t)pb * a.nq + q;
    if (!(a.flags2[qg] & 1)) return 0;                                     // pMP2->isBad()
    const int m = a.point1[s1 * a.n1 + i];
    if (m < 0 || m >= a.M1) return 0;                                      // !pMP1 or pMP1->isBad()
    const int i2 = a.index2[qg];
    const bool in2 = i2 >= 0 && i2 < a.n2;
    if (!in2 && !a.all_points) return 0;
    const float *T1 = a.T1w + s1 * 12, *T2 = a.T2w + (size_t)pb * 12, *X1 = a.points1 + (s1 * a.M1 + m) * 3, *X2 = a.points2 + qg * 3;
    _Pragma("unroll")
    for (int r = 0; r < 3; ++r) {
        p->P1[r] = ((T1[4 * r] * X1[0] + T1[4 * r + 1] * X1[1]) + T1[4 * r + 2] * X1[2]) + T1[4 * r + 3];
        p->P2[r] = ((T2[4 * r] * X2[0] + T2[4 * r + 1] * X2[1]) + T2[4 * r + 2] * X2[2]) + T2[4 * r + 3];
    }
    if (p->P2[2] < 0.0f) return 0;                                         // (a NaN z passes, as there)
    const float* k1 = a.xy_un1 + (s1 * a.n1 + i) * 2;
    p->o1[0] = k1[0]; p->o1[1] = k1[1];
    if (in2) {
        const float* k2 = a.xy_un2 + ((size_t)pb * a.n2 + i2) * 2;
        p->o2[0] = k2[0]; p->o2[1] = k2[1];
    } else {                                                               // :2275-2279: normalised coordinates, not pixels, as the reference writes them
        const float invz = 1 / p->P2[2];
        p->o2[0] = p->P2[0] * invz; p->o2[1] = p->P2[1] * invz;
    }
    return OS3_EDGE | (in2 ? OS3_IN_KF2 : 0);
}

// one pair in one pass.  l12 / l21: the chi2 of _error as the last computeActiveErrors (or the final computeError) left it.  robust: the Huber
// kernel is on (round 0); final: the classification computes fresh errors (round 1).  bad: += 1 | 65536 when not in KF2, per pair found bad.
XFH_HD void os3_pair_pass(int act, bool robust, bool final, const Os3Sims& S, const Os3Args& a, const Os3Pair& p, int& st, double& l12, double& l21, double* acc,
                          int& bad) {
    if (st & OS3_BAD_FIRST) return;                                        // removeEdge
    const double X1[3] = {(double)p.P1[0], (double)p.P1[1], (double)p.P1[2]}, X2[3] = {(double)p.P2[0], (double)p.P2[1], (double)p.P2[2]};
    const double o1[2] = {(double)p.o1[0], (double)p.o1[1]}, o2[2] = {(double)p.o2[0], (double)p.o2[1]};
    double e[2];
    if (act == GEO_LM_CLASSIFY) {
        if (final) {
            const Os3Sim T = S.est, Ti = S.inv;
            l12 = os3_edge_error(T, a.cam1, X2, o1, a.w1, e);
            l21 = os3_edge_error(Ti, a.cam2, X1, o2, a.w2, e);
        }
        const bool o = l12 > a.th2 || l21 > a.th2;
        if (o) { st |= final ? OS3_BAD_FINAL : OS3_BAD_FIRST; bad += (st & OS3_IN_KF2) ? 1 : 65537; }
        return;
    }
    {
        const Os3Sim T = S.est;
        const double c = os3_edge_error(T, a.cam1, X2, o1, a.w1, e);
        l12 = c;
        double r0 = c, r1 = 1.0;
        if (robust) pose_huber(c, a.delta, &r0, &r1);
        acc[35] += r0;
        if (act == GEO_LM_BUILD) {
            double J[14];
            os3_edge_jacobian(S.pert, a.cam1, X2, o1, J);
            os3_accumulate(acc, J, e, a.w1, r1);
        }
    }
    {
        const Os3Sim T = S.inv;
        const double c = os3_edge_error(T, a.cam2, X1, o2, a.w2, e);
        l21 = c;
        double r0 = c, r1 = 1.0;
        if (robust) pose_huber(c, a.delta, &r0, &r1);
        acc[35] += r0;
        if (act == GEO_LM_BUILD) {
            double J[14];
            os3_edge_jacobian(S.pinv, a.cam2, X1, o2, J);
            os3_accumulate(acc, J, e, a.w2, r1);
        }
    }
}
// what keypoint i reports: vpMatches1[i] (NULL where the pair was found bad), the status, the two chi2 its last classification read
XFH_HD void os3_pair_store(const Os3Args& a, int pb, int i, int st, double l12, double l21) {
    const size_t kg = (size_t)pb * a.n1 + i;
    const int q = a.assigned[kg];
    const bool bad = (st & (OS3_BAD_FIRST | OS3_BAD_FINAL)) != 0;
    a.assigned_out[kg] = bad ? -1 : q;
    a.status[kg] = !(st & OS3_EDGE) ? XFH_OS3_NO_EDGE : (st & OS3_BAD_FIRST) ? XFH_OS3_BAD_FIRST : (st & OS3_BAD_FINAL) ? XFH_OS3_BAD_FINAL : XFH_OS3_INLIER;
    a.chi2[kg * 2] = (st & OS3_EDGE) ? (float)l12 : 0.0f; a.chi2[kg * 2 + 1] = (st & OS3_EDGE) ? (float)l21 : 0.0f;
}

// ---- optimize(5), the classification, optimize(5 or 10), the final classification: the Levenberg machine of geom_common.h (geo_lm_after_build /
// geo_lm_after_trial) with 7 unknowns, and around it what is OptimizeSim3's own: round 1 continues from round 0's estimate with its own iteration
// cap, CLASSIFY hands back the packed count of bad pairs, the Huber kernel is on in round 0, round 1's classification computes fresh errors.  The
// driver runs a pass over every pair with S.est's similarities.  sums: XFH_OS3_NSUM, the robust chi2 last.
struct Os3LM {
    Os3Sim input, est, backup;
    double H[28], b[7], x[7];
    double lambda, ni, currentChi, iniChi;
    int round, iter, iters, qmax, nbad_lm, solved, fix_scale;
    int hdr[XFH_OS3_HEADER_INTS];
    static constexpr int N = 7, H_ITERATIONS = XFH_OS3_H_ITERATIONS;
    static XFH_HD int iterations(const Os3LM& S) { return S.iters; }
    static XFH_HD Os3Sim oplus(const Os3LM& S) { Os3Sim n; os3_oplus(S.x, S.est, S.fix_scale, &n); return n; }
};
XFH_HD bool os3_lm_robust(const Os3LM& S) { return S.round == 0; }
XFH_HD bool os3_lm_final(const Os3LM& S) { return S.round == 1; }

XFH_HD int os3_lm_begin(Os3LM& S, const Os3Sim& input, int fix_scale, int n_corr, int n_out_kf2) {
    S.input = input; S.est = input; S.round = 0; S.iter = 0; S.iters = XFH_OS3_ITERS_FIRST; S.currentChi = 0.0; S.fix_scale = fix_scale;
    _Pragma("unroll")
    for (int k = 0; k < 7; ++k) S.x[k] = 0.0;                               // the solver's x: a failed LDLT leaves the previous solve's there
    _Pragma("unroll")
    for (int k = 0; k < XFH_OS3_HEADER_INTS; ++k) S.hdr[k] = 0;
    S.hdr[XFH_OS3_H_CORR] = n_corr; S.hdr[XFH_OS3_H_OUT_KF2] = n_out_kf2; S.hdr[XFH_OS3_H_IN_KF2] = n_corr - n_out_kf2;
    return n_corr > 0 ? GEO_LM_BUILD : GEO_LM_CLASSIFY;                     // no edge: optimize() returns at once
}
// The names under which tests/cpp/asan_optsim3_test.cpp drives the machine.  That program is the independent statement the library is compared with
// and stays as it was written before the machine was shared, so that it holds this build without having been touched: nothing else uses these.
enum { XFH_OS3_BUILD = GEO_LM_BUILD, XFH_OS3_TRIAL = GEO_LM_TRIAL, XFH_OS3_CLASSIFY = GEO_LM_CLASSIFY, XFH_OS3_DONE = GEO_LM_DONE };
XFH_HD int os3_lm_after_build(Os3LM& S, const double* sums) { return geo_lm_after_build(S, sums); }
XFH_HD int os3_lm_after_trial(Os3LM& S, double chi) { return geo_lm_after_trial(S, chi); }
XFH_HD int os3_lm_after_classify(Os3LM& S, int bad_packed) {
    const int n_bad = bad_packed & 0xFFFF, n_bad_out = bad_packed >> 16;
    ++S.hdr[XFH_OS3_H_ROUNDS];
    if (S.round == 0) {
        S.hdr[XFH_OS3_H_BAD] = n_bad; S.hdr[XFH_OS3_H_BAD_OUT_KF2] = n_bad_out;
        S.hdr[XFH_OS3_H_MORE] = n_bad > 0 ? XFH_OS3_ITERS_MORE_BAD : XFH_OS3_ITERS_MORE;
        if (S.hdr[XFH_OS3_H_CORR] - n_bad < XFH_OS3_MIN_PAIRS) { S.est = S.input; return GEO_LM_DONE; }    // return 0 before :2378: g2oS12 stays the input
        S.round = 1; S.iter = 0; S.iters = S.hdr[XFH_OS3_H_MORE];
        return GEO_LM_BUILD;                                                // continues from round 0's estimate; lambda afresh (iter == 0)
    }
    S.hdr[XFH_OS3_H_RETURN] = (S.hdr[XFH_OS3_H_CORR] - S.hdr[XFH_OS3_H_BAD]) - n_bad;
    return GEO_LM_DONE;
}

// what lane 0 writes at the end: the state, S12_out, the composed pose for the next search (LoopClosing.cc:771-773, ORBmatcher.cc:621-622), the header
XFH_HD void os3_finish(const Os3Args& a, int pb, const Os3LM& S) {
    const Os3Sim E = S.est;
    double* st = a.state + (size_t)pb * 8;
    st[0] = E.q[0]; st[1] = E.q[1]; st[2] = E.q[2]; st[3] = E.q[3]; st[4] = E.t[0]; st[5] = E.t[1]; st[6] = E.t[2]; st[7] = E.s;
    os3_to_floats(E, a.S12_out + (size_t)pb * a.S12_out_stride);
    if (a.Tmw) {
        const float* T = a.Tmw + (size_t)pb * 12;
        Os3Sim m, c;
        pose_quat_from_entries((double)T[0], (double)T[1], (double)T[2], (double)T[4], (double)T[5], (double)T[6], (double)T[8], (double)T[9], (double)T[10], m.q);
        m.t[0] = (double)T[3]; m.t[1] = (double)T[7]; m.t[2] = (double)T[11]; m.s = 1.0;
        os3_mul(E, m, &c);
        double R[9];
        pose_matrix_from_quat(c.q, R);
        const double ts[3] = {c.t[0] / c.s, c.t[1] / c.s, c.t[2] / c.s};
        float *Tc = a.Tcw + (size_t)pb * 12, *Ow = a.Ow + (size_t)pb * 3;
        _Pragma("unroll")
        for (int r = 0; r < 3; ++r) {
            Tc[4 * r] = (float)R[3 * r]; Tc[4 * r + 1] = (float)R[3 * r + 1]; Tc[4 * r + 2] = (float)R[3 * r + 2]; Tc[4 * r + 3] = (float)ts[r];
            Ow[r] = (float)(-((R[r] * ts[0] + R[3 + r] * ts[1]) + R[6 + r] * ts[2]));
        }
    }
    _Pragma("unroll")
    for (int n = 0; n < XFH_OS3_HEADER_INTS; ++n) a.header[(size_t)pb * XFH_OS3_HEADER_INTS + n] = S.hdr[n];
    a.final_chi2[pb] = S.currentChi;
}

// ---- the whole rule for problem pb on ONE host thread: the kernel's passes and its fold (lane l of 256 adds its keypoints l, l + 256, ..; the xor
// butterfly 32 .. 1 inside each wave of 64; the four waves in order), the pair state in the caller's workspace
inline double os3_host_fold(double (*part)[XFH_OS3_NSUM], int n) {
    double w[4];
    for (int wv = 0; wv < 4; ++wv) {
        double x[64], y[64];
        for (int l = 0; l < 64; ++l) x[l] = part[wv * 64 + l][n];
        for (int m = 32; m >= 1; m >>= 1) {
            for (int l = 0; l < 64; ++l) y[l] = x[l] + x[l ^ m];
            for (int l = 0; l < 64; ++l) x[l] = y[l];
        }
        w[wv] = x[0];
    }
    return ((w[0] + w[1]) + w[2]) + w[3];
}
inline void os3_host_problem(const Os3Args& a, int pb) {
    double* last = (double*)(a.ws + (size_t)pb * a.ws_stride);
    int* st = (int*)(a.ws + (size_t)pb * a.ws_stride + os3_ws_last_bytes(a.n1));
    Os3Pair p;
    int n_corr = 0, n_out = 0;
    for (int i = 0; i < a.n1; ++i) {
        st[i] = os3_pair_load(a, pb, i, &p);
        last[2 * i] = 0.0; last[2 * i + 1] = 0.0;
        n_corr += st[i] ? 1 : 0; n_out += (st[i] && !(st[i] & OS3_IN_KF2)) ? 1 : 0;
    }
    Os3LM S;
    Os3Sim in;
    os3_from_floats(a.S12 + (size_t)pb * a.S12_stride, &in);
    int act = os3_lm_begin(S, in, a.fix_scale, n_corr, n_out);
    static thread_local double part[XFH_OS3_THREADS][XFH_OS3_NSUM];
    for (int pass = 0; pass <= XFH_OS3_MAX_PASSES && act != GEO_LM_DONE; ++pass) {
        Os3Sims sims;
        for (int j = act == GEO_LM_BUILD ? 0 : 14; j < 15; ++j) os3_sims_piece(S.est, a.fix_scale, j, &sims);
        for (int l = 0; l < XFH_OS3_THREADS; ++l)
            for (int n = 0; n < XFH_OS3_NSUM; ++n) part[l][n] = 0.0;
        int bad = 0;
        for (int i = 0; i < a.n1; ++i) {
            if (!(st[i] & OS3_EDGE)) continue;
            os3_pair_load(a, pb, i, &p);
            os3_pair_pass(act, os3_lm_robust(S), os3_lm_final(S), sims, a, p, st[i], last[2 * i], last[2 * i + 1], part[i % XFH_OS3_THREADS], bad);
        }
        if (act == GEO_LM_BUILD) {
            double sums[XFH_OS3_NSUM];
            for (int n = 0; n < XFH_OS3_NSUM; ++n) sums[n] = os3_host_fold(part, n);
            act = geo_lm_after_build(S, sums);
        } else if (act == GEO_LM_TRIAL) act = geo_lm_after_trial(S, os3_host_fold(part, 35));
        else act = os3_lm_after_classify(S, bad);
    }
    for (int i = 0; i < a.n1; ++i) os3_pair_store(a, pb, i, st[i], last[2 * i], last[2 * i + 1]);
    os3_finish(a, pb, S);
}
