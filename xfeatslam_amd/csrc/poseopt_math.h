// poseopt_math.h -- the arithmetic of Optimizer::PoseOptimization (src/Optimizer.cc:814-1114, the conventional-camera branch), written ONCE for
// k_pose_optimize (poseopt.hip.h) and the host entry point xfh_pose_edge (capi_poseopt.cpp): the SE3Quat pose (types/se3quat.h), the mono edge
// EdgeSE3ProjectXYZOnlyPose with Pinhole::project / projectJac and the stereo edge EdgeStereoSE3ProjectXYZOnlyPose (types_six_dof_expmap.cpp),
// the Huber kernel, one edge's share of H and b (base_unary_edge.hpp:43-72) and the four rounds around the Levenberg machine of geom_common.h.  The
// quaternion product is written here for OptimizeSim3 (optsim3_math.h) too.  IEEE double throughout, every product and
// sum in the order written here (the library is built without contraction); tests/ref_poseopt.py restates these lines.
#pragma once
#include "geom_common.h"
#include <math.h>

#define XFH_POSE_CHI2_MONO 5.991f
#define XFH_POSE_CHI2_STEREO 7.815f
#define XFH_POSE_ROUNDS 4
#define XFH_POSE_ITERATIONS 10            /* optimize(its[it]) */
#define XFH_POSE_NSUM 28                  /* 21 upper entries of H (row-major, i <= j), 6 of b, the robust chi2 */

struct PosePose { double q[4]; double t[3]; };          // SE3Quat: unit quaternion (x, y, z, w) and translation
struct PoseCam { double fx, fy, cx, cy, bf; };
// the arguments of k_pose_optimize: device pointers as xfh_pose_optimize_device takes them, w = (double)inv_sigma2
struct PoseArgs {
    int nt, nq;
    const float* Tcw; PoseCam cam; const float* xy_un; const float* uright; const int* assigned; const float* points; double w;
    float* Tcw_out; unsigned char* outlier; float* chi2; int* header; double* final_chi2;
    char* ws; size_t ws_stride;
};

// the workspace of one problem: used by the form for nt > 4096 only, whose per-edge state does not fit the register file: double last[nt], int st[nt]
XFH_HD size_t pose_ws_last_bytes(int nt) { return ((size_t)nt * 8 + 255) & ~(size_t)255; }
XFH_HD size_t pose_ws_bytes(int nt) { return pose_ws_last_bytes(nt) + (((size_t)nt * 4 + 255) & ~(size_t)255); }

// SE3Quat::normalizeRotation: w < 0 flips the sign, then the coefficients are divided by the norm
XFH_HD void pose_normalize(double* q) {
    if (q[3] < 0.0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
    const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n;
}

// Quaterniond(Matrix3d): the trace rule, else the largest diagonal entry (the later index wins only when strictly larger).  The entries come as
// scalars and every case is written out: no run-time index, so the matrix and q stay in registers.
XFH_HD void pose_quat_from_entries(double m00, double m01, double m02, double m10, double m11, double m12, double m20, double m21, double m22, double* q) {
    double t = (m00 + m11) + m22;
    if (t > 0.0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m21 - m12) * t; q[1] = (m02 - m20) * t; q[2] = (m10 - m01) * t;
    } else {
        int i = 0;
        if (m11 > m00) i = 1;
        if (m22 > (i == 0 ? m00 : m11)) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;                        // q[i] from the diagonal, w from (k, j) - (j, k), q[j] and q[k] from the sums
        const double dii = i == 0 ? m00 : (i == 1 ? m11 : m22), djj = j == 0 ? m00 : (j == 1 ? m11 : m22), dkk = k == 0 ? m00 : (k == 1 ? m11 : m22);
        const double kj = i == 0 ? m21 - m12 : (i == 1 ? m02 - m20 : m10 - m01);
        const double ji = i == 0 ? m10 + m01 : (i == 1 ? m21 + m12 : m02 + m20);
        const double ki = i == 0 ? m20 + m02 : (i == 1 ? m01 + m10 : m12 + m21);
        t = sqrt(((dii - djj) - dkk) + 1.0);
        const double h = 0.5 * t;
        t = 0.5 / t;
        const double w = kj * t, qj = ji * t, qk = ki * t;
        q[3] = w;
        q[0] = i == 0 ? h : (j == 0 ? qj : qk);
        q[1] = i == 1 ? h : (j == 1 ? qj : qk);
        q[2] = i == 2 ? h : (j == 2 ? qj : qk);
    }
}
XFH_HD void pose_quat_from_matrix(const double* R, double* q) { pose_quat_from_entries(R[0], R[1], R[2], R[3], R[4], R[5], R[6], R[7], R[8], q); }

// Quaterniond::toRotationMatrix, row-major
XFH_HD void pose_matrix_from_quat(const double* q, double* R) {
    const double tx = 2.0 * q[0], ty = 2.0 * q[1], tz = 2.0 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3], txx = tx * q[0], txy = ty * q[0], txz = tz * q[0], tyy = ty * q[1], tyz = tz * q[1],
                 tzz = tz * q[2];
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
}

// the library's row-major 3x4 float [R|t] -> SE3Quat(Quaterniond(R), t), and back as the float cast of [toRotationMatrix | t]
XFH_HD void pose_from_tcw(const float* T, PosePose* P) {
    pose_quat_from_entries((double)T[0], (double)T[1], (double)T[2], (double)T[4], (double)T[5], (double)T[6], (double)T[8], (double)T[9], (double)T[10], P->q);
    pose_normalize(P->q);
    P->t[0] = (double)T[3]; P->t[1] = (double)T[7]; P->t[2] = (double)T[11];
}
XFH_HD void pose_to_tcw(const PosePose& P, float* T) {
    double R[9];
    pose_matrix_from_quat(P.q, R);
    _Pragma("unroll")
    for (int r = 0; r < 3; ++r) { T[4 * r] = (float)R[3 * r]; T[4 * r + 1] = (float)R[3 * r + 1]; T[4 * r + 2] = (float)R[3 * r + 2]; T[4 * r + 3] = (float)P.t[r]; }
}

// Quaterniond * Vector3d: uv = 2 (q.vec x v);  v + w uv + q.vec x uv
XFH_HD void pose_rotate(const double* q, const double* v, double* o) {
    const double ux = 2.0 * (q[1] * v[2] - q[2] * v[1]), uy = 2.0 * (q[2] * v[0] - q[0] * v[2]), uz = 2.0 * (q[0] * v[1] - q[1] * v[0]);
    o[0] = (v[0] + q[3] * ux) + (q[1] * uz - q[2] * uy);
    o[1] = (v[1] + q[3] * uy) + (q[2] * ux - q[0] * uz);
    o[2] = (v[2] + q[3] * uz) + (q[0] * uy - q[1] * ux);
}

// Quaterniond * Quaterniond, the Hamilton product a b of two (x, y, z, w); o is neither a nor b
XFH_HD void pose_quat_mul(const double* a, const double* b, double* o) {
    o[3] = ((a[3] * b[3] - a[0] * b[0]) - a[1] * b[1]) - a[2] * b[2];
    o[0] = ((a[3] * b[0] + a[0] * b[3]) + a[1] * b[2]) - a[2] * b[1];
    o[1] = ((a[3] * b[1] + a[1] * b[3]) + a[2] * b[0]) - a[0] * b[2];
    o[2] = ((a[3] * b[2] + a[2] * b[3]) + a[0] * b[1]) - a[1] * b[0];
}

// VertexSE3Expmap::oplusImpl: SE3Quat::exp(u) * est, u = (omega, upsilon)
XFH_HD void pose_oplus(const double* u, const PosePose& est, PosePose* out) {
    const double wx = u[0], wy = u[1], wz = u[2];
    const double theta = sqrt((wx * wx + wy * wy) + wz * wz);
    const double O[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
    double O2[9], R[9], V[9];
    _Pragma("unroll")
    for (int r = 0; r < 3; ++r)
        _Pragma("unroll")
        for (int c = 0; c < 3; ++c) O2[3 * r + c] = (O[3 * r] * O[c] + O[3 * r + 1] * O[3 + c]) + O[3 * r + 2] * O[6 + c];
    if (theta < 0.00001) {
        _Pragma("unroll")
        for (int k = 0; k < 9; ++k) { R[k] = ((k % 4 == 0 ? 1.0 : 0.0) + O[k]) + O2[k]; V[k] = R[k]; }
    } else {
        const double s = sin(theta), c = cos(theta), t2 = theta * theta;
        const double a = s / theta, b = (1.0 - c) / t2, d = (theta - s) / (t2 * theta);
        _Pragma("unroll")
        for (int k = 0; k < 9; ++k) {
            const double id = k % 4 == 0 ? 1.0 : 0.0;
            R[k] = (id + a * O[k]) + b * O2[k];
            V[k] = (id + b * O[k]) + d * O2[k];
        }
    }
    PosePose e;
    pose_quat_from_matrix(R, e.q);
    _Pragma("unroll")
    for (int r = 0; r < 3; ++r) e.t[r] = (V[3 * r] * u[3] + V[3 * r + 1] * u[4]) + V[3 * r + 2] * u[5];
    pose_normalize(e.q);                                                   // SE3Quat(q, t)
    double rt[3];
    pose_rotate(e.q, est.t, rt);                                           // operator*: t = e.t + e.r * est.t;  r = e.r * est.r;  normalizeRotation
    pose_quat_mul(e.q, est.q, out->q);
    out->t[0] = e.t[0] + rt[0]; out->t[1] = e.t[1] + rt[1]; out->t[2] = e.t[2] + rt[2];
    pose_normalize(out->q);
}

// computeError + chi2 of one edge at pose P: pc = P.map(X); mono (Pinhole::project, double) e = obs - (fx*x/z + cx, fy*y/z + cy); stereo
// (cam_project: invz is a FLOAT there) e = obs - (x*invz*fx + cx, y*invz*fy + cy, u - bf*invz).  chi2 = sum e_r * (w * e_r).
XFH_HD double pose_edge_error(const PosePose& P, const PoseCam& cam, const double* X, const double* obs, bool stereo, double w, double* pc, double* e) {
    double r[3];
    pose_rotate(P.q, X, r);
    pc[0] = r[0] + P.t[0]; pc[1] = r[1] + P.t[1]; pc[2] = r[2] + P.t[2];
    if (!stereo) {
        e[0] = obs[0] - (cam.fx * pc[0] / pc[2] + cam.cx);
        e[1] = obs[1] - (cam.fy * pc[1] / pc[2] + cam.cy);
        e[2] = 0.0;
        return e[0] * (w * e[0]) + e[1] * (w * e[1]);
    }
    const double invz = (double)(float)(1.0 / pc[2]);
    const double u = pc[0] * invz * cam.fx + cam.cx;
    e[0] = obs[0] - u;
    e[1] = obs[1] - (pc[1] * invz * cam.fy + cam.cy);
    e[2] = obs[2] - (u - cam.bf * invz);
    return (e[0] * (w * e[0]) + e[1] * (w * e[1])) + e[2] * (w * e[2]);
}

// linearizeOplus at the camera-frame point pc: J is [3][6] row-major, the third row zero for a mono edge.  Mono: -projectJac(pc) * SE3deriv with the
// structural zeros of the product left out; stereo: types_six_dof_expmap.cpp:375-404.
XFH_HD void pose_edge_jacobian(const PoseCam& cam, const double* pc, bool stereo, double* J) {
    const double x = pc[0], y = pc[1], z = pc[2];
    if (!stereo) {
        const double a = cam.fx / z, c = -cam.fx * x / (z * z), b = cam.fy / z, d = -cam.fy * y / (z * z);
        J[0] = -(c * y); J[1] = -(a * z - c * x); J[2] = -(-a * y); J[3] = -a; J[4] = 0.0; J[5] = -c;
        J[6] = -(d * y - b * z); J[7] = -(-d * x); J[8] = -(b * x); J[9] = 0.0; J[10] = -b; J[11] = -d;
        _Pragma("unroll")
        for (int k = 12; k < 18; ++k) J[k] = 0.0;
        return;
    }
    const double invz = 1.0 / z, invz_2 = invz * invz;
    J[0] = x * y * invz_2 * cam.fx; J[1] = -(1.0 + (x * x * invz_2)) * cam.fx; J[2] = y * invz * cam.fx; J[3] = -invz * cam.fx; J[4] = 0.0; J[5] = x * invz_2 * cam.fx;
    J[6] = (1.0 + y * y * invz_2) * cam.fy; J[7] = -x * y * invz_2 * cam.fy; J[8] = -x * invz * cam.fy; J[9] = 0.0; J[10] = -invz * cam.fy; J[11] = y * invz_2 * cam.fy;
    J[12] = J[0] - cam.bf * y * invz_2; J[13] = J[1] + cam.bf * x * invz_2; J[14] = J[2]; J[15] = J[3]; J[16] = 0.0; J[17] = J[5] - cam.bf * invz_2;
}

// RobustKernelHuber::robustify (robust_kernel_impl.cpp:78): rho[0] and rho[1]; delta is the float the reference sets, dsqr = delta * delta in double
XFH_HD void pose_huber(double chi2, double delta, double* rho0, double* rho1) {
    const double dsqr = delta * delta;
    if (chi2 <= dsqr) { *rho0 = chi2; *rho1 = 1.0; return; }               // (a NaN chi2 takes the other branch, as there)
    const double sq = sqrt(chi2);
    *rho0 = 2.0 * sq * delta - dsqr;
    *rho1 = delta / sq;
}
XFH_HD double pose_delta(bool stereo) { return (double)(stereo ? (float)sqrt(7.815) : (float)sqrt(5.991)); }

// constructQuadraticForm of one edge added to a lane's partial sums: H += A^T (rho1 w) A (rho[2]'s term is commented out in base_edge.h:96-102),
// b -= rho1 A^T (w e); without a kernel rho1 = 1.  Each entry's share is summed over the edge's rows first and then added.
XFH_HD void pose_accumulate(double* acc, const double* J, const double* e, bool stereo, double w, double rho1) {
    const double ww = rho1 * w;
    int n = 0;
    _Pragma("unroll")
    for (int i = 0; i < 6; ++i)
        _Pragma("unroll")
        for (int j = i; j < 6; ++j, ++n) {
            double c = J[i] * (ww * J[j]) + J[6 + i] * (ww * J[6 + j]);
            if (stereo) c = c + J[12 + i] * (ww * J[12 + j]);
            acc[n] += c;
        }
    _Pragma("unroll")
    for (int i = 0; i < 6; ++i) {
        double c = J[i] * (w * e[0]) + J[6 + i] * (w * e[1]);
        if (stereo) c = c + J[12 + i] * (w * e[2]);
        acc[21 + i] -= rho1 * c;
    }
}

// ---- the four rounds of optimize(10): the Levenberg machine of geom_common.h (geo_lm_after_build / geo_lm_after_trial, the LDL^T that MLPnP's
// Gauss-Newton shares) with 6 unknowns, and around it what is PoseOptimization's own: every round starts from the input pose, CLASSIFY hands back the
// number of edges over their threshold, the Huber kernel is on in a pass iff pose_lm_robust(S).  sums: XFH_POSE_NSUM, the robust chi2 last.
enum { XFH_POSE_H_INITIAL = 0, XFH_POSE_H_BAD = 1, XFH_POSE_H_RETURN = 2, XFH_POSE_H_ROUNDS = 3, XFH_POSE_H_ITERATIONS = 4, XFH_POSE_H_TRIALS = 5,
       XFH_POSE_H_REJECTED = 6, XFH_POSE_H_LDLT_FAILURES = 7 };
struct PoseLM {
    PosePose input, est, backup;
    double H[21], b[6], x[6];
    double lambda, ni, currentChi, iniChi;
    int round, iter, qmax, nbad_lm, solved;
    int hdr[8];
    static constexpr int N = 6, H_ITERATIONS = XFH_POSE_H_ITERATIONS;
    static XFH_HD int iterations(const PoseLM&) { return XFH_POSE_ITERATIONS; }
    static XFH_HD PosePose oplus(const PoseLM& S) { PosePose n; pose_oplus(S.x, S.est, &n); return n; }
};
XFH_HD bool pose_lm_robust(const PoseLM& S) { return S.round < 3; }        // `if (it == 2) e->setRobustKernel(0)`

XFH_HD int pose_lm_round(PoseLM& S) {                                       // setEstimate(pFrame->GetPose()); initializeOptimization(0); optimize(10)
    S.est = S.input; S.iter = 0;
    return S.hdr[XFH_POSE_H_INITIAL] - S.hdr[XFH_POSE_H_BAD] > 0 ? GEO_LM_BUILD : GEO_LM_CLASSIFY;       // no level-0 edge: optimize() returns at once
}
XFH_HD int pose_lm_begin(PoseLM& S, const PosePose& input, int n_initial) {
    S.input = input; S.round = 0; S.currentChi = 0.0;
    _Pragma("unroll")
    for (int k = 0; k < 6; ++k) S.x[k] = 0.0;                               // the solver's x: a failed LDLT leaves the previous solve's there
    _Pragma("unroll")
    for (int k = 0; k < 8; ++k) S.hdr[k] = 0;
    S.hdr[XFH_POSE_H_INITIAL] = n_initial;
    return pose_lm_round(S);
}
XFH_HD int pose_lm_after_classify(PoseLM& S, int n_bad) {
    S.hdr[XFH_POSE_H_BAD] = n_bad;
    S.hdr[XFH_POSE_H_RETURN] = S.hdr[XFH_POSE_H_INITIAL] - n_bad;
    ++S.hdr[XFH_POSE_H_ROUNDS];
    if (S.hdr[XFH_POSE_H_INITIAL] < 10) return GEO_LM_DONE;                 // `if (optimizer.edges().size() < 10) break`
    if (++S.round == XFH_POSE_ROUNDS) return GEO_LM_DONE;
    return pose_lm_round(S);
}

// The names under which tests/cpp/asan_poseopt_test.cpp drives the machine.  That program is the independent statement the library is compared with
// and stays as it was written before the machine was shared, so that it holds this build without having been touched: nothing else uses these.
enum { XFH_POSE_BUILD = GEO_LM_BUILD, XFH_POSE_TRIAL = GEO_LM_TRIAL, XFH_POSE_CLASSIFY = GEO_LM_CLASSIFY, XFH_POSE_DONE = GEO_LM_DONE };
XFH_HD int pose_lm_after_build(PoseLM& S, const double* sums) { return geo_lm_after_build(S, sums); }
XFH_HD int pose_lm_after_trial(PoseLM& S, double chi) { return geo_lm_after_trial(S, chi); }
