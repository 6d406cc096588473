// asan_poseopt_test.cpp -- the host side of the pose-optimisation entry points under AddressSanitizer + UBSan, linked against the sanitizer build of
// libxfeat_hip (make -C xfeatslam_amd/csrc asan).  Host code only: nothing here runs on a GPU.
//   asan_poseopt_test                  xfh_pose_edge / _oplus / _solve / _from_tcw / _to_tcw against poseopt_math.h compiled here, over ordinary and
//                                      hostile operands (NaN, Inf, a point in the camera plane), and every argument check that returns before a HIP call
//   asan_poseopt_test in.bin out.bin   the loop of k_pose_optimize run by one thread on one problem: the same state machine, the same per-edge lines,
//                                      256 lanes' partial sums and the kernel's fold, so that tests/test_poseopt_ref.py can hold the C lines against
//                                      the Python restatement bit by bit without a GPU
// in.bin : int32 nt, nq, has_uright; float Tcw[12], cam[5] (fx fy cx cy bf), inv_sigma2; float xy[nt][2]; float uright[nt] if has_uright;
//          int32 assigned[nt]; float points[nq][3].   out.bin: float Tcw_out[12]; uint8 outlier[nt]; float chi2[nt]; int32 header[8]; double final_chi2
// Exit code 0 = clean.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "xfeat_hip.h"
#include "xfeat_hip_bench.h"
#include "poseopt_math.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "asan_poseopt_test: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

static bool same(double a, double b) { return memcmp(&a, &b, 8) == 0 || (std::isnan(a) && std::isnan(b)); }
static PoseCam cam_of(const xfh_camera& c) { return PoseCam{(double)c.fx, (double)c.fy, (double)c.cx, (double)c.cy, (double)c.bf}; }

static double fold(const std::vector<double>& lanes, int n) {              // lanes[256][28] -> entry n in the kernel's order
    double w[4];
    for (int wv = 0; wv < 4; ++wv) {
        double v[64], t[64];
        for (int l = 0; l < 64; ++l) v[l] = lanes[(size_t)(wv * 64 + l) * XFH_POSE_NSUM + n];
        for (int m = 32; m >= 1; m >>= 1) { for (int l = 0; l < 64; ++l) t[l] = v[l] + v[l ^ m]; memcpy(v, t, sizeof v); }
        w[wv] = v[0];
    }
    return ((w[0] + w[1]) + w[2]) + w[3];
}

static int run_problem(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    int h[3]; float T[12], cf[5], w32;
    CHECK(f && fread(h, 4, 3, f) == 3 && fread(T, 4, 12, f) == 12 && fread(cf, 4, 5, f) == 5 && fread(&w32, 4, 1, f) == 1);
    const int nt = h[0], nq = h[1];
    CHECK(nt >= 1 && nt <= XFH_GRID_MAX_N && nq >= 1 && nq <= XFH_GRID_MAX_N);
    std::vector<float> xy((size_t)nt * 2), ur(nt, -1.0f), pts((size_t)nq * 3);
    std::vector<int> as(nt);
    CHECK(fread(xy.data(), 4, xy.size(), f) == xy.size());
    if (h[2]) CHECK(fread(ur.data(), 4, nt, f) == (size_t)nt);
    CHECK(fread(as.data(), 4, nt, f) == (size_t)nt && fread(pts.data(), 4, pts.size(), f) == pts.size());
    fclose(f);
    const PoseCam cam = {(double)cf[0], (double)cf[1], (double)cf[2], (double)cf[3], (double)cf[4]};
    const double w = (double)w32;
    std::vector<int> st(nt, 0);
    std::vector<double> last(nt, 0.0);
    std::vector<uint8_t> outlier(nt, 0);
    std::vector<float> chi2(nt, 0.0f), To(T, T + 12);
    int n_initial = 0, hdr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double final_chi2 = 0.0;
    for (int k = 0; k < nt; ++k)
        if (as[k] >= 0 && as[k] < nq) { st[k] = 1 | (ur[k] < 0.0f ? 0 : 2); ++n_initial; }
    hdr[0] = n_initial;
    if (n_initial >= 3) {
        PoseLM S; PosePose inp;
        pose_from_tcw(T, &inp);
        int act = pose_lm_begin(S, inp, n_initial);
        std::vector<double> lanes((size_t)256 * XFH_POSE_NSUM);
        for (int pass = 0; pass < 444 && act != XFH_POSE_DONE; ++pass) {
            const PosePose P = S.est;
            const bool robust = pose_lm_robust(S);
            std::fill(lanes.begin(), lanes.end(), 0.0);
            int bad = 0;
            for (int k = 0; k < nt; ++k) {                                 // lane k % 256 meets its keypoints in rising order
                if (!(st[k] & 1)) continue;
                const bool stereo = (st[k] & 2) != 0, o = (st[k] & 4) != 0;
                if (act != XFH_POSE_CLASSIFY && o) continue;
                const float* X = &pts[(size_t)as[k] * 3];
                const double Xd[3] = {(double)X[0], (double)X[1], (double)X[2]}, od[3] = {(double)xy[2 * (size_t)k], (double)xy[2 * (size_t)k + 1], (double)ur[k]};
                double pc[3], e[3];
                if (act == XFH_POSE_CLASSIFY) {
                    const double c = o ? pose_edge_error(P, cam, Xd, od, stereo, w, pc, e) : last[k];
                    const float c32 = (float)c;
                    const bool no = c32 > (stereo ? XFH_POSE_CHI2_STEREO : XFH_POSE_CHI2_MONO);
                    st[k] = (st[k] & ~4) | (no ? 4 : 0);
                    bad += no; outlier[k] = no; chi2[k] = c32;
                    continue;
                }
                double* acc = &lanes[(size_t)(k % 256) * XFH_POSE_NSUM];
                const double c = pose_edge_error(P, cam, Xd, od, stereo, w, pc, e);
                last[k] = c;
                double r0 = c, r1 = 1.0;
                if (robust) pose_huber(c, pose_delta(stereo), &r0, &r1);
                acc[27] += r0;
                if (act == XFH_POSE_BUILD) { double J[18]; pose_edge_jacobian(cam, pc, stereo, J); pose_accumulate(acc, J, e, stereo, w, r1); }
            }
            if (act == XFH_POSE_BUILD) { double sums[XFH_POSE_NSUM]; for (int n = 0; n < XFH_POSE_NSUM; ++n) sums[n] = fold(lanes, n); act = pose_lm_after_build(S, sums); }
            else if (act == XFH_POSE_TRIAL) act = pose_lm_after_trial(S, fold(lanes, 27));
            else act = pose_lm_after_classify(S, bad);
        }
        CHECK(act == XFH_POSE_DONE);
        pose_to_tcw(S.est, To.data());
        memcpy(hdr, S.hdr, sizeof hdr);
        final_chi2 = S.currentChi;
    }
    FILE* o = fopen(out, "wb");
    CHECK(o);
    fwrite(To.data(), 4, 12, o); fwrite(outlier.data(), 1, nt, o); fwrite(chi2.data(), 4, nt, o); fwrite(hdr, 4, 8, o); fwrite(&final_chi2, 8, 1, o);
    fclose(o);
    printf("asan_poseopt_test ok (problem: %d edges, %d bad)\n", hdr[0], hdr[1]);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 3) return run_problem(argv[1], argv[2]);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    xfh_camera cam; memset(&cam, 0, sizeof cam);
    cam.fx = 517.3f; cam.fy = 516.5f; cam.cx = 318.6f; cam.cy = 255.3f; cam.bf = 40.0f;
    const PoseCam pcam = cam_of(cam);
    // the pose lines: Tcw -> pose -> Tcw, an update, hostile values
    const float Ts[3][12] = {{1, 0, 0, 0.5f, 0, 1, 0, -0.25f, 0, 0, 1, 2.0f},
                             {-1, 0, 0, 1, 0, -1, 0, 2, 0, 0, 1, 3},                  // trace < 0, largest diagonal entry last
                             {nan, 0, inf, 1, 0, 1, 0, 2, 0, 0, -inf, nan}};
    unsigned seed = 11;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (double)(seed >> 8) / 16777216.0 - 0.5; };
    long long n = 0;
    for (const auto& T : Ts) {
        double p[7], q[7]; float back[12];
        CHECK(xfh_pose_from_tcw(T, p) == XFH_OK && xfh_pose_to_tcw(p, back) == XFH_OK);
        PosePose P; pose_from_tcw(T, &P);
        for (int k = 0; k < 4; ++k) CHECK(same(p[k], P.q[k]));
        for (int k = 0; k < 3; ++k) CHECK(same(p[4 + k], P.t[k]));
        if (!std::isnan(p[0])) for (int k = 0; k < 12; ++k) CHECK(fabsf(back[k] - T[k]) < 1e-6f);
        for (int it = 0; it < 200; ++it) {
            double u[6];
            for (double& v : u) v = rnd() * (it % 4 == 0 ? 1e-6 : 1.0);
            if (it == 7) u[2] = nan;
            if (it == 9) { for (double& v : u) v = 0.0; }
            CHECK(xfh_pose_oplus(p, u, q) == XFH_OK);
            PosePose O; pose_oplus(u, P, &O);
            for (int k = 0; k < 4; ++k) CHECK(same(q[k], O.q[k]));
            for (int k = 0; k < 3; ++k) CHECK(same(q[4 + k], O.t[k]));
            if (it == 9 && !std::isnan(p[0])) for (int k = 0; k < 7; ++k) CHECK(fabs(q[k] - p[k]) < 1e-15);
            // an edge at the updated pose, mono and stereo, ordinary and hostile points
            const float pts[5][3] = {{(float)rnd(), (float)rnd(), 4.0f + (float)rnd()}, {0.1f, 0.2f, 0.0f}, {nan, 0, 1}, {inf, -inf, inf}, {1e30f, 1e30f, 1e-30f}};
            for (const auto& X : pts) for (float ur : {-1.0f, 300.0f, nan}) for (int robust : {0, 1}) {
                const float xy[2] = {320.0f + 100.0f * (float)rnd(), 240.0f};
                double e[3], c, J[18], r1;
                CHECK(xfh_pose_edge(q, &cam, X, xy, ur, 1.25f, robust, e, &c, J, &r1) == XFH_OK);
                const bool stereo = !(ur < 0.0f);
                const double Xd[3] = {(double)X[0], (double)X[1], (double)X[2]}, od[3] = {(double)xy[0], (double)xy[1], (double)ur};
                double pc[3], e2[3], J2[18], r0, r12 = 1.0;
                const double c2 = pose_edge_error(O, pcam, Xd, od, stereo, (double)1.25f, pc, e2);
                pose_edge_jacobian(pcam, pc, stereo, J2);
                if (robust) pose_huber(c2, pose_delta(stereo), &r0, &r12);
                CHECK(same(c, c2) && same(r1, r12));
                for (int k = 0; k < 3; ++k) CHECK(same(e[k], e2[k]));
                for (int k = 0; k < 18; ++k) CHECK(same(J[k], J2[k]));
                if (!stereo) { CHECK(e[2] == 0.0); for (int k = 12; k < 18; ++k) CHECK(J[k] == 0.0); }
                CHECK(xfh_pose_edge(q, &cam, X, xy, ur, 1.25f, robust, nullptr, nullptr, nullptr, nullptr) == XFH_OK);
                ++n;
            }
        }
    }
    // the solve: identity, a singular matrix without and with lambda, NaN
    {
        double H[21] = {0}, b[6] = {1, 2, 3, 4, 5, 6}, x[6] = {9, 9, 9, 9, 9, 9};
        for (int j = 0, k = 0; j < 6; k += 6 - j, ++j) H[k] = 2.0;
        CHECK(xfh_pose_solve(H, 0.0, b, x) == 1);
        for (int k = 0; k < 6; ++k) CHECK(x[k] == b[k] / 2.0);
        double Z[21] = {0};
        x[0] = 7.0;
        CHECK(xfh_pose_solve(Z, 0.0, b, x) == 0 && x[0] == 7.0);                       // a zero pivot fails and leaves x alone
        CHECK(xfh_pose_solve(Z, 0.5, b, x) == 1 && x[5] == 12.0);
        Z[3] = std::numeric_limits<double>::quiet_NaN();
        CHECK(xfh_pose_solve(Z, 0.5, b, x) == 0);
        H[20] = -3.0;
        CHECK(xfh_pose_solve(H, 1.0, b, x) == 0 && xfh_pose_solve(H, 4.0, b, x) == 1);
        CHECK(xfh_pose_solve(nullptr, 0.0, b, x) == 0);
    }
    // the argument checks that return before any HIP call
    float* f = (float*)malloc(4096); int* ip = (int*)malloc(4096); uint8_t* u8 = (uint8_t*)malloc(64); double* d = (double*)malloc(64);
    double p7[7] = {0, 0, 0, 1, 0, 0, 0};
    CHECK(xfh_pose_from_tcw(nullptr, p7) == XFH_ERR_INVALID_ARG && xfh_pose_to_tcw(p7, nullptr) == XFH_ERR_INVALID_ARG && xfh_pose_oplus(p7, nullptr, p7) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_pose_edge(p7, nullptr, f, f, -1.0f, 1.0f, 1, nullptr, nullptr, nullptr, nullptr) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_pose_optimize_device(nullptr, 1, 8, 8, f, &cam, f, nullptr, ip, f, 1.0f, f, f, u8, f, ip, d) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_pose_optimize(nullptr, 8, 8, f, &cam, f, nullptr, ip, f, 1.0f, f, u8, f, ip, d) == XFH_ERR_INVALID_ARG);
    CHECK(xfh_pose_optimize_workspace_bytes(8, 1) > 0 && xfh_pose_optimize_workspace_bytes(8, 3) == 3 * xfh_pose_optimize_workspace_bytes(8, 1));
    for (int bad : {0, -1, XFH_GRID_MAX_N + 1}) CHECK(xfh_pose_optimize_workspace_bytes(bad, 1) == 0);
    CHECK(xfh_pose_optimize_workspace_bytes(8, 0) == 0 && xfh_pose_optimize_workspace_bytes(8, 65536) == 0);
    CHECK(strcmp(xfh_kernel_name(XFH_K_POSE_OPTIMIZE), "k_pose_optimize") == 0 && XFH_K_POSE_OPTIMIZE == 35 && XFH_K_BOWDB_SELECT == 34);
    free(f); free(ip); free(u8); free(d);
    printf("asan_poseopt_test ok (%lld edges)\n", n);
    return 0;
}
