// asan_local_ba_test.cpp -- lba_math.h alone under AddressSanitizer + UBSan (tests/test_local_ba_ref.py::test_lba_math_under_sanitizers builds and runs it):
// a stand-alone program, nothing of the library linked, nothing on a GPU, nothing loaded into Python.
//   1. The two Levenberg machines: geo_lm_* of geom_common.h (PoseLM, the dense 6 x 6 form in one lane) and the distributed restatement (LbaCtl) driven with
//      the same H, b and the same sequence of chi2 values -- improvements, regressions, equal values, NaN, Inf, failed factorisations -- every field compared
//      after every step.
//   2. The stale-error rule with a FORCED rejected last trial: the chi2 the decision sees is replaced by a NaN, the trial is rejected, and the chi2 every
//      edge reports must be, bit for bit, its error at the REJECTED estimate (computed here edge by edge), while the flag's depth is that of the restored one.
//   3. Problem files written by the test (argv[1..]): the whole rule (lba_host_run) in buffers of EXACT size.  A file that carries expected outputs (the
//      Python rule's, tests/ref_local_ba.py) is compared byte for byte; a NaN or hostile one must terminate with the plan's counts.
#include "lba_math.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)
static bool same(double a, double b) { return memcmp(&a, &b, 8) == 0 || (a != a && b != b); }

// ---- 1. the two machines --------------------------------------------------------------------------------------------------------------------------------
static unsigned long long rng_state = 88172645463325252ull;
static double rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (double)(rng_state >> 11) / 9007199254740992.0; }

static void machines(int seed) {
    rng_state += (unsigned long long)seed * 0x9E3779B97F4A7C15ull;
    PoseLM G;
    const PosePose id{{0.0, 0.0, 0.0, 1.0}, {0.0, 0.0, 0.0}};
    int act = pose_lm_begin(G, id, 100);
    CHECK(act == GEO_LM_BUILD);
    LbaCtl L = {};
    L.ni = 2.0; L.act = LBA_BUILD; L.max_it = XFH_POSE_ITERATIONS;
    double x[6] = {0, 0, 0, 0, 0, 0}, b[6], chi = 100.0 + 50.0 * rnd();
    for (int step = 0; step < 200 && act != GEO_LM_CLASSIFY; ++step) {
        if (act == GEO_LM_BUILD) {
            double sums[XFH_POSE_NSUM] = {};
            const bool bad_H = rnd() < 0.15;                                 // a diagonal that fails the factorisation
            double m = 0.0;
            for (int j = 0, n = 0; j < 6; n += 6 - j, ++j) { sums[n] = bad_H && j == 3 ? -1.0 : 1.0 + 10.0 * rnd(); const double a = fabs(sums[n]); m = (a < m) ? m : a; }
            for (int j = 0; j < 6; ++j) { sums[21 + j] = b[j] = rnd() - 0.5; }
            sums[27] = chi;
            act = geo_lm_after_build(G, sums);
            lba_lm_after_build(L, chi, m);
        } else {
            const double r = rnd();                                          // the next chi2: better, worse, equal, NaN, Inf
            const double next = r < 0.45 ? chi * (0.5 + 0.5 * rnd()) : r < 0.75 ? chi * (1.0 + rnd()) : r < 0.85 ? G.currentChi : r < 0.9 ? NAN : r < 0.93 ? INFINITY : chi * 0.9999999;
            // the distributed side: the same solve, the scale summed in index order
            const int solved = geo_ldlt_solve<6>(G.H, L.lambda, b, x) ? 1 : 0;
            CHECK(solved == G.solved && same(L.lambda, G.lambda));
            for (int j = 0; j < 6; ++j) CHECK(same(x[j], G.x[j]));
            double scale = 0.0;
            for (int j = 0; j < 6; ++j) scale += x[j] * (L.lambda * x[j] + b[j]);
            L.solved = solved;
            const int cur = L.cur;
            lba_lm_after_trial(L, next, scale);
            act = geo_lm_after_trial(G, next);
            const bool accepted = L.cur != cur;
            if (accepted && next == next) chi = next;
        }
        const int more = act == GEO_LM_TRIAL ? 1 : 0;                        // geo_lm_trial has already counted the trial it started
        CHECK(same(L.lambda, G.lambda) && same(L.ni, G.ni) && same(L.currentChi, G.currentChi) && same(L.iniChi, G.iniChi));
        CHECK(L.iter == G.iter || act == GEO_LM_CLASSIFY);
        CHECK(L.qmax == G.qmax && L.nbad_lm == G.nbad_lm);
        CHECK(L.hdr[LBA_H_ITERATIONS] == G.hdr[XFH_POSE_H_ITERATIONS] && L.hdr[LBA_H_TRIALS] == G.hdr[XFH_POSE_H_TRIALS] - more);
        CHECK(L.hdr[LBA_H_REJECTED] == G.hdr[XFH_POSE_H_REJECTED]);
        CHECK(L.hdr[LBA_H_LDLT_FAILURES] == G.hdr[XFH_POSE_H_LDLT_FAILURES] - (more && !G.solved ? 1 : 0));
        CHECK((L.act == LBA_BUILD) == (act == GEO_LM_BUILD) && (L.act == LBA_TRIAL) == (act == GEO_LM_TRIAL) && (L.act == LBA_DONE) == (act == GEO_LM_CLASSIFY));
    }
    CHECK(act == GEO_LM_CLASSIFY && L.act == LBA_DONE);
}

// ---- problems -------------------------------------------------------------------------------------------------------------------------------------------
struct Problem {
    int nK, n_free, nP, nE, pose_rows, point_rows, max_it, write_back, has_expected;
    float cam[5], inv_sigma2;
    float *pose_table, *point_table, *edge_obs; int *kf_row, *point_row, *edge_begin, *edge_kf; unsigned char* kf_fixed;
    float *Tcw_out, *points_out, *chi2; unsigned char* erase; int* header; double* final_chi2; char* ws;
    std::vector<void*> owned;
    template <class T> T* take(size_t n) { T* p = (T*)malloc(n * sizeof(T) ? n * sizeof(T) : 1); CHECK(p); owned.push_back(p); return p; }   // exact size: one byte past is ASan's
    void alloc() {
        pose_table = take<float>(12 * (size_t)pose_rows); point_table = take<float>(3 * (size_t)point_rows); kf_row = take<int>(nK); kf_fixed = take<unsigned char>(nK);
        point_row = take<int>(nP); edge_begin = take<int>(nP + 1); edge_kf = take<int>(nE); edge_obs = take<float>(3 * (size_t)nE);
        Tcw_out = take<float>(12 * (size_t)nK); points_out = take<float>(3 * (size_t)nP); erase = take<unsigned char>(nE); chi2 = take<float>(nE);
        header = take<int>(XFH_LBA_HDR_INTS); final_chi2 = take<double>(1);
        const size_t wsb = lba_ws(nullptr, nK, nP, nE, n_free).bytes;
        ws = take<char>(wsb);
        memset(ws, 0x3C, wsb);
    }
    LbaArgs args() const {
        LbaArgs a = {};
        a.nK = nK; a.nP = nP; a.nE = nE; a.n_free = n_free; a.pose_rows = pose_rows; a.point_rows = point_rows; a.max_it = max_it; a.write_back = write_back;
        a.pose_table = pose_table; a.point_table = point_table; a.kf_row = kf_row; a.kf_fixed = kf_fixed; a.point_row = point_row; a.edge_begin = edge_begin;
        a.edge_kf = edge_kf; a.edge_obs = edge_obs; a.cam = PoseCam{(double)cam[0], (double)cam[1], (double)cam[2], (double)cam[3], (double)cam[4]};
        a.w = (double)inv_sigma2; a.Tcw_out = Tcw_out; a.points_out = points_out; a.erase = erase; a.chi2 = chi2; a.header = header; a.final_chi2 = final_chi2; a.ws = ws;
        return a;
    }
    ~Problem() { for (void* p : owned) free(p); }
};
static void rd(FILE* f, void* p, size_t n) { CHECK(fread(p, 1, n, f) == n); }

// the file: 9 ints, 6 floats, the eight input arrays, then (has_expected) Tcw_out, points_out, erase, chi2, header, final_chi2, else 5 ints: header[0 .. 4]
static void run_file(const char* path) {
    FILE* f = fopen(path, "rb");
    CHECK(f);
    Problem P;
    int hd[9];
    rd(f, hd, sizeof hd);
    P.nK = hd[0]; P.n_free = hd[1]; P.nP = hd[2]; P.nE = hd[3]; P.pose_rows = hd[4]; P.point_rows = hd[5]; P.max_it = hd[6]; P.write_back = hd[7]; P.has_expected = hd[8];
    float fl[6];
    rd(f, fl, sizeof fl);
    memcpy(P.cam, fl, 20); P.inv_sigma2 = fl[5];
    P.alloc();
    rd(f, P.pose_table, 48 * (size_t)P.pose_rows); rd(f, P.point_table, 12 * (size_t)P.point_rows); rd(f, P.kf_row, 4 * (size_t)P.nK); rd(f, P.kf_fixed, P.nK);
    rd(f, P.point_row, 4 * (size_t)P.nP); rd(f, P.edge_begin, 4 * (size_t)(P.nP + 1)); rd(f, P.edge_kf, 4 * (size_t)P.nE); rd(f, P.edge_obs, 12 * (size_t)P.nE);
    lba_host_run(P.args());
    if (P.has_expected) {
        std::vector<char> e(48 * (size_t)P.nK + 12 * (size_t)P.nP + 5 * (size_t)P.nE + 4 * XFH_LBA_HDR_INTS + 8);
        rd(f, e.data(), e.size());
        const char* q = e.data();
        CHECK(memcmp(q, P.Tcw_out, 48 * (size_t)P.nK) == 0); q += 48 * (size_t)P.nK;
        CHECK(memcmp(q, P.points_out, 12 * (size_t)P.nP) == 0); q += 12 * (size_t)P.nP;
        CHECK(memcmp(q, P.erase, P.nE) == 0); q += P.nE;
        CHECK(memcmp(q, P.chi2, 4 * (size_t)P.nE) == 0); q += 4 * (size_t)P.nE;
        CHECK(memcmp(q, P.header, 4 * XFH_LBA_HDR_INTS) == 0); q += 4 * XFH_LBA_HDR_INTS;
        CHECK(memcmp(q, P.final_chi2, 8) == 0);
    } else {
        int want[5];
        rd(f, want, sizeof want);
        for (int k = 1; k < 5; ++k) CHECK(P.header[k] == want[k]);
        CHECK(P.header[LBA_H_ITERATIONS] <= P.max_it && P.header[LBA_H_TRIALS] <= 10 * P.max_it && P.header[LBA_H_ERASE] <= P.nE);
    }
    fclose(f);
}

// ---- 2. the stale-error rule -------------------------------------------------------------------------------------------------------------------------------
static int g_force_trial;
static double force_nan(int trial, double chi) { return trial == g_force_trial ? NAN : chi; }

static void stale_errors() {
    // two fixed keyframes and one free one on a baseline, 24 points in front of them, every point seen by all three, stereo and mono in turn
    Problem P;
    P.nK = 3; P.n_free = 1; P.nP = 24; P.nE = 72; P.pose_rows = 3; P.point_rows = 24; P.max_it = 2; P.write_back = 0;
    const float cam[5] = {500.f, 500.f, 320.f, 240.f, 40.f};
    memcpy(P.cam, cam, 20); P.inv_sigma2 = 1.f;
    P.alloc();
    for (int k = 0; k < 3; ++k) {
        const float T[12] = {1, 0, 0, -0.3f * k, 0, 1, 0, 0, 0, 0, 1, 0};
        memcpy(P.pose_table + 12 * k, T, 48);
        P.kf_row[k] = k; P.kf_fixed[k] = k == 1 ? 0 : 1;
    }
    P.edge_begin[0] = 0;
    for (int p = 0; p < 24; ++p) {
        const float X[3] = {-1.f + 0.13f * p, -0.5f + 0.04f * p, 4.f + 0.1f * (p % 7)};
        memcpy(P.point_table + 3 * p, X, 12);
        P.point_row[p] = p;
        for (int k = 0; k < 3; ++k) {
            const int e = 3 * p + k;
            const float x = X[0] - 0.3f * k, u = 500.f * x / X[2] + 320.f, v = 500.f * X[1] / X[2] + 240.f;
            P.edge_kf[e] = k;
            P.edge_obs[3 * e] = u + 0.7f * ((e * 7) % 5 - 2); P.edge_obs[3 * e + 1] = v - 0.6f * ((e * 3) % 5 - 2); P.edge_obs[3 * e + 2] = (e & 1) ? u - 40.f / X[2] : -1.f;
        }
        P.edge_begin[p + 1] = 3 * (p + 1);
    }
    P.pose_table[12 + 3] += 0.02f;                                          // the free keyframe starts off its place
    const LbaArgs a = P.args();
    lba_host_run(a);                                                         // unforced: which trial is the last one
    CHECK(P.header[LBA_H_STATUS] == LBA_OK && P.header[LBA_H_TRIALS] >= 1);
    g_force_trial = P.header[LBA_H_TRIALS] - 1;
    const int rejected_before = P.header[LBA_H_REJECTED];
    lba_host_run(a, force_nan);
    // a NaN rho ends the trials with the estimate restored: the forced trial was the last one
    CHECK(P.header[LBA_H_TRIALS] == g_force_trial + 1 && P.header[LBA_H_REJECTED] >= 1 && P.header[LBA_H_REJECTED] <= rejected_before + 1);
    const LbaWs w = lba_ws(a.ws, a.nK, a.nP, a.nE, a.n_free);
    const int cur = w.ctl->cur;
    int differ = 0;
    for (int e = 0; e < P.nE; ++e) {
        const int p = e / 3, k = P.edge_kf[e];
        double obs[3], pc[3], er[3];
        lba_obs(a, e, obs);
        const double* Xr = w.pt + 3 * ((size_t)(1 - cur) * a.nP + p);       // the REJECTED estimate lives in the buffer that was not taken
        const double* Xc = w.pt + 3 * ((size_t)cur * a.nP + p);
        const double c_rej = pose_edge_error(lba_pose_get(w.pose + 8 * ((size_t)(1 - cur) * a.nK + k)), a.cam, Xr, obs, lba_stereo(a, e), a.w, pc, er);
        const double c_cur = pose_edge_error(lba_pose_get(w.pose + 8 * ((size_t)cur * a.nK + k)), a.cam, Xc, obs, lba_stereo(a, e), a.w, pc, er);
        const float want = (float)c_rej;
        CHECK(memcmp(&want, &P.chi2[e], 4) == 0);
        differ += (float)c_cur != want ? 1 : 0;
        const int flag = (c_rej > (lba_stereo(a, e) ? 7.815 : 5.991) || !(pc[2] > 0.0)) ? 1 : 0;     // pc: at the restored estimate
        CHECK(flag == P.erase[e]);
    }
    CHECK(differ > P.nE / 2);                                                // the two estimates are different ones: the test could tell
}

int main(int argc, char** argv) {
    for (int s = 0; s < 200; ++s) machines(s);
    stale_errors();
    for (int i = 1; i < argc; ++i) run_file(argv[i]);
    printf("asan_local_ba_test ok (%d files)\n", argc - 1);
    return 0;
}
