// asan_optsim3_test.cpp -- optsim3_math.h alone under AddressSanitizer + UBSan: a stand-alone program, nothing of the library is linked and nothing
// runs on a GPU.  It runs the loop of k_sim3_optimize on ONE host thread the way the kernel's register instance lays it out -- 256 lanes that each own
// EPT slots with the pair, its state word and its two stored chi2 in per-lane arrays, lanes 0 .. 14 building the similarities of a pass, per-lane
// partial sums, the xor butterfly inside each wave of 64 and the four waves in order, lane 0 driving the state machine -- over good, NaN and hostile
// problems, and compares every output byte for byte with the host form os3_host_problem (the workspace layout).  Every buffer is a std::vector of its
// exact size, so a load or store outside a named buffer is an AddressSanitizer report.  Exit code 0 and "asan_optsim3_test ok" = clean.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "optsim3_math.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "asan_optsim3_test: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

static uint64_t g_rng = 88172645463325252ull;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 16); }
static double uni(double a, double b) { return a + (b - a) * (rnd() / 4294967296.0); }

struct Problem {
    int B, n1, M1, nq, n2, shared, fix_scale, all_points, with_tmw;
    std::vector<float> T1w, xy1, points1, points2, xy2, T2w, S12, Tmw;
    std::vector<int> point1, assigned, index2;
    std::vector<unsigned char> flags2;
};
struct Outputs {
    std::vector<int> assigned_out, header; std::vector<unsigned char> status; std::vector<float> chi2, S12_out, Tcw, Ow; std::vector<double> state, final_chi2;
    std::vector<char> ws;
    Outputs(const Problem& p) : assigned_out((size_t)p.B * p.n1, 77), header((size_t)p.B * 16, 77), status((size_t)p.B * p.n1, 77), chi2((size_t)p.B * p.n1 * 2, 77.0f),
                                S12_out((size_t)p.B * 13, 77.0f), Tcw((size_t)p.B * 12, 77.0f), Ow((size_t)p.B * 3, 77.0f), state((size_t)p.B * 8, 77.0),
                                final_chi2(p.B, 77.0), ws(os3_ws_bytes(p.n1) * (size_t)p.B + 16, 0x3C) {}
};

static Os3Args args_of(const Problem& p, Outputs& o) {
    Os3Args a = {};
    a.n1 = p.n1; a.M1 = p.M1; a.nq = p.nq; a.n2 = p.n2; a.side1_shared = p.shared; a.fix_scale = p.fix_scale; a.all_points = p.all_points;
    a.T1w = p.T1w.data(); a.xy_un1 = p.xy1.data(); a.points1 = p.points1.data(); a.point1 = p.point1.data(); a.assigned = p.assigned.data();
    a.points2 = p.points2.data(); a.flags2 = p.flags2.data(); a.index2 = p.index2.data(); a.xy_un2 = p.xy2.data(); a.T2w = p.T2w.data();
    a.S12 = p.S12.data(); a.S12_stride = 13; a.Tmw = p.with_tmw ? p.Tmw.data() : nullptr;
    a.cam1 = Os3Cam{517.3, 516.5, 318.6, 255.3}; a.cam2 = Os3Cam{520.9, 521.0, 325.1, 249.7};
    a.th2 = 10.0; a.w1 = 1.0; a.w2 = (double)0.69444f; a.delta = (double)sqrtf(10.0f);
    a.ws = o.ws.data() + ((16 - (uintptr_t)o.ws.data() % 16) % 16); a.ws_stride = os3_ws_bytes(p.n1);
    a.assigned_out = o.assigned_out.data(); a.status = o.status.data(); a.chi2 = o.chi2.data(); a.state = o.state.data(); a.S12_out = o.S12_out.data();
    a.S12_out_stride = 13; a.Tcw = o.Tcw.data(); a.Ow = o.Ow.data(); a.header = o.header.data(); a.final_chi2 = o.final_chi2.data();
    return a;
}

// a forced rejection: round 1 is cut to optimize(2) and the chi2 sum of the first trial of its second iteration -- a full Levenberg step far from
// convergence -- is replaced by a NaN, so that rho is a NaN, the trial is rejected and popped whatever its merit, no further trial follows (rho < 0
// is false) and the classification comes next
struct Forced { bool done = false; Os3Sim rejected, restored; };

// the kernel's loop for problem pb, register instance: lane l, slot j <-> keypoint l + 256 j
static void lanes_problem(const Os3Args& a, int pb, Forced* forced = nullptr) {
    const int EPT = (a.n1 + XFH_OS3_THREADS - 1) / XFH_OS3_THREADS;
    std::vector<Os3Pair> P((size_t)XFH_OS3_THREADS * EPT);
    std::vector<double> l12(P.size(), 0.0), l21(P.size(), 0.0);
    std::vector<int> st(P.size(), 0);
    int cnt[4] = {0, 0, 0, 0};
    for (int tid = 0; tid < XFH_OS3_THREADS; ++tid)
        for (int j = 0; j < EPT; ++j) {
            const int k = tid + j * XFH_OS3_THREADS;
            const size_t s = (size_t)tid * EPT + j;
            P[s] = Os3Pair{};
            if (k < a.n1) st[s] = os3_pair_load(a, pb, k, &P[s]);
            cnt[tid >> 6] += st[s] ? ((st[s] & OS3_IN_KF2) ? 1 : 65537) : 0;
        }
    Os3LM S;
    Os3Sims sims;
    Os3Sim in;
    os3_from_floats(a.S12 + (size_t)pb * a.S12_stride, &in);
    const int n = ((cnt[0] + cnt[1]) + cnt[2]) + cnt[3];
    int act = os3_lm_begin(S, in, a.fix_scale, n & 0xFFFF, n >> 16);
    std::vector<double> acc((size_t)XFH_OS3_THREADS * XFH_OS3_NSUM);
    for (int pass = 0; pass <= XFH_OS3_MAX_PASSES; ++pass) {
        if (act == XFH_OS3_DONE) break;
        for (int tid = 0; tid < 15; ++tid)
            if (tid == 14 || act == XFH_OS3_BUILD) os3_sims_piece(S.est, a.fix_scale, tid, &sims);
        const bool robust = os3_lm_robust(S), final = os3_lm_final(S);
        int bad[4] = {0, 0, 0, 0};
        for (int tid = 0; tid < XFH_OS3_THREADS; ++tid) {
            double* mine = &acc[(size_t)tid * XFH_OS3_NSUM];
            for (int k = 0; k < XFH_OS3_NSUM; ++k) mine[k] = 0.0;
            for (int j = 0; j < EPT; ++j) {
                const size_t s = (size_t)tid * EPT + j;
                if (st[s] & OS3_EDGE) os3_pair_pass(act, robust, final, sims, a, P[s], st[s], l12[s], l21[s], mine, bad[tid >> 6]);
            }
        }
        auto fold = [&](int k) {
            double w[4];
            for (int wv = 0; wv < 4; ++wv) {
                double v[64], t[64];
                for (int l = 0; l < 64; ++l) v[l] = acc[(size_t)(wv * 64 + l) * XFH_OS3_NSUM + k];
                for (int m = 32; m >= 1; m >>= 1) { for (int l = 0; l < 64; ++l) t[l] = v[l] + v[l ^ m]; memcpy(v, t, sizeof v); }
                w[wv] = v[0];
            }
            return ((w[0] + w[1]) + w[2]) + w[3];
        };
        if (act == XFH_OS3_BUILD) {
            double sums[XFH_OS3_NSUM];
            for (int k = 0; k < XFH_OS3_NSUM; ++k) sums[k] = fold(k);
            act = os3_lm_after_build(S, sums);
        } else if (act == XFH_OS3_TRIAL && forced && !forced->done && S.round == 0 && S.iter == 1) {
            S.iters = 2;
            forced->rejected = S.est;
            act = os3_lm_after_trial(S, std::numeric_limits<double>::quiet_NaN());
            forced->restored = S.est;
            forced->done = act == XFH_OS3_CLASSIFY;
        } else if (act == XFH_OS3_TRIAL) act = os3_lm_after_trial(S, fold(35));
        else act = os3_lm_after_classify(S, ((bad[0] + bad[1]) + bad[2]) + bad[3]);
    }
    for (int tid = 0; tid < XFH_OS3_THREADS; ++tid)
        for (int j = 0; j < EPT; ++j) {
            const int k = tid + j * XFH_OS3_THREADS;
            const size_t s = (size_t)tid * EPT + j;
            if (k < a.n1) os3_pair_store(a, pb, k, st[s], l12[s], l21[s]);
        }
    os3_finish(a, pb, S);
}

static void rotation(double rx, double ry, double rz, double* R) {
    const double u[7] = {rx, ry, rz, 0, 0, 0, 0};
    Os3Sim e;
    os3_exp(u, &e);
    pose_matrix_from_quat(e.q, R);
}
static void pose(float* T, double rot, double tr) {
    double R[9];
    rotation(uni(-rot, rot), uni(-rot, rot), uni(-rot, rot), R);
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) T[4 * r + c] = (float)R[3 * r + c]; T[4 * r + 3] = (float)uni(-tr, tr); }
}

// good: B problems of two keyframes seeing n_pairs common points through a known similarity, a perturbed start, some outliers and points not in KF2
static Problem good(int B, int n1, int n_pairs, int shared, int fix_scale, int all_points, int with_tmw) {
    Problem p{B, n1, n_pairs + 3, n_pairs + 5, n_pairs + 4, shared, fix_scale, all_points, with_tmw};
    const int S1 = shared ? 1 : B;
    p.T1w.resize((size_t)S1 * 12); p.xy1.assign((size_t)S1 * n1 * 2, 100.0f); p.points1.assign((size_t)S1 * p.M1 * 3, 1.0f); p.point1.assign((size_t)S1 * n1, -1);
    p.assigned.assign((size_t)B * n1, -1); p.points2.assign((size_t)B * p.nq * 3, 1.0f); p.flags2.assign((size_t)B * p.nq, 1); p.index2.assign((size_t)B * p.nq, -1);
    p.xy2.assign((size_t)B * p.n2 * 2, 50.0f); p.T2w.resize((size_t)B * 12); p.S12.resize((size_t)B * 13); p.Tmw.resize((size_t)B * 12);
    for (int s = 0; s < S1; ++s) pose(&p.T1w[(size_t)s * 12], 0.3, 1.0);
    std::vector<double> P1c((size_t)S1 * n_pairs * 3);                       // the camera-1 points are side 1's: drawn once per side-1 block
    for (int b = 0; b < B; ++b) {
        pose(&p.T2w[(size_t)b * 12], 0.3, 1.0); pose(&p.Tmw[(size_t)b * 12], 0.3, 1.0);
        const double u0[7] = {uni(-0.1, 0.1), uni(-0.1, 0.1), uni(-0.1, 0.1), uni(-0.3, 0.3), uni(-0.3, 0.3), uni(-0.3, 0.3), fix_scale ? 0.0 : uni(-0.1, 0.1)};
        Os3Sim truth, inv, start;
        os3_exp(u0, &truth);
        os3_inverse(truth, &inv);
        const double du[7] = {uni(-0.01, 0.01), uni(-0.01, 0.01), uni(-0.01, 0.01), uni(-0.03, 0.03), uni(-0.03, 0.03), uni(-0.03, 0.03), uni(-0.02, 0.02)};
        os3_oplus(du, truth, fix_scale, &start);
        os3_to_floats(start, &p.S12[(size_t)b * 13]);
        const float* T1 = &p.T1w[(size_t)(shared ? 0 : b) * 12];
        const float* T2 = &p.T2w[(size_t)b * 12];
        for (int j = 0; j < n_pairs; ++j) {
            const size_t s1 = (size_t)(shared ? 0 : b);
            double* X1 = &P1c[(s1 * n_pairs + j) * 3];
            double X2[3];
            if (b == 0 || !shared) { const double z = uni(2.5, 9.0); X1[0] = uni(-0.35, 0.35) * z; X1[1] = uni(-0.25, 0.25) * z; X1[2] = z; }
            os3_map(inv, X1, X2);
            const int k = (int)(((long long)j * n1) / n_pairs);             // keypoint of pair j: spread over 0 .. n1 - 1, the first and (nearly) the last
            const int kk = j == n_pairs - 1 ? n1 - 1 : k;
            for (int r = 0; r < 3; ++r) {                                    // world = R^T (Xc - t)
                p.points1[(s1 * p.M1 + j) * 3 + r] = (float)((T1[r] * (X1[0] - T1[3]) + T1[4 + r] * (X1[1] - T1[7])) + T1[8 + r] * (X1[2] - T1[11]));
                p.points2[((size_t)b * p.nq + j) * 3 + r] = (float)((T2[r] * (X2[0] - T2[3]) + T2[4 + r] * (X2[1] - T2[7])) + T2[8 + r] * (X2[2] - T2[11]));
            }
            p.point1[s1 * n1 + kk] = j; p.assigned[(size_t)b * n1 + kk] = j;
            const bool in2 = j % 7 != 3;
            p.index2[(size_t)b * p.nq + j] = in2 ? j : -1;
            const double out = j % 5 == 4 ? 40.0 : 0.0;                      // every fifth pair is a gross outlier in image 2
            p.xy1[(s1 * n1 + kk) * 2] = (float)(517.3 * X1[0] / X1[2] + 318.6 + uni(-0.7, 0.7));
            p.xy1[(s1 * n1 + kk) * 2 + 1] = (float)(516.5 * X1[1] / X1[2] + 255.3 + uni(-0.7, 0.7));
            p.xy2[((size_t)b * p.n2 + j) * 2] = (float)(520.9 * X2[0] / X2[2] + 325.1 + uni(-0.7, 0.7) + out);
            p.xy2[((size_t)b * p.n2 + j) * 2 + 1] = (float)(521.0 * X2[1] / X2[2] + 249.7 + uni(-0.7, 0.7));
        }
    }
    return p;
}

static float hostile_float() {
    switch (rnd() % 8) {
        case 0: return std::numeric_limits<float>::quiet_NaN();
        case 1: return std::numeric_limits<float>::infinity();
        case 2: return -std::numeric_limits<float>::infinity();
        case 3: return 0.0f;
        case 4: return 3.0e38f;
        case 5: return -1.0e-38f;
        default: return (float)uni(-1000.0, 1000.0);
    }
}
static int hostile_int(int n) {
    switch (rnd() % 6) {
        case 0: return std::numeric_limits<int>::min();
        case 1: return std::numeric_limits<int>::max();
        case 2: return -1;
        case 3: return n;
        default: return (int)(rnd() % (unsigned)n);
    }
}
// hostile: every array holds anything; `level` 0 leaves the geometry good and spoils the index arrays only, 1 spoils a share of the floats too, 2 everything
static void spoil(Problem& p, int level) {
    for (auto& v : p.assigned) if (rnd() % 3 == 0) v = hostile_int(p.nq);
    for (auto& v : p.point1) if (rnd() % 3 == 0) v = hostile_int(p.M1);
    for (auto& v : p.index2) if (rnd() % 3 == 0) v = hostile_int(p.n2);
    for (auto& v : p.flags2) if (rnd() % 3 == 0) v = (unsigned char)rnd();
    if (level == 0) return;
    const unsigned every = level == 1 ? 16 : 1;
    for (std::vector<float>* a : {&p.T1w, &p.xy1, &p.points1, &p.points2, &p.xy2, &p.T2w, &p.S12, &p.Tmw})
        for (auto& v : *a) if (rnd() % every == 0) v = hostile_float();
}

static bool same_bytes(const void* a, const void* b, size_t n) { return memcmp(a, b, n) == 0; }
template <class T> static bool same_vec(const std::vector<T>& a, const std::vector<T>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i) {
        if (same_bytes(&a[i], &b[i], sizeof(T))) continue;
        if ((double)a[i] != (double)a[i] && (double)b[i] != (double)b[i]) continue;   // two NaNs: the sign of a NaN out of 0 * Inf is the compiler's
        return false;
    }
    return true;
}

static int compare(const Problem& p, const char* tag, bool expect_work) {
    Outputs h(p), l(p);
    const Os3Args ah = args_of(p, h), al = args_of(p, l);
    for (int b = 0; b < p.B; ++b) { os3_host_problem(ah, b); lanes_problem(al, b); }
    const bool same = same_vec(h.assigned_out, l.assigned_out) && same_vec(h.status, l.status) && same_vec(h.chi2, l.chi2) && same_vec(h.state, l.state) &&
                      same_vec(h.S12_out, l.S12_out) && same_vec(h.header, l.header) && same_vec(h.final_chi2, l.final_chi2) &&
                      (!p.with_tmw || (same_vec(h.Tcw, l.Tcw) && same_vec(h.Ow, l.Ow)));
    if (!same) { fprintf(stderr, "asan_optsim3_test: %s: the lanes and the host form differ\n", tag); return 1; }
    for (int b = 0; b < p.B; ++b) {
        const int* hd = &h.header[(size_t)b * 16];
        CHECK(hd[8] >= 0 && hd[8] <= 15 && hd[9] >= hd[8] && hd[9] <= 150 && hd[10] <= hd[9] && hd[11] <= hd[9] && hd[12] == 0 && hd[15] == 0);
        CHECK(hd[0] >= 0 && hd[0] <= p.n1 && hd[1] + hd[2] == hd[0] && hd[3] <= hd[0] && hd[6] <= hd[0] - hd[3] && (hd[7] == 1 || hd[7] == 2));
        if (expect_work) CHECK(hd[0] >= 10 && hd[7] == 2 && hd[6] >= 10 && hd[3] > 0);
        for (int i = 0; i < p.n1; ++i) CHECK(h.status[(size_t)b * p.n1 + i] <= XFH_OS3_INLIER);
    }
    if (!p.with_tmw) CHECK(h.Tcw[0] == 77.0f && h.Ow[0] == 77.0f);         // not written without Tmw
    return 0;
}

// the stale-error rule with a forced rejected last trial: classification 1 reads _error as the last computeActiveErrors() left it, that is at the
// REJECTED estimate.  The answers are written out here from the rejected estimate itself, edge by edge.
static int stale_case() {
    Problem p = good(1, 40, 30, 0, 0, 0, 0);
    Outputs o(p);
    const Os3Args a = args_of(p, o);
    Forced f;
    lanes_problem(a, 0, &f);
    CHECK(f.done);                                                           // round 1 ended on the forced rejection
    CHECK(memcmp(&f.rejected, &f.restored, sizeof(Os3Sim)) != 0 && o.header[10] >= 1);
    Os3Sim inv_rej, inv_res;
    os3_inverse(f.rejected, &inv_rej); os3_inverse(f.restored, &inv_res);
    int bad = 0, differ = 0;
    for (int i = 0; i < p.n1; ++i) {
        if (o.status[i] != XFH_OS3_BAD_FIRST) continue;                      // (a survivor's chi2 is overwritten by the final classification)
        ++bad;
        Os3Pair pr;
        CHECK(os3_pair_load(a, 0, i, &pr) & OS3_EDGE);
        const double X1[3] = {pr.P1[0], pr.P1[1], pr.P1[2]}, X2[3] = {pr.P2[0], pr.P2[1], pr.P2[2]}, o1[2] = {pr.o1[0], pr.o1[1]}, o2[2] = {pr.o2[0], pr.o2[1]};
        double e[2];
        const float s12 = (float)os3_edge_error(f.rejected, a.cam1, X2, o1, a.w1, e), s21 = (float)os3_edge_error(inv_rej, a.cam2, X1, o2, a.w2, e);
        const float r12 = (float)os3_edge_error(f.restored, a.cam1, X2, o1, a.w1, e), r21 = (float)os3_edge_error(inv_res, a.cam2, X1, o2, a.w2, e);
        CHECK(same_bytes(&o.chi2[2 * i], &s12, 4) && same_bytes(&o.chi2[2 * i + 1], &s21, 4));      // the stale values, not the fresh ones
        CHECK(s12 > 10.0f || s21 > 10.0f);
        differ += (!same_bytes(&s12, &r12, 4) || !same_bytes(&s21, &r21, 4)) ? 1 : 0;
        CHECK(o.assigned_out[i] == -1);
    }
    CHECK(bad >= 5 && bad == o.header[3] && differ == bad);                  // the gross outliers at least; a full step moves every chi2
    return 0;
}

int main() {
    if (stale_case()) return 1;
    int n = 0;
    for (int n1 : {1, 40, 255, 256, 257, 700, 1024}) {
        for (int v = 0; v < 4; ++v) {
            const int pairs = n1 < 30 ? 1 : (n1 < 100 ? 30 : 60);
            Problem p = good(v == 3 ? 3 : 1, n1, pairs, v == 3, v & 1, v >> 1 & 1, v != 2);
            if (compare(p, "good", n1 >= 40)) return 1;
            ++n;
            Problem q = p;
            q.points2[4] = std::numeric_limits<float>::quiet_NaN();          // a NaN z passes the z < 0 test
            if (compare(q, "nan", false)) return 1;
            for (int level = 0; level < 3; ++level) {
                Problem hsl = p;
                spoil(hsl, level);
                if (compare(hsl, "hostile", false)) return 1;
                ++n;
            }
        }
    }
    double x[7] = {7, 7, 7, 7, 7, 7, 7}, H[28] = {}, b[7] = {1, 1, 1, 1, 1, 1, 1};
    CHECK(!geo_ldlt_solve<7>(H, 0.0, b, x) && x[0] == 7.0);                   // a zero pivot: x untouched
    CHECK(geo_ldlt_solve<7>(H, 2.0, b, x) && x[0] == 0.5 && x[6] == 0.5);     // H_66 = lambda alone
    printf("asan_optsim3_test ok (%d problems)\n", n);
    return 0;
}
