// asan_essgraph_test.cpp -- essgraph_math.h alone under AddressSanitizer + UBSan (tests/test_essential_graph_ref.py::test_essgraph_math_under_sanitizers
// builds and runs it): a stand-alone program, nothing of the library linked, nothing on a GPU, nothing loaded into Python.
//   1. The pieces: exp(log(S)) = S over the four branches of Sim3::log, the 3 x 3 partial-pivot LU against a residual, the numeric Jacobian's exact zero
//      column under fix_scale, the solver on a system whose pivot fails (x untouched) in buffers of exact size.
//   2. Problem files written by the test (argv[1..]): the whole rule (eg_host_run) in buffers of EXACT size, compared byte for byte with the outputs of
//      the Python rule (tests/ref_essential_graph.py) the file carries; a NaN compares equal to a NaN.
#include "essgraph_math.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)
static bool same(double a, double b) { return memcmp(&a, &b, 8) == 0 || (a != a && b != b); }
static bool samef(float a, float b) { return memcmp(&a, &b, 4) == 0 || (a != a && b != b); }

static unsigned long long rng_state = 88172645463325252ull;
static double rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (double)(rng_state >> 11) / 9007199254740992.0; }

static void pieces() {
    const double thetas[] = {0.0, 1e-4, 0.0044721, 0.0044722, 0.01, 0.7, 2.5}, sigmas[] = {0.0, 0.5e-5, 1e-5, 2e-5, -2e-5, 0.3, -0.7};
    for (double th : thetas)
        for (double sg : sigmas) {
            if (th > 0.0 && th < 0.00447215 && fabs(sg) >= 1e-5) continue;   // sim3.h's own lines do not invert each other here: log's near branch, exp's general one
            const double u[7] = {th * 0.6, -th * 0.64, th * 0.48, 0.3, -1.2, 0.5, sg};
            Os3Sim S, B;
            os3_exp(u, &S);
            double l[7];
            eg_sim3_log(S, l);
            for (int k = 0; k < 7; ++k) CHECK(fabs(l[k] - u[k]) < 2e-5);     // the series branches are cut at eps = 1e-5
            os3_exp(l, &B);
            for (int k = 0; k < 3; ++k) CHECK(fabs(B.t[k] - S.t[k]) < 2e-5);
            CHECK(fabs(B.s - S.s) < 1e-9);
        }
    for (int it = 0; it < 200; ++it) {                                        // the LU: rows that must be swapped, residual small
        double M[9], M0[9], t[3], t0[3], x[3];
        for (int k = 0; k < 9; ++k) M0[k] = M[k] = rnd() - 0.5;
        if (it % 3 == 0) M0[0] = M[0] = 0.0;                                   // a zero where the first pivot would be
        for (int k = 0; k < 3; ++k) t0[k] = t[k] = rnd() - 0.5;
        eg_lu3_solve(M, t, x);
        for (int r = 0; r < 3; ++r) CHECK(fabs(M0[3 * r] * x[0] + M0[3 * r + 1] * x[1] + M0[3 * r + 2] * x[2] - t0[r]) < 1e-9 * (1.0 + fabs(x[0]) + fabs(x[1]) + fabs(x[2])));
    }
    {                                                                         // an edge under fix_scale: column 6 is exactly zero, a fixed vertex has no Jacobian
        const double ui[7] = {0.1, -0.2, 0.3, 1.0, 2.0, -1.0, 0.2}, uj[7] = {-0.3, 0.1, 0.2, 0.5, -1.0, 2.0, -0.1}, uc[7] = {0.01, 0.02, -0.01, 0.05, 0.0, -0.03, 0.02};
        Os3Sim Si, Sj, E, Sji, Swi, C;
        os3_exp(ui, &Si); os3_exp(uj, &Sj); os3_exp(uc, &E);
        os3_inverse(Si, &Swi); os3_mul(Sj, Swi, &Sji); os3_mul(E, Sji, &C);
        Os3Sims si, sj;
        for (int k = 0; k < 15; ++k) { os3_sims_piece(Si, 1, k, &si); os3_sims_piece(Sj, 1, k, &sj); }
        std::vector<double> perti(14 * 8), pinvj(14 * 8), e(7), Ji(49), Jj(49);
        for (int k = 0; k < 14; ++k) { eg_sim_put(si.pert[k], perti.data() + 8 * k); eg_sim_put(sj.pinv[k], pinvj.data() + 8 * k); }
        const double chi = eg_edge_linearize(C, Si, sj.inv, perti.data(), pinvj.data(), true, false, e.data(), Ji.data(), Jj.data());
        CHECK(chi > 0.0);
        for (int r = 0; r < 7; ++r) CHECK(Ji[7 * r + 6] == 0.0);
        for (int k = 0; k < 49; ++k) CHECK(Jj[k] == 0.0);
        double acc[XFH_EG_NSUM] = {};
        eg_accumulate(acc, Ji.data(), e.data());
        CHECK(acc[0] > 0.0 && acc[27] == 0.0);
    }
    for (int n : {1, 7, 64, 65}) {                                            // the solver in buffers of exact size; a failing pivot leaves x alone
        std::vector<double> S((size_t)n * n), b(n), x(n, 7.0), y(n);
        for (int i = 0; i < n; ++i) { for (int j = 0; j <= i; ++j) S[(size_t)i * n + j] = i == j ? n + 1.0 : rnd() - 0.5; b[i] = rnd(); }
        std::vector<double> S2 = S;
        CHECK(lba_ldlt_solve_host(S.data(), n, b.data(), x.data(), y.data()));
        S2[(size_t)(n - 1) * n + n - 1] = NAN;
        std::vector<double> x2(n, 7.0);
        CHECK(!lba_ldlt_solve_host(S2.data(), n, b.data(), x2.data(), y.data()));
        for (int i = 0; i < n; ++i) CHECK(x2[i] == 7.0);
    }
}

template <class T>
static std::vector<T> take(const char*& p, const char* end, size_t count) {
    CHECK((size_t)(end - p) >= count * sizeof(T));
    std::vector<T> v(count);
    if (count) memcpy(v.data(), p, count * sizeof(T));
    p += count * sizeof(T);
    return v;
}

static void problem(const char* path) {
    FILE* f = fopen(path, "rb");
    CHECK(f);
    fseek(f, 0, SEEK_END);
    const long size = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<char> file((size_t)size);
    CHECK(fread(file.data(), 1, (size_t)size, f) == (size_t)size);
    fclose(f);
    const char *p = file.data(), *end = p + size;
    const std::vector<int> h = take<int>(p, end, 10);
    const int nV = h[0], n_free = h[1], nE = h[2], nP = h[3], nS = h[4], pose_rows = h[5], point_rows = h[6];
    std::vector<float> pose = take<float>(p, end, (size_t)pose_rows * 12), pts = take<float>(p, end, (size_t)point_rows * 3);
    const std::vector<int> kf_row = take<int>(p, end, nV);
    const std::vector<unsigned char> kf_fixed = take<unsigned char>(p, end, nV);
    const std::vector<int> ci = take<int>(p, end, nV), ni = take<int>(p, end, nV);
    const std::vector<double> sim3 = take<double>(p, end, (size_t)nS * 8);
    const std::vector<int> ei = take<int>(p, end, nE), ej = take<int>(p, end, nE), ek = take<int>(p, end, nE), prow = take<int>(p, end, nP), pref = take<int>(p, end, nP);
    const std::vector<double> xS = take<double>(p, end, (size_t)nV * 8);
    const std::vector<float> xT = take<float>(p, end, (size_t)nV * 12), xP = take<float>(p, end, (size_t)nP * 3), xc = take<float>(p, end, nE);
    const std::vector<int> xh = take<int>(p, end, XFH_EG_HDR_INTS);
    const std::vector<double> xf = take<double>(p, end, 1);
    CHECK(p == end);
    std::vector<double> oS((size_t)nV * 8), of(1);
    std::vector<float> oT((size_t)nV * 12), oP((size_t)nP * 3), oc(nE);
    std::vector<int> oh(XFH_EG_HDR_INTS);
    std::vector<char> ws(eg_ws(nullptr, nV, nE, n_free).bytes);
    EgArgs a = {};
    a.nV = nV; a.nP = nP; a.nE = nE; a.nS = nS; a.n_free = n_free; a.pose_rows = pose_rows; a.point_rows = point_rows; a.fix_scale = h[7]; a.max_it = h[8]; a.write_back = h[9];
    a.pose_table = pose.data(); a.point_table = pts.data(); a.kf_row = kf_row.data(); a.kf_fixed = kf_fixed.data(); a.corrected_index = ci.data();
    a.noncorrected_index = ni.data(); a.sim3 = sim3.data(); a.edge_i = ei.data(); a.edge_j = ej.data(); a.edge_kind = ek.data(); a.point_row = prow.data();
    a.point_ref = pref.data(); a.Sim3_out = oS.data(); a.Tcw_out = oT.data(); a.points_out = oP.data(); a.chi2 = oc.data(); a.header = oh.data();
    a.final_chi2 = of.data(); a.ws = ws.data();
    eg_host_run(a);
    for (int k = 0; k < XFH_EG_HDR_INTS; ++k) CHECK(oh[k] == xh[k]);
    for (size_t k = 0; k < oS.size(); ++k) CHECK(same(oS[k], xS[k]));
    for (size_t k = 0; k < oT.size(); ++k) CHECK(samef(oT[k], xT[k]));
    for (size_t k = 0; k < oP.size(); ++k) CHECK(samef(oP[k], xP[k]));
    for (size_t k = 0; k < oc.size(); ++k) CHECK(samef(oc[k], xc[k]));
    CHECK(same(of[0], xf[0]));
}

int main(int argc, char** argv) {
    pieces();
    for (int k = 1; k < argc; ++k) problem(argv[k]);
    printf("asan_essgraph_test ok (%d files)\n", argc - 1);
    return 0;
}
