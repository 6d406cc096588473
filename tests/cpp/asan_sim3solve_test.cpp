// asan_sim3solve_test.cpp -- the rule of xfh_sim3_solve_device and xfh_sim3_merge_matches_device (xfeatslam_amd/csrc/sim3solve_math.h, the kernels'
// own lines) on ONE host thread under AddressSanitizer + UBSan: a stand-alone program built from the header alone (tests/test_sim3solve_ref.py);
// nothing of the library is linked, nothing runs on a GPU, nothing is loaded into Python.
//   asan_sim3solve_test                     good, NaN and hostile problems: indices far out of range, draws of any int, absurd iteration counts
//   asan_sim3solve_test solve in.bin out.bin   one problem written by the Python test; the outputs (over 0xA5 bytes) for a byte comparison with the rule
//   asan_sim3solve_test merge in.bin out.bin   one merge likewise
#include "sim3solve_math.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

struct Problem {
    int n1 = 0, M = 0, max_iters = 0, rand_max = 32767, min_inliers = 15, fix_scale = 0;
    float cam[8] = {458.654f, 457.296f, 367.215f, 248.375f, 435.2f, 435.2f, 376.0f, 240.0f}, max_err[2] = {9.0f, 9.0f};
    std::vector<float> points, T1w, T2w;
    std::vector<int> point1, matched, table, draws;
};
struct Outputs { std::vector<int> header; std::vector<float> floats, Tcw, Ow; std::vector<unsigned char> inliers; };

static Outputs run(const Problem& p) {
    Outputs o;
    o.header.assign(S3_HEADER_INTS, (int)0xA5A5A5A5); o.floats.resize(S3_FLOATS); o.Tcw.resize(12); o.Ow.resize(3); o.inliers.assign(p.n1, 0xA5);
    memset(o.floats.data(), 0xA5, S3_FLOATS * 4); memset(o.Tcw.data(), 0xA5, 48); memset(o.Ow.data(), 0xA5, 12);
    std::vector<unsigned char> ws(s3_workspace_bytes(p.n1, p.M, 1));        // exactly the documented size: the sanitizer sees any byte past it
    S3Args a = {};
    a.B = 1; a.n1 = p.n1; a.M = p.M; a.max_iters = p.max_iters; a.rand_max = p.rand_max; a.min_inliers = p.min_inliers; a.fix_scale = p.fix_scale;
    a.cam1 = GeoCam{p.cam[0], p.cam[1], p.cam[2], p.cam[3]}; a.cam2 = GeoCam{p.cam[4], p.cam[5], p.cam[6], p.cam[7]};
    a.max_err1 = p.max_err[0]; a.max_err2 = p.max_err[1];
    a.points = p.points.data(); a.T1w = p.T1w.data(); a.T2w = p.T2w.data(); a.point1 = p.point1.data(); a.matched = p.matched.data();
    a.iters_of_N = p.table.data(); a.draws = p.draws.data(); a.ws = ws.data();
    a.header = o.header.data(); a.fout = o.floats.data(); a.inliers = o.inliers.data(); a.Tcw = o.Tcw.data(); a.Ow = o.Ow.data();
    s3_host_problem(a, 0);
    return o;
}

static unsigned rng_state = 12345u;
static unsigned rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static float frand(float lo, float hi) { return lo + (hi - lo) * (float)(rnd() & 0xffff) / 65535.0f; }

static Problem synthetic(int n1, int M, int max_iters) {
    Problem p;
    p.n1 = n1; p.M = M; p.max_iters = max_iters;
    p.points.resize((size_t)M * 3); p.point1.resize(n1); p.matched.resize(n1); p.table.resize(n1 + 1); p.draws.resize((size_t)max_iters * 3);
    p.T1w = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}; p.T2w = {1, 0, 0, 0.1f, 0, 1, 0, -0.05f, 0, 0, 1, 0.02f};
    for (int i = 0; i < M / 2; ++i) {
        const float x = frand(-2, 2), y = frand(-1.5f, 1.5f), z = frand(3, 9);
        p.points[3 * i] = x; p.points[3 * i + 1] = y; p.points[3 * i + 2] = z;
        float* q = &p.points[3 * (size_t)(M / 2 + i)];
        q[0] = x - 0.1f; q[1] = y + 0.05f; q[2] = z - 0.02f;
    }
    for (int i = 0; i < n1; ++i) { p.point1[i] = i % (M / 2); p.matched[i] = (i % 3 == 2) ? -1 : M / 2 + i % (M / 2); }
    for (int N = 0; N <= n1; ++N) p.table[N] = s3_iterations(0.99, p.min_inliers, 300, N);
    for (size_t k = 0; k < p.draws.size(); ++k) p.draws[k] = (int)(rnd() % 32768u);
    return p;
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static int hostile() {
    Problem good = synthetic(70, 64, 40);
    Outputs o = run(good);
    CHECK(o.header[S3_H_STATUS] == S3_CONVERGED && o.header[S3_H_N] == 47 && o.header[S3_H_NINL] == 47);
    Problem p = good;                                                       // indices far out of range: no correspondence
    p.point1[0] = 64; p.point1[1] = -1; p.point1[3] = 2147483647; p.matched[4] = -2147483647 - 1; p.matched[6] = 1 << 30; p.matched[7] = 64;
    o = run(p);
    CHECK(o.header[S3_H_N] == 47 - 6 && o.header[S3_H_STATUS] == S3_CONVERGED);
    p = good;                                                               // draws of any int
    for (size_t k = 0; k < p.draws.size(); ++k) p.draws[k] = (k % 4 == 0) ? -2147483647 - 1 : ((k % 4 == 1) ? 2147483647 : (int)(rnd() * 977u));
    o = run(p);
    CHECK(o.header[S3_H_STATUS] != S3_TOO_FEW && o.header[S3_H_ITS] >= 1 && o.header[S3_H_ITS] <= 40);
    const int absurd[] = {0, -1, -2147483647 - 1, 2147483647, 4097, 41};   // a table of absurd iteration counts: clamped into 1 .. max_iters
    for (int v : absurd) {
        p = good;
        for (int& t : p.table) t = v;
        for (int i = 0; i < p.M / 2; ++i) p.points[3 * (size_t)(p.M / 2 + i)] += frand(3, 30);      // no hypothesis converges: every iteration runs
        o = run(p);
        CHECK(o.header[S3_H_STATUS] == S3_NO_MORE && o.header[S3_H_ITS] == (v < 1 ? 1 : 40) && o.header[S3_H_CONSUMED] == o.header[S3_H_ITS]);
    }
    p = good;                                                               // NaN and Inf everywhere
    for (size_t k = 0; k < p.points.size(); k += 5) p.points[k] = (k % 2) ? NAN : INFINITY;
    p.T2w[3] = NAN; p.cam[6] = INFINITY;
    o = run(p);
    CHECK(o.header[S3_H_STATUS] == S3_NO_MORE && o.header[S3_H_BEST_COUNT] == 0);
    p = synthetic(3, 8, 1);                                                 // the smallest problems
    p.min_inliers = 0; p.matched = {4, 5, 6};
    o = run(p);
    CHECK(o.header[S3_H_N] == 3 && o.header[S3_H_STATUS] != S3_TOO_FEW);
    p.matched[1] = -1;
    o = run(p);
    CHECK(o.header[S3_H_N] == 2 && o.header[S3_H_STATUS] == S3_TOO_FEW && o.inliers[0] == 0xA5);
    p = synthetic(1, 2, 1);
    o = run(p);
    CHECK(o.header[S3_H_STATUS] == S3_TOO_FEW);
    // the merge on hostile lists
    const int J = 3, n1 = 50, n2 = 40, M = 30;
    std::vector<int> m12((size_t)J * n1), p2((size_t)J * n2), owner(M), matched(n1), kf(n1);
    for (int& v : m12) v = (int)(rnd() % 60u) - 10;
    for (int& v : p2) v = (int)(rnd() % 50u) - 10;
    m12[5] = 2147483647; m12[6] = -2147483647 - 1; p2[3] = 2147483647; p2[4] = -2147483647 - 1;
    int num = -1;
    s3_merge_host(J, n1, n2, M, m12.data(), p2.data(), owner.data(), matched.data(), kf.data(), &num);
    int distinct = 0, filled = 0;
    for (int r = 0; r < M; ++r) distinct += owner[r] != INT_MAX;
    for (int k = 0; k < n1; ++k) { CHECK(matched[k] >= -1 && matched[k] < M && kf[k] >= -1 && kf[k] < J && (matched[k] < 0) == (kf[k] < 0)); filled += matched[k] >= 0; }
    CHECK(num == distinct && filled <= num && num > 0);
    printf("asan_sim3solve_test ok\n");
    return 0;
}

template <typename T> static bool rd(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }
template <typename T> static void wr(FILE* f, const std::vector<T>& v) { fwrite(v.data(), sizeof(T), v.size(), f); }

int main(int argc, char** argv) {
    if (argc == 1) return hostile();
    if (argc != 4) return 2;
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 3;
    const std::string mode = argv[1];
    if (mode == "solve") {
        Problem p;
        int h[6];
        if (fread(h, 4, 6, f) != 6 || fread(p.cam, 4, 8, f) != 8 || fread(p.max_err, 4, 2, f) != 2) return 4;
        p.n1 = h[0]; p.M = h[1]; p.max_iters = h[2]; p.rand_max = h[3]; p.min_inliers = h[4]; p.fix_scale = h[5];
        if (!rd(f, p.points, (size_t)p.M * 3) || !rd(f, p.point1, p.n1) || !rd(f, p.matched, p.n1) || !rd(f, p.T1w, 12) || !rd(f, p.T2w, 12) ||
            !rd(f, p.table, (size_t)p.n1 + 1) || !rd(f, p.draws, (size_t)p.max_iters * 3)) return 4;
        fclose(f);
        const Outputs o = run(p);
        FILE* g = fopen(argv[3], "wb");
        if (!g) return 5;
        wr(g, o.header); wr(g, o.floats); wr(g, o.inliers); wr(g, o.Tcw); wr(g, o.Ow);
        fclose(g);
        return 0;
    }
    if (mode == "merge") {
        int h[4];
        if (fread(h, 4, 4, f) != 4) return 4;
        std::vector<int> m12, p2, owner(h[3]), matched(h[1]), kf(h[1]), num(1);
        if (!rd(f, m12, (size_t)h[0] * h[1]) || !rd(f, p2, (size_t)h[0] * h[2])) return 4;
        fclose(f);
        s3_merge_host(h[0], h[1], h[2], h[3], m12.data(), p2.data(), owner.data(), matched.data(), kf.data(), num.data());
        FILE* g = fopen(argv[3], "wb");
        if (!g) return 5;
        wr(g, matched); wr(g, kf); wr(g, num);
        fclose(g);
        return 0;
    }
    return 2;
}
