// asan_mlpnp_test.cpp -- the rule of xfh_mlpnp_solve_host (xfeatslam_amd/csrc/mlpnp_math.h, the kernels' own lines) as a stand-alone program for
// AddressSanitizer + UBSan (tests/test_mlpnp_ref.py builds it with clang++ -fsanitize=address,undefined from this header alone: nothing of the library
// is linked, nothing runs on a GPU).
//   asan_mlpnp_test                      hostile inputs: any ints, NaN and Inf, draws out of range, hostile tables; every buffer sized exactly
//   asan_mlpnp_test solve IN OUT         one problem read from IN (see tests/test_mlpnp_ref.py), the four outputs over a 0xA5 pattern written to OUT
#include "mlpnp_math.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

struct Problem {
    int n, nq, max_iters, rand_max, chunk, start_iter;
    float cam[4], max_err;
    std::vector<float> xy, points;
    std::vector<int> assigned, iters, mins, draws;
    std::vector<unsigned char> valid;
};

static void run(const Problem& p, std::vector<int>& header, std::vector<float>& Tcw, std::vector<unsigned char>& inliers, std::vector<int>& aout) {
    header.assign(ML_HEADER_INTS, (int)0xA5A5A5A5); Tcw.resize(12); memset(Tcw.data(), 0xA5, 48); inliers.assign((size_t)p.n, 0xA5); aout.assign((size_t)p.n, (int)0xA5A5A5A5);
    std::vector<double> ws(ml_layout(p.n, p.max_iters).per_problem / 8 + 2);            // exactly the layout's bytes, 16-byte aligned below
    unsigned char* wp = (unsigned char*)(((uintptr_t)ws.data() + 15) & ~(uintptr_t)15);
    MlArgs a = {};
    a.B = 1; a.n = p.n; a.nq = p.nq; a.max_iters = p.max_iters; a.rand_max = p.rand_max; a.chunk = p.chunk; a.draws_stride = 0;
    a.cam = GeoCam{p.cam[0], p.cam[1], p.cam[2], p.cam[3]}; a.max_err = p.max_err; a.xy_un = p.xy.data(); a.points = p.points.data(); a.assigned = p.assigned.data();
    a.iters_of_N = p.iters.data(); a.min_of_N = p.mins.data(); a.start_iter = &p.start_iter; a.draws = p.draws.data(); a.valid = p.valid.empty() ? nullptr : p.valid.data();
    a.ws = wp; a.header = header.data(); a.Tcw = Tcw.data(); a.inliers = inliers.data(); a.assigned_out = aout.data();
    std::vector<unsigned char> flag((size_t)p.n);
    ml_host_problem(a, 0, flag.data());
}

static unsigned rnd(unsigned& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

static int hostile() {
    unsigned seed = 12345u;
    const float specials[6] = {NAN, INFINITY, -INFINITY, 0.0f, 1e30f, -1e-30f};
    const int ints[6] = {INT_MAX, INT_MIN, 0, -1, 1 << 30, 7};
    for (int round = 0; round < 40; ++round) {
        Problem p;
        p.n = 6 + (int)(rnd(seed) % 60); p.nq = 1 + (int)(rnd(seed) % 70); p.max_iters = 1 + (int)(rnd(seed) % 9); p.rand_max = 1 + (int)(rnd(seed) % 40000);
        p.chunk = (int)(rnd(seed) % 7); p.start_iter = ints[rnd(seed) % 6];
        const float cam[4] = {458.654f, 457.296f, 367.215f, 248.375f};
        for (int k = 0; k < 4; ++k) p.cam[k] = round % 7 == 6 ? specials[rnd(seed) % 6] : cam[k];
        p.max_err = 5.991f;
        p.xy.resize((size_t)p.n * 2); p.points.resize((size_t)p.nq * 3); p.assigned.resize((size_t)p.n); p.iters.resize((size_t)p.n + 1); p.mins.resize((size_t)p.n + 1);
        p.draws.resize((size_t)p.max_iters * 6);
        if (round & 1) p.valid.resize((size_t)p.nq);
        for (auto& v : p.xy) v = rnd(seed) % 9 == 0 ? specials[rnd(seed) % 6] : (float)(rnd(seed) % 700);
        for (auto& v : p.points) v = rnd(seed) % 9 == 0 ? specials[rnd(seed) % 6] : (float)(rnd(seed) % 2000) * 0.01f - 10.0f;
        for (auto& v : p.assigned) v = rnd(seed) % 5 == 0 ? ints[rnd(seed) % 6] : (int)(rnd(seed) % (unsigned)p.nq);
        for (auto& v : p.iters) v = rnd(seed) % 3 == 0 ? ints[rnd(seed) % 6] : (int)(rnd(seed) % 12);
        for (auto& v : p.mins) v = rnd(seed) % 3 == 0 ? ints[rnd(seed) % 6] : (int)(rnd(seed) % 12);
        for (auto& v : p.draws) v = rnd(seed) % 4 == 0 ? ints[rnd(seed) % 6] : (int)(rnd(seed) % 32768);
        for (auto& v : p.valid) v = (unsigned char)(rnd(seed) % 4 != 0);
        std::vector<int> header, aout; std::vector<float> Tcw; std::vector<unsigned char> inl;
        run(p, header, Tcw, inl, aout);
        if (header[ML_H_STATUS] < ML_TOO_FEW || header[ML_H_STATUS] > ML_REFINED) return 1;
    }
    // the pieces on degenerate input
    double rs[6]; const double f0[3] = {0.0, 0.0, 1.0}, fn[3] = {NAN, 1.0, 1.0};
    ml_nullspace(f0, rs); ml_nullspace(fn, rs);
    int set[6]; const int d[6] = {INT_MIN, INT_MAX, -1, 0, 5, 1 << 30};
    geo_set<ML_MIN_SET>(d, 1, 6, set);
    for (int k = 0; k < 6; ++k) if (set[k] < 0 || set[k] >= 6) return 2;
    const double z6[6] = {0, 0, 0, 0, 0, 0}, n6[6] = {NAN, 1, 2, INFINITY, 0, 1};
    if (ml_rank3(z6) != 0) return 3;
    ml_rank3(n6);
    int its, mn;
    ml_params(0.99, 10, 300, 6, 0.5f, 0, &its, &mn); ml_params(1.0, 10, 300, 6, 1.0f, 50, &its, &mn); ml_params(0.99, 10, 0, 6, 0.0f, 5, &its, &mn);
    return 0;
}

template <typename T> static bool rd(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc == 1) {
        const int rc = hostile();
        if (rc) { printf("asan_mlpnp_test FAILED %d\n", rc); return 1; }
        printf("asan_mlpnp_test ok\n");
        return 0;
    }
    if (argc != 4 || strcmp(argv[1], "solve")) return 2;
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 3;
    Problem p; int hdr[7];
    if (fread(hdr, 4, 7, f) != 7 || fread(p.cam, 4, 4, f) != 4 || fread(&p.max_err, 4, 1, f) != 1) return 4;
    p.n = hdr[0]; p.nq = hdr[1]; p.max_iters = hdr[2]; p.rand_max = hdr[3]; p.chunk = hdr[4]; p.start_iter = hdr[5];
    if (!rd(f, p.xy, (size_t)p.n * 2) || !rd(f, p.assigned, (size_t)p.n) || !rd(f, p.points, (size_t)p.nq * 3) || !rd(f, p.valid, hdr[6] ? (size_t)p.nq : 0) ||
        !rd(f, p.iters, (size_t)p.n + 1) || !rd(f, p.mins, (size_t)p.n + 1) || !rd(f, p.draws, (size_t)p.max_iters * 6)) return 5;
    fclose(f);
    std::vector<int> header, aout; std::vector<float> Tcw; std::vector<unsigned char> inl;
    run(p, header, Tcw, inl, aout);
    FILE* o = fopen(argv[3], "wb");
    if (!o) return 6;
    fwrite(header.data(), 4, header.size(), o); fwrite(Tcw.data(), 4, 12, o); fwrite(inl.data(), 1, inl.size(), o); fwrite(aout.data(), 4, aout.size(), o);
    fclose(o);
    return 0;
}
