// asan_twoview_test.cpp -- the whole rule of xfh_two_view_device (xfeatslam_amd/csrc/twoview_math.h, the header the kernels compile) run on ONE host
// thread under AddressSanitizer + UBSan.  A stand-alone program: it links nothing of the library and never touches a GPU.
//   asan_twoview_test                 hostile inputs: NaN, Inf and huge coordinates, matches outside 0 .. n2 - 1, duplicate idx2, draws below 0 and above
//                                     rand_max, tiny and odd sizes: every problem terminates with a status in range and indices inside the buffers
//   asan_twoview_test in.bin out.bin  the problem tests/test_twoview_ref.py wrote -> header, floats, the three flag arrays, p3d, matches_out, which the
//                                     test compares byte for byte with the Python rule
#include "twoview_math.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

struct Problem {
    int n1, n2, iters, rand_max, min_tri;
    float cam[4], sigma;
    double mpc;
    std::vector<float> xy1, xy2;
    std::vector<int> m12, draws;
    // outputs
    std::vector<int> header, matches_out;
    std::vector<float> floats, p3d;
    std::vector<unsigned char> inl_h, inl_f, tri;
};

static void run(Problem& p) {
    const TvLayout L = tv_layout(p.n1, p.iters);
    std::vector<double> ws(L.per_problem / 8 + 2);                          // 16-byte aligned pieces inside an 8-byte aligned block: offsets are multiples of 16
    std::vector<float> scratch((size_t)(p.n1 > p.n2 ? p.n1 : p.n2));
    p.header.assign(TV_HEADER_INTS, 0); p.floats.assign(TV_FLOATS, 0.0f);
    p.inl_h.assign(p.n1, 0); p.inl_f.assign(p.n1, 0); p.tri.assign(p.n1, 0); p.p3d.assign((size_t)p.n1 * 3, 0.0f); p.matches_out = p.m12;
    TvArgs a = {};
    a.B = 1; a.n1 = p.n1; a.n2 = p.n2; a.iters = p.iters; a.rand_max = p.rand_max; a.min_tri = p.min_tri; a.draws_stride = 0;
    a.cam = GeoCam{p.cam[0], p.cam[1], p.cam[2], p.cam[3]}; a.sigma = p.sigma; a.min_parallax_cos = p.mpc;
    a.xy1 = p.xy1.data(); a.xy2 = p.xy2.data(); a.match12 = p.m12.data(); a.draws = p.draws.data(); a.ws = (unsigned char*)ws.data();
    a.header = p.header.data(); a.fout = p.floats.data(); a.inl_h = p.inl_h.data(); a.inl_f = p.inl_f.data(); a.tri = p.tri.data();
    a.p3d = p.p3d.data(); a.matches_out = p.matches_out.data();
    tv_host_problem(a, 0, scratch.data());
}

static unsigned lcg(unsigned& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

static int hostile() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float bad[] = {nan, inf, -inf, 1e38f, -1e38f, 0.0f, -0.0f, 1e-38f};
    const int sizes[][3] = {{1, 1, 1}, {7, 9, 2}, {8, 8, 3}, {9, 8, 1}, {65, 33, 5}, {130, 257, 4}};
    unsigned seed = 777u;
    long count = 0;
    for (const auto& sz : sizes)
        for (int mode = 0; mode < 12; ++mode) {
            Problem p;
            p.n1 = sz[0]; p.n2 = sz[1]; p.iters = sz[2]; p.rand_max = mode % 3 == 0 ? 1 : (mode % 3 == 1 ? 32767 : 2147483647); p.min_tri = mode & 1 ? 0 : 50;
            p.cam[0] = 458.654f; p.cam[1] = 457.296f; p.cam[2] = 367.215f; p.cam[3] = 248.375f;
            if (mode == 10) p.cam[0] = 0.0f;
            if (mode == 11) p.cam[3] = nan;
            p.sigma = mode == 9 ? 1e-20f : 1.0f; p.mpc = 0.9998476951563913;
            p.xy1.resize((size_t)p.n1 * 2); p.xy2.resize((size_t)p.n2 * 2); p.m12.resize(p.n1); p.draws.resize((size_t)p.iters * 8);
            for (auto& v : p.xy1) v = (float)(lcg(seed) % 7520) * 0.1f;
            for (auto& v : p.xy2) v = (float)(lcg(seed) % 7520) * 0.1f;
            for (int i = 0; i < p.n1; ++i) {
                const unsigned r = lcg(seed);
                p.m12[i] = mode == 1 ? 0                                       // every keypoint matched to the same idx2
                           : mode == 2 ? (int)(r % (2u * p.n2 + 4u)) - 2         // entries below 0 and at or above n2
                           : mode == 3 ? (r & 1 ? (int)0x7fffffff : (int)0x80000000)
                                       : (int)(r % (unsigned)p.n2);
            }
            for (auto& d : p.draws) {
                const unsigned r = lcg(seed);
                d = mode == 4 ? -1 - (int)(r % 1000u) : mode == 5 ? 2147483647 : mode == 6 ? 0 : (int)(r % 0x7fffffffu);    // below 0, above rand_max, all equal
            }
            if (mode == 7) for (size_t k = 0; k < p.xy1.size(); k += 3) p.xy1[k] = bad[(k / 3) % 8];
            if (mode == 8) { for (auto& v : p.xy2) v = bad[lcg(seed) % 8]; for (auto& v : p.xy1) v = 100.0f; }
            run(p);
            const int st = p.header[TV_H_STATUS], ch = p.header[TV_H_CHOSEN];
            if (st < TV_TOO_FEW || st > TV_OK_F || ch < -1 || ch > 7 || p.header[TV_H_N] < 0 || p.header[TV_H_N] > p.n1) { printf("bad header: status %d chosen %d\n", st, ch); return 1; }
            if ((st >= TV_OK_H) != (ch >= 0)) { printf("status %d with chosen %d\n", st, ch); return 1; }
            ++count;
        }
    // the set generator alone: every N from 8 to 80 with draws at both ends -> eight distinct indices below N
    for (int N = 8; N <= 80; ++N)
        for (int k = 0; k < 50; ++k) {
            int d[8], s[8];
            for (int j = 0; j < 8; ++j) { const unsigned r = lcg(seed); d[j] = k == 0 ? 0 : k == 1 ? 32767 : k == 2 ? 40000 : k == 3 ? -5 : (int)(r % 32768u); }
            geo_set<TV_MIN_SET>(d, 32767, N, s);
            for (int j = 0; j < 8; ++j) {
                if (s[j] < 0 || s[j] >= N) { printf("set index %d outside 0 .. %d\n", s[j], N - 1); return 1; }
                for (int i = 0; i < j; ++i) if (s[i] == s[j]) { printf("set repeats %d\n", s[j]); return 1; }
            }
            ++count;
        }
    printf("hostile problems: %ld\n", count);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) {
        if (hostile()) return 1;
        printf("asan_twoview_test ok\n");
        return 0;
    }
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) return 2;
    Problem p;
    int h[5];
    if (fread(h, 4, 5, fi) != 5 || fread(p.cam, 4, 4, fi) != 4 || fread(&p.sigma, 4, 1, fi) != 1 || fread(&p.mpc, 8, 1, fi) != 1) return 2;
    p.n1 = h[0]; p.n2 = h[1]; p.iters = h[2]; p.rand_max = h[3]; p.min_tri = h[4];
    if (p.n1 < 1 || p.n1 > 16384 || p.n2 < 1 || p.n2 > 16384 || p.iters < 1 || p.iters > TV_MAX_ITERS || p.rand_max < 1) return 2;
    p.xy1.resize((size_t)p.n1 * 2); p.xy2.resize((size_t)p.n2 * 2); p.m12.resize(p.n1); p.draws.resize((size_t)p.iters * 8);
    if (fread(p.xy1.data(), 4, p.xy1.size(), fi) != p.xy1.size() || fread(p.xy2.data(), 4, p.xy2.size(), fi) != p.xy2.size() ||
        fread(p.m12.data(), 4, p.m12.size(), fi) != p.m12.size() || fread(p.draws.data(), 4, p.draws.size(), fi) != p.draws.size()) return 2;
    fclose(fi);
    run(p);
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) return 2;
    fwrite(p.header.data(), 4, p.header.size(), fo); fwrite(p.floats.data(), 4, p.floats.size(), fo);
    fwrite(p.inl_h.data(), 1, p.inl_h.size(), fo); fwrite(p.inl_f.data(), 1, p.inl_f.size(), fo); fwrite(p.tri.data(), 1, p.tri.size(), fo);
    fwrite(p.p3d.data(), 4, p.p3d.size(), fo); fwrite(p.matches_out.data(), 4, p.matches_out.size(), fo);
    fclose(fo);
    printf("asan_twoview_test ok\n");
    return 0;
}
