// asan_triangulate_test.cpp -- the per-pair rule of xfh_triangulate_device (xfeatslam_amd/csrc/triangulate_math.h, the header the kernels compile) run on
// the host under AddressSanitizer + UBSan.  A stand-alone program: it links nothing of the library and never touches a GPU.
//   asan_triangulate_test                 hostile inputs (NaN, Inf, zeros, huge values in every field): every pair terminates with a status in range
//   asan_triangulate_test in.bin out.bin  the pairs tests/test_triangulate_ref.py wrote -> status, kind, x3D, normal, dist, x3Dh of each, which the test
//                                         compares byte for byte with the Python rule
#include "triangulate_math.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

struct Rec { float v[21]; };                                              // x, y, xr, yr, ur, depth, T[12], Ow[3]
static TriangObs obs_of(const Rec& r) { return TriangObs{r.v[0], r.v[1], r.v[2], r.v[3], r.v[4], r.v[5], r.v + 6, r.v + 18}; }

static TriangParams params_of(const float* f, int inertial) {
    TriangParams p;
    p.fx = f[0]; p.fy = f[1]; p.cx = f[2]; p.cy = f[3]; p.invfx = 1.0f / f[0]; p.invfy = 1.0f / f[1]; p.bf = f[4]; p.mb = f[4] / f[0];
    p.sigma2 = f[5]; p.ratio_factor = f[6]; p.scale_last = f[7]; p.far_th = f[8]; p.inertial = inertial;
    return p;
}

static int hostile() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float vals[] = {0.0f, -0.0f, 1.0f, -1.0f, 320.0f, 1e-38f, 1e38f, -1e38f, inf, -inf, nan, 4.0f, 0.0773f};
    const int nv = (int)(sizeof vals / sizeof vals[0]);
    const float cam[9] = {517.3f, 516.5f, 318.6f, 255.3f, 40.0f, 1.0f, 1.8f, 3.58f, 0.0f};
    const TriangParams p = params_of(cam, 0);
    Rec a, b;
    const float base1[21] = {384, 240, 384, 240, 374, 4, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0};
    const float base2[21] = {256, 240, 256, 240, -1, -1, 1, 0, 0, -1, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0};
    long count = 0;
    unsigned seed = 12345u;
    for (int f = 0; f < 42; ++f)
        for (int k = 0; k < nv; ++k)
            for (int g = 0; g < 42; g += 5) {
                memcpy(a.v, base1, sizeof base1); memcpy(b.v, base2, sizeof base2);
                (f < 21 ? a.v[f] : b.v[f - 21]) = vals[k];
                seed = seed * 1664525u + 1013904223u;
                (g < 21 ? a.v[g] : b.v[g - 21]) = vals[(seed >> 16) % nv];
                TriangPair r;
                triang_pair(p, obs_of(a), obs_of(b), &r);
                if (r.status < TRIANG_LOW_PARALLAX || r.status > TRIANG_ACCEPTED || r.kind < 0 || r.kind > 2) { printf("bad status %d kind %d\n", r.status, r.kind); return 1; }
                float nrm[3], dst[3];
                triang_normal_depth(r.x3D, a.v + 18, b.v + 18, p.scale_last, nrm, dst);
                ++count;
            }
    printf("hostile pairs: %ld\n", count);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) {
        if (hostile()) return 1;
        printf("asan_triangulate_test ok\n");
        return 0;
    }
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) return 2;
    int n = 0, inertial = 0;
    float cam[9];
    if (fread(&n, 4, 1, fi) != 1 || fread(cam, 4, 9, fi) != 9 || fread(&inertial, 4, 1, fi) != 1 || n < 0 || n > (1 << 20)) return 2;
    std::vector<Rec> recs((size_t)2 * n);
    if (n && fread(recs.data(), sizeof(Rec), recs.size(), fi) != recs.size()) return 2;
    fclose(fi);
    const TriangParams p = params_of(cam, inertial);
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) return 2;
    for (int i = 0; i < n; ++i) {
        const Rec &a = recs[2 * (size_t)i], &b = recs[2 * (size_t)i + 1];
        TriangPair r;
        triang_pair(p, obs_of(a), obs_of(b), &r);
        float nrm[3] = {0, 0, 0}, dst[3] = {0, 0, 0};
        if (r.status == TRIANG_ACCEPTED) triang_normal_depth(r.x3D, a.v + 18, b.v + 18, p.scale_last, nrm, dst);
        fwrite(&r.status, 4, 1, fo); fwrite(&r.kind, 4, 1, fo); fwrite(r.x3D, 4, 3, fo); fwrite(nrm, 4, 3, fo); fwrite(dst, 4, 3, fo); fwrite(r.x3Dh, 8, 4, fo);
    }
    fclose(fo);
    printf("asan_triangulate_test ok\n");
    return 0;
}
