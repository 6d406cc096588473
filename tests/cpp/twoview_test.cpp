// twoview_test.cpp -- ORB_SLAM3::XFtwoView (include/xfeat/TwoViewReconstruction_xfeat.h) compiled with g++ against libxfeat_hip.so.
//   twoview_test in.bin out.bin   the problem tests/test_gpu_twoview_cpp.py wrote (the format of tests/cpp/asan_twoview_test.cpp) through the device
//                                 overload, the host-container overload and the C ABI's host-pointer form xfh_two_view; per form: the bool, the
//                                 header, T21, the flags, the points and the match list, which the test compares with each other and with the rule
#include "xfeat/TwoViewReconstruction_xfeat.h"

#include <cstdio>
#include <vector>

static void put(FILE* f, bool ok, const int* header, const float* T21, const std::vector<unsigned char>& tri, const std::vector<float>& p3d,
                const std::vector<int>& m) {
    const int b = ok ? 1 : 0;
    fwrite(&b, 4, 1, f); fwrite(header, 4, XFH_TWO_VIEW_HEADER_INTS, f); fwrite(T21, 4, 12, f);
    fwrite(tri.data(), 1, tri.size(), f); fwrite(p3d.data(), 4, p3d.size(), f); fwrite(m.data(), 4, m.size(), f);
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) return 2;
    int h[5]; float camv[4], sigma; double mpc;
    if (fread(h, 4, 5, fi) != 5 || fread(camv, 4, 4, fi) != 4 || fread(&sigma, 4, 1, fi) != 1 || fread(&mpc, 8, 1, fi) != 1) return 2;
    const int n1 = h[0], n2 = h[1], iters = h[2], rand_max = h[3], min_tri = h[4];
    std::vector<float> xy1((size_t)n1 * 2), xy2((size_t)n2 * 2);
    std::vector<int> m12(n1), draws((size_t)iters * 8);
    if (fread(xy1.data(), 4, xy1.size(), fi) != xy1.size() || fread(xy2.data(), 4, xy2.size(), fi) != xy2.size() || fread(m12.data(), 4, m12.size(), fi) != m12.size() ||
        fread(draws.data(), 4, draws.size(), fi) != draws.size()) return 2;
    fclose(fi);
    xfh_camera cam = {};
    cam.fx = camv[0]; cam.fy = camv[1]; cam.cx = camv[2]; cam.cy = camv[3];
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) return 2;
    try {
        xfh_config cfg; xfh_config_default(&cfg);
        cfg.nfeatures = 1; cfg.max_height = 32; cfg.max_width = 32;
        xfh_ctx* ctx = nullptr;
        if (xfh_create(&cfg, &ctx) != XFH_OK) return 4;
        {
            ORB_SLAM3::XFtwoView tv(ctx, cam, sigma, iters);
            tv.setDraws(draws.data(), rand_max);
            // 1. the device overload on arrays this program put on the device
            void *d1 = nullptr, *d2 = nullptr, *dm = nullptr;
            if (xfh_dev_alloc(&d1, xy1.size() * 4) || xfh_dev_alloc(&d2, xy2.size() * 4) || xfh_dev_alloc(&dm, m12.size() * 4)) return 4;
            if (xfh_memcpy_h2d(d1, xy1.data(), xy1.size() * 4) || xfh_memcpy_h2d(d2, xy2.data(), xy2.size() * 4) || xfh_memcpy_h2d(dm, m12.data(), m12.size() * 4)) return 4;
            for (int form = 0; form < 2; ++form) {
                const bool ok = form == 0 ? tv.Reconstruct(n1, (const float*)d1, n2, (const float*)d2, (const int*)dm, 1.0f, min_tri)
                                          : tv.Reconstruct(xy1, xy2, m12, 1.0f, min_tri);          // 2. the host containers
                std::vector<unsigned char> tri(tv.vbTriangulated.begin(), tv.vbTriangulated.end());
                std::vector<int> m = m12;
                if (tv.deviceMatches()) tv.matches(m);
                if (ok != (tv.status() >= XFH_TWO_VIEW_OK_H)) return 5;
                if (ok && !(tv.parallaxDegrees(tv.header[13]) >= 1.0f)) return 6;                  // the chosen hypothesis had the parallax asked for
                put(fo, ok, tv.header, tv.T21(), tri, tv.vP3D, m);
            }
            xfh_dev_free(d1); xfh_dev_free(d2); xfh_dev_free(dm);
        }
        // 3. the C ABI's host-pointer form with the same cosine
        int header[XFH_TWO_VIEW_HEADER_INTS] = {}; float floats[XFH_TWO_VIEW_FLOATS] = {};
        std::vector<unsigned char> ih(n1, 0), jf(n1, 0), tri(n1, 0);
        std::vector<float> p3d((size_t)n1 * 3, 0.0f);
        std::vector<int> m = m12;
        const double c1 = std::cos(1.0 * 3.14159265358979323846 / 180.0);
        if (xfh_two_view(ctx, n1, n2, xy1.data(), xy2.data(), m12.data(), &cam, sigma, iters, draws.data(), rand_max, c1, min_tri, header, floats, ih.data(),
                         jf.data(), tri.data(), p3d.data(), m.data()) != XFH_OK) return 7;
        put(fo, header[1] >= XFH_TWO_VIEW_OK_H, header, floats + 21, tri, p3d, m);
        xfh_destroy(ctx);
    } catch (const std::exception& e) {
        fprintf(stderr, "twoview_test: %s\n", e.what());
        return 3;
    }
    fclose(fo);
    printf("twoview_test ok\n");
    return 0;
}
