// mlpnp_test.cpp -- ORB_SLAM3::XFmlpnpSolver (include/xfeat/MLPnPsolver_xfeat.h) compiled with g++ against libxfeat_hip.so.
//   mlpnp_test in.bin out.bin   the problem tests/test_gpu_mlpnp_cpp.py wrote (the "solve" format of tests/cpp/asan_mlpnp_test.cpp, then prob, min_inliers,
//                               max_its, eps, th2) through the call sequence of Tracking.cc:3715-3773 -- SetRansacParameters, then iterate(chunk) three times
//                               on the same solver, each call resuming where the last one returned -- in three forms: the device overload, the
//                               host-container overload, and the C ABI's host-pointer form xfh_mlpnp_solve with start_iter = the previous header's
//                               consumed count.  Per form and call: the bool, bNoMore, nInliers, the header, Tcw, the flags and mvpMapPoints, which
//                               the test compares with each other and with the rule
#include "xfeat/MLPnPsolver_xfeat.h"

#include <cstdio>
#include <vector>

static void put(FILE* f, bool ok, bool noMore, int nInl, const int* header, const float* Tcw, const std::vector<unsigned char>& inl, const std::vector<int>& assigned) {
    const int b[3] = {ok ? 1 : 0, noMore ? 1 : 0, nInl};
    fwrite(b, 4, 3, f); fwrite(header, 4, XFH_MLPNP_HEADER_INTS, f); fwrite(Tcw, 4, 12, f); fwrite(inl.data(), 1, inl.size(), f); fwrite(assigned.data(), 4, assigned.size(), f);
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) return 2;
    int h[7]; float camv[4], max_err;
    if (fread(h, 4, 7, fi) != 7 || fread(camv, 4, 4, fi) != 4 || fread(&max_err, 4, 1, fi) != 1) return 2;
    const int n = h[0], nq = h[1], iters = h[2], rand_max = h[3], chunk = h[4];
    std::vector<float> xy((size_t)n * 2), points((size_t)nq * 3);
    std::vector<int> assigned(n), ti((size_t)n + 1), tm((size_t)n + 1), draws((size_t)iters * 6);
    std::vector<unsigned char> valid(nq);
    double prob; int min_inliers, max_its; float eps, th2;
    if (fread(xy.data(), 4, xy.size(), fi) != xy.size() || fread(assigned.data(), 4, n, fi) != (size_t)n || fread(points.data(), 4, points.size(), fi) != points.size() ||
        fread(valid.data(), 1, nq, fi) != (size_t)nq || fread(ti.data(), 4, ti.size(), fi) != ti.size() || fread(tm.data(), 4, tm.size(), fi) != tm.size() ||
        fread(draws.data(), 4, draws.size(), fi) != draws.size() || fread(&prob, 8, 1, fi) != 1 || fread(&min_inliers, 4, 1, fi) != 1 || fread(&max_its, 4, 1, fi) != 1 ||
        fread(&eps, 4, 1, fi) != 1 || fread(&th2, 4, 1, fi) != 1) return 2;
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
            ORB_SLAM3::XFmlpnpSolver solver(ctx, cam, iters);
            solver.SetRansacParameters(prob, min_inliers, max_its, 6, eps, th2);
            solver.setDraws(draws.data(), rand_max);
            void *dxy = nullptr, *da = nullptr, *dp = nullptr, *dv = nullptr;
            if (xfh_dev_alloc(&dxy, xy.size() * 4) || xfh_dev_alloc(&da, (size_t)n * 4) || xfh_dev_alloc(&dp, points.size() * 4) || xfh_dev_alloc(&dv, (size_t)nq + 16)) return 4;
            if (xfh_memcpy_h2d(dxy, xy.data(), xy.size() * 4) || xfh_memcpy_h2d(da, assigned.data(), (size_t)n * 4) || xfh_memcpy_h2d(dp, points.data(), points.size() * 4) ||
                xfh_memcpy_h2d(dv, valid.data(), (size_t)nq)) return 4;
            for (int form = 0; form < 2; ++form) {
                if (form == 0) solver.setProblem(n, nq, (const float*)dxy, (const int*)da, (const float*)dp, (const unsigned char*)dv);     // 1. arrays this program put on the device
                else solver.setProblem(xy, assigned, points, &valid);                                                                     // 2. the host containers
                for (int call = 0; call < 3; ++call) {
                    bool bNoMore = false; std::vector<bool> vbInliers; int nInliers = -1; float Tcw[12] = {};
                    const bool ok = solver.iterate(chunk, bNoMore, vbInliers, nInliers, Tcw);
                    if (ok != (solver.deviceTcw() != nullptr) || (ok && vbInliers.size() != (size_t)n) || (!ok && (nInliers != 0 || !vbInliers.empty()))) return 5;
                    int count = 0;
                    for (bool b : vbInliers) count += b;
                    if (ok && count != nInliers) return 6;
                    std::vector<unsigned char> inl(solver.vbInliers.begin(), solver.vbInliers.end());
                    std::vector<int> aout((size_t)n, -1);
                    if (solver.deviceAssigned() && xfh_memcpy_d2h(aout.data(), solver.deviceAssigned(), (size_t)n * 4)) return 4;
                    put(fo, ok, bNoMore, nInliers, solver.header, Tcw, inl, aout);
                }
            }
            xfh_dev_free(dxy); xfh_dev_free(da); xfh_dev_free(dp); xfh_dev_free(dv);
        }
        // 3. the C ABI's host-pointer form with the test's tables, resumed through start_iter
        int start = 0;
        for (int call = 0; call < 3; ++call) {
            int header[XFH_MLPNP_HEADER_INTS] = {}; float Tcw[12] = {};
            std::vector<unsigned char> inl(n, 0); std::vector<int> aout(n, -1);
            if (xfh_mlpnp_solve(ctx, n, nq, xy.data(), assigned.data(), points.data(), valid.data(), &cam, max_err, ti.data(), tm.data(), chunk, start, iters, draws.data(),
                                rand_max, header, Tcw, inl.data(), aout.data()) != XFH_OK) return 7;
            const bool ok = header[1] == XFH_MLPNP_REFINED || header[1] == XFH_MLPNP_BEST;
            put(fo, ok, header[1] != XFH_MLPNP_REFINED, ok ? header[5] : 0, header, Tcw, inl, aout);
            if (header[1] != XFH_MLPNP_TOO_FEW) start = header[8];
        }
        xfh_destroy(ctx);
    } catch (const std::exception& e) {
        fprintf(stderr, "mlpnp_test: %s\n", e.what());
        return 3;
    }
    fclose(fo);
    printf("mlpnp_test ok\n");
    return 0;
}
