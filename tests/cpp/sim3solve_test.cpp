// sim3solve_test.cpp -- ORB_SLAM3::XFsim3Solver (include/xfeat/Sim3Solver_xfeat.h) compiled with g++ against libxfeat_hip.so.
//   sim3solve_test in.bin out.bin   the problem tests/test_gpu_sim3solve_cpp.py wrote (the "solve" format of tests/cpp/asan_sim3solve_test.cpp, then prob
//                                   and max_its) through the device overload, the host-container overload and the C ABI's host-pointer form
//                                   xfh_sim3_solve; per form: the bool, the header, the floats, the flags and the composed pose, which the test
//                                   compares with each other and with the rule
#include "xfeat/Sim3Solver_xfeat.h"

#include <cstdio>
#include <vector>

static void put(FILE* f, bool ok, const int* header, const float* floats, const std::vector<unsigned char>& inl, const float* Tcw, const float* Ow) {
    const int b = ok ? 1 : 0;
    fwrite(&b, 4, 1, f); fwrite(header, 4, XFH_SIM3_SOLVE_HEADER_INTS, f); fwrite(floats, 4, XFH_SIM3_SOLVE_FLOATS, f);
    fwrite(inl.data(), 1, inl.size(), f); fwrite(Tcw, 4, 12, f); fwrite(Ow, 4, 3, f);
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) return 2;
    int h[6]; float camv[8], max_err[2];
    if (fread(h, 4, 6, fi) != 6 || fread(camv, 4, 8, fi) != 8 || fread(max_err, 4, 2, fi) != 2) return 2;
    const int n1 = h[0], M = h[1], iters = h[2], rand_max = h[3], min_inliers = h[4]; const bool fix = h[5] != 0;
    std::vector<float> points((size_t)M * 3), T1w(12), T2w(12);
    std::vector<int> point1(n1), matched(n1), table((size_t)n1 + 1), draws((size_t)iters * 3);
    double prob; int max_its;
    if (fread(points.data(), 4, points.size(), fi) != points.size() || fread(point1.data(), 4, n1, fi) != (size_t)n1 || fread(matched.data(), 4, n1, fi) != (size_t)n1 ||
        fread(T1w.data(), 4, 12, fi) != 12 || fread(T2w.data(), 4, 12, fi) != 12 || fread(table.data(), 4, table.size(), fi) != table.size() ||
        fread(draws.data(), 4, draws.size(), fi) != draws.size() || fread(&prob, 8, 1, fi) != 1 || fread(&max_its, 4, 1, fi) != 1) return 2;
    fclose(fi);
    xfh_camera cam1 = {}, cam2 = {};
    cam1.fx = camv[0]; cam1.fy = camv[1]; cam1.cx = camv[2]; cam1.cy = camv[3]; cam2.fx = camv[4]; cam2.fy = camv[5]; cam2.cx = camv[6]; cam2.cy = camv[7];
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) return 2;
    try {
        xfh_config cfg; xfh_config_default(&cfg);
        cfg.nfeatures = 1; cfg.max_height = 32; cfg.max_width = 32;
        xfh_ctx* ctx = nullptr;
        if (xfh_create(&cfg, &ctx) != XFH_OK) return 4;
        {
            ORB_SLAM3::XFsim3Solver solver(ctx, cam1, cam2, iters);
            solver.SetRansacParameters(prob, min_inliers, max_its);
            solver.setDraws(draws.data(), rand_max);
            // 1. the device overload on arrays this program put on the device
            void *dp = nullptr, *d1 = nullptr, *dm = nullptr, *dT = nullptr;
            if (xfh_dev_alloc(&dp, points.size() * 4) || xfh_dev_alloc(&d1, (size_t)n1 * 4) || xfh_dev_alloc(&dm, (size_t)n1 * 4) || xfh_dev_alloc(&dT, 512)) return 4;
            if (xfh_memcpy_h2d(dp, points.data(), points.size() * 4) || xfh_memcpy_h2d(d1, point1.data(), (size_t)n1 * 4) || xfh_memcpy_h2d(dm, matched.data(), (size_t)n1 * 4) ||
                xfh_memcpy_h2d(dT, T1w.data(), 48) || xfh_memcpy_h2d((char*)dT + 256, T2w.data(), 48)) return 4;
            for (int form = 0; form < 2; ++form) {
                const bool ok = form == 0 ? solver.solve(n1, M, (const float*)dp, (const int*)d1, (const int*)dm, (const float*)dT, (const float*)((char*)dT + 256), fix)
                                          : solver.solve(points, point1, matched, T1w.data(), T2w.data(), fix);       // 2. the host containers
                if (ok != (solver.status() == XFH_SIM3_SOLVE_CONVERGED) || ok != (solver.deviceTcw() != nullptr)) return 5;
                int count = 0;
                for (bool b : solver.inliers()) count += b;
                if (count != solver.nInliers() || solver.GetEstimatedScale() != solver.floats[24] || solver.T12() != solver.floats) return 6;
                std::vector<unsigned char> inl(solver.inliers().begin(), solver.inliers().end());
                put(fo, ok, solver.header, solver.floats, inl, solver.Tcw, solver.Ow);
            }
            xfh_dev_free(dp); xfh_dev_free(d1); xfh_dev_free(dm); xfh_dev_free(dT);
        }
        // 3. the C ABI's host-pointer form with the same table
        int header[XFH_SIM3_SOLVE_HEADER_INTS] = {}; float floats[XFH_SIM3_SOLVE_FLOATS] = {}, Tcw[12] = {}, Ow[3] = {};
        std::vector<unsigned char> inl(n1, 0);
        if (xfh_sim3_solve(ctx, n1, M, points.data(), point1.data(), matched.data(), T1w.data(), T2w.data(), &cam1, &cam2, max_err[0], max_err[1], fix ? 1 : 0,
                           min_inliers, table.data(), iters, draws.data(), rand_max, header, floats, inl.data(), Tcw, Ow) != XFH_OK) return 7;
        put(fo, header[1] == XFH_SIM3_SOLVE_CONVERGED, header, floats, inl, Tcw, Ow);
        xfh_destroy(ctx);
    } catch (const std::exception& e) {
        fprintf(stderr, "sim3solve_test: %s\n", e.what());
        return 3;
    }
    fclose(fo);
    printf("sim3solve_test ok\n");
    return 0;
}
