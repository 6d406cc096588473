// poseopt_test.cpp -- ORB_SLAM3::XFoptimizer (include/xfeat/Optimizer_xfeat.h) on a scene the Python side writes out.
// usage: poseopt_test in.bin out.bin
// in.bin : int32 nt, nq, has_uright; float Tcw[12], cam[5] (fx fy cx cy bf), inv_sigma2; float xy[nt][2]; float uright[nt] if has_uright;
//          int32 assigned[nt]; float points[nq][3]
// out.bin: int32 return value; float Tcw[12]; uint8 outlier[nt]; float chi2[nt]; int32 header[8]; double final_chi2; then the same again from
//          a second call on the same object (it reuses its buffer), and float devicePose[12] read back from the device
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "xfeat/Optimizer_xfeat.h"

template <class T> static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T> static T* up(const std::vector<T>& v) {
    void* d = nullptr;
    if (xfh_dev_alloc(&d, v.size() * sizeof(T) + 16) != XFH_OK || xfh_memcpy_h2d(d, v.data(), v.size() * sizeof(T)) != XFH_OK) exit(3);
    return (T*)d;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    int h[3]; float T[12], cf[5], w;
    if (!f || !rd(f, h, 3) || !rd(f, T, 12) || !rd(f, cf, 5) || !rd(f, &w, 1)) return 2;
    const int nt = h[0], nq = h[1];
    std::vector<float> xy((size_t)nt * 2), ur(nt), pts((size_t)nq * 3);
    std::vector<int> as(nt);
    if (!rd(f, xy.data(), xy.size()) || (h[2] && !rd(f, ur.data(), ur.size())) || !rd(f, as.data(), as.size()) || !rd(f, pts.data(), pts.size())) return 2;
    fclose(f);
    try {
        xfh_config cfg; xfh_config_default(&cfg);
        cfg.nfeatures = 1; cfg.max_height = 32; cfg.max_width = 32;
        xfh_ctx* ctx = nullptr;
        if (xfh_create(&cfg, &ctx) != XFH_OK) return 4;
        xfh_camera cam; memset(&cam, 0, sizeof cam);
        cam.fx = cf[0]; cam.fy = cf[1]; cam.cx = cf[2]; cam.cy = cf[3]; cam.bf = cf[4]; cam.width = 640; cam.height = 480;
        float* dxy = up(xy); float* dur = h[2] ? up(ur) : nullptr; int* das = up(as); float* dp = up(pts);
        FILE* o = fopen(argv[2], "wb");
        {
            ORB_SLAM3::XFoptimizer opt(ctx);
            for (int rep = 0; rep < 2; ++rep) {
                float pose[12]; memcpy(pose, T, sizeof pose);
                const int ret = opt.PoseOptimization(pose, cam, nt, dxy, dur, das, nq, dp, w);
                std::vector<unsigned char> ol; std::vector<float> c2;
                opt.outliers(ol); opt.chi2(c2);
                if (ret != opt.nInitialCorrespondences() - opt.nBad() && opt.nInitialCorrespondences() >= 3) return 6;
                fwrite(&ret, 4, 1, o); fwrite(pose, 4, 12, o); fwrite(ol.data(), 1, nt, o); fwrite(c2.data(), 4, nt, o); fwrite(opt.header, 4, 8, o);
                fwrite(&opt.finalChi2, 8, 1, o);
            }
            float back[12];
            if (xfh_memcpy_d2h(back, opt.devicePose(), 48) != XFH_OK) return 5;
            fwrite(back, 4, 12, o);
            bool threw = false;                                            // what does not fit is refused
            try { float pose[12] = {0}; opt.PoseOptimization(pose, cam, XFH_GRID_MAX_N + 1, dxy, dur, das, nq, dp, w); } catch (const std::exception&) { threw = true; }
            if (!threw) return 6;
        }
        fclose(o);
        xfh_dev_free(dxy); if (dur) xfh_dev_free(dur); xfh_dev_free(das); xfh_dev_free(dp);
        xfh_destroy(ctx);
    } catch (const std::exception& e) { fprintf(stderr, "%s\n", e.what()); return 5; }
    return 0;
}
