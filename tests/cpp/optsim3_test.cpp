// optsim3_test.cpp -- ORB_SLAM3::XFoptimizer::OptimizeSim3 (include/xfeat/Optimizer_xfeat.h) on a scene the Python side writes out.
// usage: optsim3_test in.bin out.bin
// in.bin : int32 n1, M1, nq, n2, fix_scale, all_points, has_tmw; float cam[4] (fx fy cx cy), th2; float T1w[12], xy_un1[n1][2]; int32 point1[n1];
//          float points1[M1][3]; int32 assigned[n1]; float points2[nq][3]; uint8 flags2[nq]; int32 index2[nq]; float xy_un2[n2][2], T2w[12], S12[13], Tmw[12]
// out.bin: int32 return value; float S12[13]; int32 matches[n1]; uint8 status[n1]; float chi2[n1][2]; int32 header[16]; double state[8], final_chi2;
//          float Scw[12], Ow[3] read back from the device; then the same again from a second call on the same object (it reuses its buffer)
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
    int h[7]; float cf[4], th2;
    if (!f || !rd(f, h, 7) || !rd(f, cf, 4) || !rd(f, &th2, 1)) return 2;
    const int n1 = h[0], M1 = h[1], nq = h[2], n2 = h[3];
    std::vector<float> T1w(12), xy1((size_t)n1 * 2), pts1((size_t)M1 * 3), pts2((size_t)nq * 3), xy2((size_t)n2 * 2), T2w(12), S12(13), Tmw(12);
    std::vector<int> p1(n1), as(n1), i2(nq);
    std::vector<unsigned char> fl(nq);
    if (!rd(f, T1w.data(), 12) || !rd(f, xy1.data(), xy1.size()) || !rd(f, p1.data(), p1.size()) || !rd(f, pts1.data(), pts1.size()) || !rd(f, as.data(), as.size()) ||
        !rd(f, pts2.data(), pts2.size()) || !rd(f, fl.data(), fl.size()) || !rd(f, i2.data(), i2.size()) || !rd(f, xy2.data(), xy2.size()) || !rd(f, T2w.data(), 12) ||
        !rd(f, S12.data(), 13) || !rd(f, Tmw.data(), 12)) return 2;
    fclose(f);
    try {
        xfh_config cfg; xfh_config_default(&cfg);
        cfg.nfeatures = 1; cfg.max_height = 32; cfg.max_width = 32;
        xfh_ctx* ctx = nullptr;
        if (xfh_create(&cfg, &ctx) != XFH_OK) return 4;
        xfh_camera cam; memset(&cam, 0, sizeof cam);
        cam.fx = cf[0]; cam.fy = cf[1]; cam.cx = cf[2]; cam.cy = cf[3]; cam.width = 640; cam.height = 480;
        ORB_SLAM3::XFoptimizer::Sim3Input in = {n1, M1, nq, n2, up(T1w), up(xy1), up(p1), up(pts1), up(as), up(pts2), up(fl), up(i2), up(xy2), up(T2w), h[6] ? up(Tmw) : nullptr};
        FILE* o = fopen(argv[2], "wb");
        {
            ORB_SLAM3::XFoptimizer opt(ctx);
            for (int rep = 0; rep < 2; ++rep) {
                float S[13]; memcpy(S, S12.data(), sizeof S);
                const int ret = opt.OptimizeSim3(in, S, cam, cam, th2, h[4] != 0, h[5] != 0);
                std::vector<int> m; std::vector<unsigned char> st; std::vector<float> c2;
                opt.matches(m); opt.pairStatus(st); opt.pairChi2(c2);
                float Scw[12] = {0}, Ow[3] = {0}, back[13];
                if (h[6] && (xfh_memcpy_d2h(Scw, opt.deviceScw(), 48) != XFH_OK || xfh_memcpy_d2h(Ow, opt.deviceOw(), 12) != XFH_OK)) return 5;
                if (xfh_memcpy_d2h(back, opt.deviceS12(), 52) != XFH_OK || memcmp(back, S, 52) != 0) return 6;   // the similarity on the device is the one returned
                fwrite(&ret, 4, 1, o); fwrite(S, 4, 13, o); fwrite(m.data(), 4, n1, o); fwrite(st.data(), 1, n1, o); fwrite(c2.data(), 4, (size_t)n1 * 2, o);
                fwrite(opt.sim3Header, 4, 16, o); fwrite(opt.sim3State, 8, 8, o); fwrite(&opt.sim3FinalChi2, 8, 1, o); fwrite(Scw, 4, 12, o); fwrite(Ow, 4, 3, o);
            }
            {                                                              // without d_Tmw nothing is composed: the getters say so
                ORB_SLAM3::XFoptimizer::Sim3Input bare = in;
                bare.d_Tmw = nullptr;
                float S[13]; memcpy(S, S12.data(), sizeof S);
                opt.OptimizeSim3(bare, S, cam, cam, th2, h[4] != 0, h[5] != 0);
                if (opt.deviceScw() || opt.deviceOw() || !opt.deviceS12()) return 7;
            }
            bool threw = false;                                            // what does not fit is refused
            ORB_SLAM3::XFoptimizer::Sim3Input big = in;
            big.n1 = XFH_GRID_MAX_N + 1;
            try { float S[13] = {0}; opt.OptimizeSim3(big, S, cam, cam, th2, false, false); } catch (const std::exception&) { threw = true; }
            if (!threw) return 6;
        }
        fclose(o);
        xfh_destroy(ctx);
    } catch (const std::exception& e) { fprintf(stderr, "%s\n", e.what()); return 5; }
    return 0;
}
