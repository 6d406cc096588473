// fuse_test.cpp -- XFmatcher::fuse (include/xfeat/ORBmatcher_xfeat.h), host and device overloads, against the C ABI (xfh_fuse_search) on one
// scene: three dumps that must be identical.
// usage: fuse_test in.bin out.bin
// in.bin : int32 nq, nt, nlevels, sim3; float th, scale_factor; xfh_camera (64 B); float Tcw[12], Ow[3]; keypoints[nt * 28 B]; targets[nt * 64 f32];
//          uright[nt f32]; queries[nq * 64 f32]; points, normals, distances[nq * 3 f32 each]; flags[nq u8]
// out.bin: three times (C ABI, host overload, device overload): int32 n_fused, best_idx[nq], status[nq] (widened), best_dist[nq], n_window[nq],
//          n_tested[nq], level[nq]
#define XFEAT_NO_OPENCV 1
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "xfeat/XFextractor.h"
#include "xfeat/ORBmatcher_xfeat.h"

using namespace ORB_SLAM3;

template <class T> static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

static void dump(FILE* o, int nfused, const std::vector<int>& idx, const std::vector<unsigned char>& status, const std::vector<int>& best,
                 const std::vector<int>& nwin, const std::vector<int>& ntest, const std::vector<int>& level) {
    fwrite(&nfused, 4, 1, o); fwrite(idx.data(), 4, idx.size(), o);
    for (unsigned char s : status) { const int v = s; fwrite(&v, 4, 1, o); }
    fwrite(best.data(), 4, best.size(), o); fwrite(nwin.data(), 4, nwin.size(), o); fwrite(ntest.data(), 4, ntest.size(), o); fwrite(level.data(), 4, level.size(), o);
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    int hdr[4]; float fl[2]; xfh_camera cam; float T[12], Ow[3];
    if (!f || !rd(f, hdr, 4) || !rd(f, fl, 2) || !rd(f, &cam, 1) || !rd(f, T, 12) || !rd(f, Ow, 3)) return 2;
    const int nq = hdr[0], nt = hdr[1], nl = hdr[2];
    const bool sim3 = hdr[3] != 0;
    const float th = fl[0];
    std::vector<float> sf(nl, 1.0f);
    for (int i = 1; i < nl; ++i) sf[i] = sf[i - 1] * fl[1];
    std::vector<XFgrid::KeyPoint> keys(nt);
    XFmatcher::Mat tg(nt, 64, 4), q(nq, 64, 4);
    std::vector<float> uright(nt), pts(3 * (size_t)nq), nr(3 * (size_t)nq), dd(3 * (size_t)nq);
    std::vector<unsigned char> flags(nq);
    if (!rd(f, keys.data(), nt) || !rd(f, tg.ptr<float>(0), (size_t)nt * 64) || !rd(f, uright.data(), nt) || !rd(f, q.ptr<float>(0), (size_t)nq * 64) ||
        !rd(f, pts.data(), pts.size()) || !rd(f, nr.data(), nr.size()) || !rd(f, dd.data(), dd.size()) || !rd(f, flags.data(), nq)) return 2;
    fclose(f);
    xfh_config cfg; xfh_config_default(&cfg);
    cfg.nfeatures = nt; cfg.max_height = 32; cfg.max_width = 32;
    xfh_ctx* ctx = nullptr;
    if (xfh_create(&cfg, &ctx) != XFH_OK) return 3;
    try {
        xfh_grid_bounds b;
        if (xfh_camera_bounds(&cam, &b) != XFH_OK) return 4;
        FILE* o = fopen(argv[2], "wb");
        std::vector<float> rmax(nl);
        if (xfh_scale_level_thresholds(fl[1], nl, rmax.data()) != XFH_OK) return 4;
        std::vector<int> idx(nq), best(nq), nwin(nq), ntest(nq), level(nq);
        std::vector<unsigned char> status(nq);
        int nf = -1;
        // the C ABI, host pointers
        if (xfh_fuse_search(ctx, nq, pts.data(), nr.data(), dd.data(), q.ptr<float>(0), flags.data(), T, Ow, &cam, &b, th, sf.data(), rmax.data(), nl,
                            (const xfh_keypoint*)keys.data(), tg.ptr<float>(0), nt, uright.data(), sim3 ? 0 : XFH_FUSE_CHI2, sim3 ? 0x7fffffff : 256, XFmatcher::TH_LOW,
                            status.data(), idx.data(), best.data(), nwin.data(), ntest.data(), level.data(), nullptr, &nf) != XFH_OK) return 4;
        dump(o, nf, idx, status, best, nwin, ntest, level);
        // the wrapper, host vectors
        XFgrid grid(ctx);
        grid.build(keys, b);
        XFmatcher matcher(ctx);
        std::vector<int> i2;
        const int n2 = matcher.fuse(q, pts, nr, dd, flags, T, Ow, cam, b, th, sf, grid, tg, i2, &uright, sim3);
        dump(o, n2, i2, matcher.lastFuseStatus(), matcher.lastFuseBestDist(), matcher.lastFuseWindow(), matcher.lastFuseTested(), matcher.lastFuseLevel());
        // the wrapper, device pointers
        const size_t bq = (size_t)nq * 256, bp = (size_t)nq * 12, bt = (size_t)nt * 256;
        void *dq, *dp, *dn, *ddd, *dfl, *dT, *dO, *dt, *du;
        if (xfh_dev_alloc(&dq, bq) || xfh_dev_alloc(&dp, bp) || xfh_dev_alloc(&dn, bp) || xfh_dev_alloc(&ddd, bp) || xfh_dev_alloc(&dfl, nq) || xfh_dev_alloc(&dT, 48) ||
            xfh_dev_alloc(&dO, 16) || xfh_dev_alloc(&dt, bt) || xfh_dev_alloc(&du, (size_t)nt * 4)) return 4;
        if (xfh_memcpy_h2d(dq, q.ptr<float>(0), bq) || xfh_memcpy_h2d(dp, pts.data(), bp) || xfh_memcpy_h2d(dn, nr.data(), bp) || xfh_memcpy_h2d(ddd, dd.data(), bp) ||
            xfh_memcpy_h2d(dfl, flags.data(), nq) || xfh_memcpy_h2d(dT, T, 48) || xfh_memcpy_h2d(dO, Ow, 12) || xfh_memcpy_h2d(dt, tg.ptr<float>(0), bt) ||
            xfh_memcpy_h2d(du, uright.data(), (size_t)nt * 4)) return 4;
        std::vector<int> i3;
        const int n3 = matcher.fuse(nq, (const float*)dp, (const float*)dn, (const float*)ddd, (const float*)dq, (const unsigned char*)dfl, (const float*)dT, (const float*)dO,
                                    cam, b, th, sf, grid, (const float*)dt, (const float*)du, i3, sim3);
        dump(o, n3, i3, matcher.lastFuseStatus(), matcher.lastFuseBestDist(), matcher.lastFuseWindow(), matcher.lastFuseTested(), matcher.lastFuseLevel());
        fclose(o);
        for (void* p : {dq, dp, dn, ddd, dfl, dT, dO, dt, du}) xfh_dev_free(p);
    } catch (const std::exception& e) { fprintf(stderr, "%s\n", e.what()); return 5; }
    xfh_destroy(ctx);
    return 0;
}
