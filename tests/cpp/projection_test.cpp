// projection_test.cpp -- XFmatcher::searchByProjection (include/xfeat/ORBmatcher_xfeat.h), host and device overloads, against the C ABI
// (xfh_search_projection) on one scene: three dumps that must be identical.
// usage: projection_test in.bin out.bin
// in.bin : int32 nq, nt, init, th_high; float nn_ratio, radius; xfh_camera (64 B); float Tcw[12]; keypoints[nt * 28 B]; targets[nt * 64 f32];
//          queries[nq * 64 f32]; points[nq * 3 f32]; flags[nq u8]; skip[nt u8]; uright[nt f32]
// out.bin: three times (C ABI, host overload, device overload): int32 match[nq], assigned[nt], nmatches, status[nq] (widened), best[nq],
//          second[nq], n_candidates[nq]
#define XFEAT_NO_OPENCV 1
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "xfeat/XFextractor.h"
#include "xfeat/ORBmatcher_xfeat.h"

using namespace ORB_SLAM3;

template <class T> static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

static void dump(FILE* o, const std::vector<int>& match, const std::vector<int>& assigned, int nmatches, const std::vector<unsigned char>& status,
                 const std::vector<int>& best, const std::vector<int>& second, const std::vector<int>& ncand) {
    fwrite(match.data(), 4, match.size(), o); fwrite(assigned.data(), 4, assigned.size(), o); fwrite(&nmatches, 4, 1, o);
    for (unsigned char s : status) { const int v = s; fwrite(&v, 4, 1, o); }
    fwrite(best.data(), 4, best.size(), o); fwrite(second.data(), 4, second.size(), o); fwrite(ncand.data(), 4, ncand.size(), o);
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    int hdr[4]; float fl[2]; xfh_camera cam; float T[12];
    if (!f || !rd(f, hdr, 4) || !rd(f, fl, 2) || !rd(f, &cam, 1) || !rd(f, T, 12)) return 2;
    const int nq = hdr[0], nt = hdr[1], init = hdr[2], th_high = hdr[3];
    const float ratio = fl[0], radius = fl[1];
    std::vector<XFgrid::KeyPoint> keys(nt);
    XFmatcher::Mat tg(nt, 64, 4), q(nq, 64, 4);
    std::vector<float> pts(3 * (size_t)nq), uright(nt);
    std::vector<unsigned char> flags(nq), skip(nt);
    if (!rd(f, keys.data(), nt) || !rd(f, tg.ptr<float>(0), (size_t)nt * 64) || !rd(f, q.ptr<float>(0), (size_t)nq * 64) || !rd(f, pts.data(), pts.size()) ||
        !rd(f, flags.data(), nq) || !rd(f, skip.data(), nt) || !rd(f, uright.data(), nt)) return 2;
    fclose(f);
    xfh_config cfg; xfh_config_default(&cfg);
    cfg.nfeatures = nt; cfg.max_height = 32; cfg.max_width = 32;
    xfh_ctx* ctx = nullptr;
    if (xfh_create(&cfg, &ctx) != XFH_OK) return 3;
    try {
        xfh_grid_bounds b;
        if (xfh_camera_bounds(&cam, &b) != XFH_OK) return 4;
        FILE* o = fopen(argv[2], "wb");
        std::vector<int> match(nq), assigned(nt), best(nq), second(nq), ncand(nq);
        std::vector<unsigned char> status(nq);
        int nm = -1;
        // the C ABI, host pointers
        if (xfh_search_projection(ctx, XFH_PROJ_POINTS, nq, pts.data(), nullptr, T, &cam, &b, radius, q.ptr<float>(0), flags.data(), (const xfh_keypoint*)keys.data(),
                                  tg.ptr<float>(0), nt, skip.data(), uright.data(), init, th_high, ratio, status.data(), match.data(), best.data(), second.data(),
                                  ncand.data(), nullptr, assigned.data(), &nm) != XFH_OK) return 4;
        dump(o, match, assigned, nm, status, best, second, ncand);
        // the wrapper, host vectors
        XFgrid grid(ctx);
        grid.build(keys, b);
        XFmatcher matcher(ctx);
        std::vector<int> m2, a2;
        int n2 = matcher.searchByProjection(q, pts, flags, T, cam, b, radius, grid, tg, m2, a2, &skip, &uright, init, ratio, th_high);
        dump(o, m2, a2, n2, matcher.lastStatus(), matcher.lastBestDist(), matcher.lastSecondDist(), matcher.lastCandidates());
        // the wrapper, device pointers
        const size_t bq = (size_t)nq * 256, bp = (size_t)nq * 12, bt = (size_t)nt * 256;
        void *dq, *dp, *dfl, *dT, *dt, *ds, *du;
        if (xfh_dev_alloc(&dq, bq) || xfh_dev_alloc(&dp, bp) || xfh_dev_alloc(&dfl, nq) || xfh_dev_alloc(&dT, 48) || xfh_dev_alloc(&dt, bt) || xfh_dev_alloc(&ds, nt) ||
            xfh_dev_alloc(&du, (size_t)nt * 4)) return 4;
        if (xfh_memcpy_h2d(dq, q.ptr<float>(0), bq) || xfh_memcpy_h2d(dp, pts.data(), bp) || xfh_memcpy_h2d(dfl, flags.data(), nq) || xfh_memcpy_h2d(dT, T, 48) ||
            xfh_memcpy_h2d(dt, tg.ptr<float>(0), bt) || xfh_memcpy_h2d(ds, skip.data(), nt) || xfh_memcpy_h2d(du, uright.data(), (size_t)nt * 4)) return 4;
        std::vector<int> m3, a3;
        int n3 = matcher.searchByProjection(XFH_PROJ_POINTS, nq, (const float*)dp, nullptr, (const float*)dT, &cam, &b, radius, (const float*)dq, (const unsigned char*)dfl, grid,
                                            (const float*)dt, (const unsigned char*)ds, (const float*)du, m3, a3, init, ratio, th_high);
        dump(o, m3, a3, n3, matcher.lastStatus(), matcher.lastBestDist(), matcher.lastSecondDist(), matcher.lastCandidates());
        fclose(o);
        for (void* p : {dq, dp, dfl, dT, dt, ds, du}) xfh_dev_free(p);
    } catch (const std::exception& e) { fprintf(stderr, "%s\n", e.what()); return 5; }
    xfh_destroy(ctx);
    return 0;
}
