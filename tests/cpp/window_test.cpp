// window_test.cpp -- XFgrid / XFmatcher::searchWindow (include/xfeat/ORBmatcher_xfeat.h) the way SearchByProjection(Frame, Frame)
// would use them: build the grid of the current frame's keypoints, one searchWindow call for all projected points, and
// featuresInArea for callers that still want the index list.
// usage: window_test in.bin out.bin
// in.bin : int32 nq, nt, init, with_filters; float bounds[4]; keypoints[nt * 28 B]; targets[nt * 64 f32]; queries[nq * 64 f32];
//          uvr[nq * 3 f32]; skip[nt u8]; uright[nt f32]; ur_query[nq f32]
// out.bin: 5 x int32[nq] (best_idx, best_dist, second_idx, second_dist, n_candidates) plain, the same with the filters, then per
//          query int32 count + int32 indices of featuresInArea (host grid built from the vector), then the same from a grid built
//          with buildFromRecord on a record made of the same keypoints
#define XFEAT_NO_OPENCV 1
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "xfeat/XFextractor.h"
#include "xfeat/ORBmatcher_xfeat.h"

using namespace ORB_SLAM3;

template <class T> static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    int hdr[4]; xfh_grid_bounds b;
    if (!f || !rd(f, hdr, 4) || !rd(f, &b, 1)) return 2;
    const int nq = hdr[0], nt = hdr[1], init = hdr[2];
    std::vector<XFgrid::KeyPoint> keys(nt);
    XFmatcher::Mat tg(nt, 64, 4), q(nq, 64, 4);
    std::vector<float> uvr(3 * (size_t)nq), uright(nt), urq(nq);
    std::vector<unsigned char> skip(nt);
    if (!rd(f, keys.data(), nt) || !rd(f, tg.ptr<float>(0), (size_t)nt * 64) || !rd(f, q.ptr<float>(0), (size_t)nq * 64) || !rd(f, uvr.data(), uvr.size()) ||
        !rd(f, skip.data(), nt) || !rd(f, uright.data(), nt) || !rd(f, urq.data(), nq)) return 2;
    fclose(f);
    xfh_config cfg; xfh_config_default(&cfg);
    cfg.nfeatures = nt; cfg.max_height = 32; cfg.max_width = 32;
    xfh_ctx* ctx = nullptr;
    if (xfh_create(&cfg, &ctx) != XFH_OK) return 3;
    try {
        XFgrid grid(ctx);
        grid.build(keys, b);
        XFmatcher matcher(ctx);
        std::vector<int> r[10];
        matcher.searchWindow(q, uvr, grid, tg, r[0], r[1], r[2], r[3], r[4], init);
        matcher.searchWindow(q, uvr, grid, tg, r[5], r[6], r[7], r[8], r[9], init, &skip, &uright, &urq);
        FILE* o = fopen(argv[2], "wb");
        for (auto& v : r) fwrite(v.data(), 4, v.size(), o);
        // a record holding the same keypoints, in device memory: header n_valid = nt, mono_index = nt
        std::vector<unsigned char> rec(xfh_record_bytes(nt), 0);
        int* rh = (int*)rec.data(); rh[0] = nt; rh[1] = nt;
        memcpy(rec.data() + xfh_record_kps_offset(), keys.data(), (size_t)nt * 28);
        void* d_rec = nullptr;
        if (xfh_dev_alloc(&d_rec, rec.size()) != XFH_OK || xfh_memcpy_h2d(d_rec, rec.data(), rec.size()) != XFH_OK) return 4;
        XFgrid grid2(ctx);
        grid2.buildFromRecord(d_rec, nt, b, XFH_GRID_SKIP_PADDING);
        for (XFgrid* g : {&grid, &grid2})
            for (int i = 0; i < nq; ++i) {
                const std::vector<size_t> v = g->featuresInArea(uvr[3 * i], uvr[3 * i + 1], uvr[3 * i + 2]);
                const int cnt = (int)v.size();
                fwrite(&cnt, 4, 1, o);
                for (size_t k : v) { const int x = (int)k; fwrite(&x, 4, 1, o); }
            }
        fclose(o);
        xfh_dev_free(d_rec);
    } catch (const std::exception& e) { fprintf(stderr, "%s\n", e.what()); return 5; }
    xfh_destroy(ctx);
    return 0;
}
