// init_test.cpp -- XFmatcher::searchForInitialization (include/xfeat/ORBmatcher_xfeat.h), host-vector and device / XFgrid overloads, against the
// C ABI's host form (xfh_init_search) on one scene: dumps that must be identical.
// usage: init_test in.bin out.bin
// in.bin : int32 n, windowSize, use_flags, pad; float nnratio, pad[3]; xfh_camera (64 B); keypoints of F2 [n * 28 B]; targets[n * 64 f32];
//          queries[n * 64 f32]; prev_matched[n * 2 f32]; flags[n u8]
// out.bin: three times (C ABI, host overload, device overload): int32 n_matches, matches12[n], status[n] (widened), claim_idx[n], best_dist[n],
//          second_dist[n], n_window[n], n_tested[n], matches21[n], matched_distance[n], prev_matched after the call [n * 2 f32, as their bits]
#define XFEAT_NO_OPENCV 1
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "xfeat/XFextractor.h"
#include "xfeat/ORBmatcher_xfeat.h"

using namespace ORB_SLAM3;

template <class T> static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
static void wr(FILE* o, const std::vector<int>& v) { fwrite(v.data(), 4, v.size(), o); }
static void wr(FILE* o, const std::vector<float>& v) { fwrite(v.data(), 4, v.size(), o); }
static void wr(FILE* o, const std::vector<unsigned char>& v) { for (unsigned char s : v) { const int w = s; fwrite(&w, 4, 1, o); } }
static void* up(const void* src, size_t bytes) {
    void* d = nullptr;
    if (xfh_dev_alloc(&d, bytes + 16) != XFH_OK || xfh_memcpy_h2d(d, src, bytes) != XFH_OK) { fprintf(stderr, "upload failed\n"); exit(4); }
    return d;
}
static void dump(FILE* o, int nm, const std::vector<int>& m12, const XFmatcher& m, const std::vector<float>& prev) {
    fwrite(&nm, 4, 1, o);
    wr(o, m12); wr(o, m.lastInitStatus()); wr(o, m.lastInitClaim()); wr(o, m.lastInitBestDist()); wr(o, m.lastInitSecondDist()); wr(o, m.lastInitWindow());
    wr(o, m.lastInitTested()); wr(o, m.lastInitMatches21()); wr(o, m.lastInitMatchedDistance()); wr(o, prev);
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    int hdr[4]; float fl[4]; xfh_camera cam;
    if (!f || !rd(f, hdr, 4) || !rd(f, fl, 4) || !rd(f, &cam, 1)) return 2;
    const int n = hdr[0], window = hdr[1];
    const bool use_flags = hdr[2] != 0;
    std::vector<XFgrid::KeyPoint> keys(n);
    XFmatcher::Mat tg(n, 64, 4), q(n, 64, 4);
    std::vector<float> prev(2 * (size_t)n);
    std::vector<unsigned char> flags(n);
    if (!rd(f, keys.data(), n) || !rd(f, tg.ptr<float>(0), (size_t)n * 64) || !rd(f, q.ptr<float>(0), (size_t)n * 64) || !rd(f, prev.data(), prev.size()) ||
        !rd(f, flags.data(), n)) return 2;
    fclose(f);
    xfh_config cfg; xfh_config_default(&cfg);
    cfg.nfeatures = n; cfg.max_height = 32; cfg.max_width = 32;
    xfh_ctx* ctx = nullptr;
    if (xfh_create(&cfg, &ctx) != XFH_OK) return 3;
    try {
        xfh_grid_bounds b;
        if (xfh_camera_bounds(&cam, &b) != XFH_OK) return 4;
        FILE* o = fopen(argv[2], "wb");
        // 1: the C ABI's host form, prev_matched updated in place
        {
            std::vector<unsigned char> st(n);
            std::vector<int> ci(n), m12(n), bd(n), sd(n), nw(n), nt(n), m21(n), md(n);
            std::vector<float> pm = prev;
            int nm = -1;
            const int rc = xfh_init_search(ctx, n, q.ptr<float>(0), pm.data(), use_flags ? flags.data() : nullptr, (float)window, (const xfh_keypoint*)keys.data(), &b,
                                           tg.ptr<float>(0), n, XFmatcher::TH_LOW, fl[0], st.data(), ci.data(), m12.data(), bd.data(), sd.data(), nw.data(), nt.data(),
                                           m21.data(), md.data(), &nm, pm.data());
            if (rc != XFH_OK) { fprintf(stderr, "xfh_init_search: %s\n", xfh_strerror(rc)); return 5; }
            fwrite(&nm, 4, 1, o);
            wr(o, m12); wr(o, st); wr(o, ci); wr(o, bd); wr(o, sd); wr(o, nw); wr(o, nt); wr(o, m21); wr(o, md); wr(o, pm);
        }
        XFgrid grid(ctx);
        grid.build(keys, b);
        XFmatcher matcher(ctx, fl[0], true);
        // 2: the host-vector overload
        {
            std::vector<float> pm = prev;
            std::vector<int> m12;
            const int nm = matcher.searchForInitialization(q, pm, grid, tg, m12, window, use_flags ? &flags : nullptr);
            dump(o, nm, m12, matcher, pm);
        }
        // 3: the device overload
        {
            std::vector<float> xy;
            grid.keysXY(xy);
            float* dq = (float*)up(q.ptr<float>(0), (size_t)n * 256); float* dt = (float*)up(tg.ptr<float>(0), (size_t)n * 256);
            float* dp = (float*)up(prev.data(), (size_t)n * 8); float* dx = (float*)up(xy.data(), (size_t)n * 8);
            unsigned char* dfl = (unsigned char*)up(flags.data(), n);
            std::vector<int> m12;
            const int nm = matcher.searchForInitialization(n, dq, dp, use_flags ? dfl : nullptr, grid, dt, dx, m12, window);
            std::vector<float> pm(2 * (size_t)n);
            if (xfh_memcpy_d2h(pm.data(), dp, (size_t)n * 8) != XFH_OK) return 5;
            dump(o, nm, m12, matcher, pm);
            xfh_dev_free(dq); xfh_dev_free(dt); xfh_dev_free(dp); xfh_dev_free(dx); xfh_dev_free(dfl);
        }
        fclose(o);
    } catch (const std::exception& e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 6;
    }
    xfh_destroy(ctx);
    return 0;
}
