// loop_test.cpp -- the loop-closing / relocalisation methods of XFmatcher (include/xfeat/ORBmatcher_xfeat.h), host-vector and device / XFgrid
// overloads, against the C ABI's host forms (xfh_map_projection_search, xfh_sim3_search) on one scene: dumps that must be identical.
// usage: loop_test in.bin out.bin
// in.bin : int32 n, nlevels, form (0 Sim3, 1 Sim3 with keyframes, 2 relocalisation), pad; float th, scale_factor, ratioHamming, ORBdist; xfh_camera (64 B);
//          float Tcw[12], Ow[3], T1w[12], T2w[12], M21[12], M12[12]; keypoints[n * 28 B]; targets[n * 64 f32]; taken[n u8];
//          map projection: queries[n * 64 f32]; points, normals, distances[n * 3 f32 each]; flags[n u8];
//          SearchBySim3, per side (both keyframes have the n keypoints and rows above): points, distances[n * 3 f32 each], mp_desc[n * 64 f32], flags[n u8]
// out.bin: map projection, three times (C ABI, host overload, device overload): int32 n_matches, match_idx[n], status[n] (widened), best_dist[n],
//          n_window[n], n_tested[n], level[n], assigned[n]; then SearchBySim3, three times: int32 n_found, match12[n], and per side match[n], status[n]
//          (widened), best_dist[n], n_window[n], n_tested[n], level[n]
#define XFEAT_NO_OPENCV 1
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "xfeat/XFextractor.h"
#include "xfeat/ORBmatcher_xfeat.h"

using namespace ORB_SLAM3;

template <class T> static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
static void wr(FILE* o, const std::vector<int>& v) { fwrite(v.data(), 4, v.size(), o); }
static void wr(FILE* o, const std::vector<unsigned char>& v) { for (unsigned char s : v) { const int w = s; fwrite(&w, 4, 1, o); } }
static void* up(const void* src, size_t bytes) {
    void* d = nullptr;
    if (xfh_dev_alloc(&d, bytes + 16) != XFH_OK || xfh_memcpy_h2d(d, src, bytes) != XFH_OK) { fprintf(stderr, "upload failed\n"); exit(4); }
    return d;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    int hdr[4]; float fl[4]; xfh_camera cam; float T[12], Ow[3], T1[12], T2[12], M21[12], M12[12];
    if (!f || !rd(f, hdr, 4) || !rd(f, fl, 4) || !rd(f, &cam, 1) || !rd(f, T, 12) || !rd(f, Ow, 3) || !rd(f, T1, 12) || !rd(f, T2, 12) || !rd(f, M21, 12) || !rd(f, M12, 12)) return 2;
    const int n = hdr[0], nl = hdr[1], form = hdr[2];
    const float th = fl[0];
    std::vector<float> sf(nl, 1.0f);
    for (int i = 1; i < nl; ++i) sf[i] = sf[i - 1] * fl[1];
    std::vector<XFgrid::KeyPoint> keys(n);
    XFmatcher::Mat tg(n, 64, 4), q(n, 64, 4), mp1(n, 64, 4), mp2(n, 64, 4);
    std::vector<float> pts(3 * (size_t)n), nr(3 * (size_t)n), dd(3 * (size_t)n), p1(3 * (size_t)n), d1(3 * (size_t)n), p2(3 * (size_t)n), d2(3 * (size_t)n);
    std::vector<unsigned char> taken(n), flags(n), f1(n), f2(n);
    if (!rd(f, keys.data(), n) || !rd(f, tg.ptr<float>(0), (size_t)n * 64) || !rd(f, taken.data(), n) || !rd(f, q.ptr<float>(0), (size_t)n * 64) ||
        !rd(f, pts.data(), pts.size()) || !rd(f, nr.data(), nr.size()) || !rd(f, dd.data(), dd.size()) || !rd(f, flags.data(), n) ||
        !rd(f, p1.data(), p1.size()) || !rd(f, d1.data(), d1.size()) || !rd(f, mp1.ptr<float>(0), (size_t)n * 64) || !rd(f, f1.data(), n) ||
        !rd(f, p2.data(), p2.size()) || !rd(f, d2.data(), d2.size()) || !rd(f, mp2.ptr<float>(0), (size_t)n * 64) || !rd(f, f2.data(), n)) return 2;
    fclose(f);
    xfh_config cfg; xfh_config_default(&cfg);
    cfg.nfeatures = n; cfg.max_height = 32; cfg.max_width = 32;
    xfh_ctx* ctx = nullptr;
    if (xfh_create(&cfg, &ctx) != XFH_OK) return 3;
    try {
        xfh_grid_bounds b;
        if (xfh_camera_bounds(&cam, &b) != XFH_OK) return 4;
        FILE* o = fopen(argv[2], "wb");
        std::vector<float> rmax(nl);
        if (xfh_scale_level_thresholds(fl[1], nl, rmax.data()) != XFH_OK) return 4;
        XFgrid grid(ctx);
        grid.build(keys, b);
        XFmatcher matcher(ctx);
        XFmatcher::Sim3Form sform; sform.ratioHamming = fl[2]; sform.withKeyFrames = form == 1;
        XFmatcher::RelocForm rform; rform.ORBdist = (int)fl[3];
        // ---- map projection: the C ABI, host pointers
        {
            std::vector<int> mi(n), best(n), nwin(n), ntest(n), level(n), asg(n);
            std::vector<unsigned char> status(n);
            int nm = -1;
            const int cform = form == 0 ? XFH_MAPPROJ_FORM_SIM3 : form == 1 ? XFH_MAPPROJ_FORM_SIM3_KF : XFH_MAPPROJ_FORM_RELOC;
            const float accept = form == 2 ? (float)(int)fl[3] : (float)XFmatcher::TH_LOW * fl[2];
            if (xfh_map_projection_search(ctx, cform, n, pts.data(), nr.data(), dd.data(), q.ptr<float>(0), flags.data(), T, Ow, &cam, &b, th, sf.data(), rmax.data(), nl,
                                          (const xfh_keypoint*)keys.data(), tg.ptr<float>(0), n, taken.data(), 256, accept, status.data(), mi.data(), best.data(), nwin.data(),
                                          ntest.data(), level.data(), nullptr, asg.data(), &nm) != XFH_OK) return 4;
            fwrite(&nm, 4, 1, o); wr(o, mi); wr(o, status); wr(o, best); wr(o, nwin); wr(o, ntest); wr(o, level); wr(o, asg);
        }
        auto dump_map = [&](int nm, const std::vector<int>& mi, const std::vector<int>& asg) {
            fwrite(&nm, 4, 1, o); wr(o, mi); wr(o, matcher.lastMapProjectionStatus()); wr(o, matcher.lastMapProjectionBestDist()); wr(o, matcher.lastMapProjectionWindow());
            wr(o, matcher.lastMapProjectionTested()); wr(o, matcher.lastMapProjectionLevel()); wr(o, asg);
        };
        std::vector<int> mi, asg;
        int nm = form == 2 ? matcher.searchByProjection(rform, q, pts, nr, dd, flags, T, Ow, cam, b, th, sf, grid, tg, mi, asg, &taken)
                           : matcher.searchByProjection(sform, q, pts, nr, dd, flags, T, Ow, cam, b, th, sf, grid, tg, mi, asg, &taken);
        dump_map(nm, mi, asg);
        const size_t bq = (size_t)n * 256, bp = (size_t)n * 12;
        const float* dq = (const float*)up(q.ptr<float>(0), bq); const float* dp = (const float*)up(pts.data(), bp); const float* dn = (const float*)up(nr.data(), bp);
        const float* ddd = (const float*)up(dd.data(), bp); const unsigned char* dfl = (const unsigned char*)up(flags.data(), n); const float* dT = (const float*)up(T, 48);
        const float* dO = (const float*)up(Ow, 12); const float* dt = (const float*)up(tg.ptr<float>(0), bq); const unsigned char* dtk = (const unsigned char*)up(taken.data(), n);
        nm = form == 2 ? matcher.searchByProjection(rform, n, dp, dn, ddd, dq, dfl, dT, dO, cam, b, th, sf, grid, dt, dtk, mi, asg)
                       : matcher.searchByProjection(sform, n, dp, dn, ddd, dq, dfl, dT, dO, cam, b, th, sf, grid, dt, dtk, mi, asg);
        dump_map(nm, mi, asg);
        // ---- SearchBySim3: the C ABI, host pointers
        {
            std::vector<int> m12(n), o1[5], o2[5];
            for (int k = 0; k < 5; ++k) { o1[k].resize(n); o2[k].resize(n); }
            std::vector<unsigned char> s1(n), s2(n);
            xfh_sim3_side a = {n, nullptr, (const xfh_keypoint*)keys.data(), tg.ptr<float>(0), 0, p1.data(), d1.data(), mp1.ptr<float>(0), f1.data(), T1, s1.data(),
                               o1[0].data(), o1[1].data(), o1[2].data(), o1[3].data(), o1[4].data(), nullptr};
            xfh_sim3_side c = {n, nullptr, (const xfh_keypoint*)keys.data(), tg.ptr<float>(0), 0, p2.data(), d2.data(), mp2.ptr<float>(0), f2.data(), T2, s2.data(),
                               o2[0].data(), o2[1].data(), o2[2].data(), o2[3].data(), o2[4].data(), nullptr};
            int nf = -1;
            if (xfh_sim3_search(ctx, &a, &c, M21, M12, &cam, &b, th, sf.data(), rmax.data(), nl, XFmatcher::TH_HIGH, m12.data(), &nf) != XFH_OK) return 4;
            fwrite(&nf, 4, 1, o); wr(o, m12);
            wr(o, o1[0]); wr(o, s1); for (int k = 1; k < 5; ++k) wr(o, o1[k]);
            wr(o, o2[0]); wr(o, s2); for (int k = 1; k < 5; ++k) wr(o, o2[k]);
        }
        auto dump_sim3 = [&](int nf, const std::vector<int>& m12) {
            fwrite(&nf, 4, 1, o); wr(o, m12);
            for (int s = 1; s <= 2; ++s) {
                wr(o, matcher.lastSim3Matches(s)); wr(o, matcher.lastSim3Status(s)); wr(o, matcher.lastSim3BestDist(s)); wr(o, matcher.lastSim3Window(s));
                wr(o, matcher.lastSim3Tested(s)); wr(o, matcher.lastSim3Level(s));
            }
        };
        std::vector<int> m12;
        XFmatcher::Sim3KeyFrame h1 = {&keys, &tg, &p1, &d1, &mp1, &f1, T1}, h2 = {&keys, &tg, &p2, &d2, &mp2, &f2, T2};
        int nf = matcher.searchBySim3(h1, h2, M21, M12, cam, b, th, sf, m12);
        dump_sim3(nf, m12);
        XFmatcher::Sim3KeyFrameDevice g1 = {&grid, dt, (const float*)up(p1.data(), bp), (const float*)up(d1.data(), bp), (const float*)up(mp1.ptr<float>(0), bq),
                                            (const unsigned char*)up(f1.data(), n), (const float*)up(T1, 48)};
        XFmatcher::Sim3KeyFrameDevice g2 = {&grid, dt, (const float*)up(p2.data(), bp), (const float*)up(d2.data(), bp), (const float*)up(mp2.ptr<float>(0), bq),
                                            (const unsigned char*)up(f2.data(), n), (const float*)up(T2, 48)};
        const float* dM21 = (const float*)up(M21, 48); const float* dM12 = (const float*)up(M12, 48);
        nf = matcher.searchBySim3(g1, g2, dM21, dM12, cam, b, th, sf, m12);
        dump_sim3(nf, m12);
        fclose(o);
        for (const void* p : {(const void*)dq, (const void*)dp, (const void*)dn, (const void*)ddd, (const void*)dfl, (const void*)dT, (const void*)dO, (const void*)dt,
                              (const void*)dtk, (const void*)g1.d_points, (const void*)g1.d_distances, (const void*)g1.d_mpDesc, (const void*)g1.d_flags, (const void*)g1.d_Tw,
                              (const void*)g2.d_points, (const void*)g2.d_distances, (const void*)g2.d_mpDesc, (const void*)g2.d_flags, (const void*)g2.d_Tw, (const void*)dM21,
                              (const void*)dM12})
            xfh_dev_free((void*)p);
    } catch (const std::exception& e) { fprintf(stderr, "%s\n", e.what()); return 5; }
    xfh_destroy(ctx);
    return 0;
}
