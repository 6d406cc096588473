// triangulate_test.cpp -- ORB_SLAM3::XFmatcher::triangulate (include/xfeat/ORBmatcher_xfeat.h), host-container form and device form, on a scene the
// Python side writes out.
// usage: triangulate_test in.bin out.bin
// in.bin : int32 B, n1, n2, stereo; float cam[5] (fx fy cx cy bf), sigma2, scale_factor, scale_last, far_th; KF1 then the B neighbours, each:
//          float xy[n][2], (uright[n], depth[n] if stereo), Tcw[12], Ow[3]; int32 match12[B][n1]
// out.bin: twice (host form, device form): int32 n_new; per point int32 idx1, neighbour, idx2, stereo; float x3D[3], normal[3], min, max,
//          fuse[3]; int32 header[B][8]; then float devicePoints[n_new][3] read back from the device
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "xfeat/ORBmatcher_xfeat.h"

template <class T> static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T> static T* up(const std::vector<T>& v) {
    void* d = nullptr;
    if (xfh_dev_alloc(&d, v.size() * sizeof(T) + 16) != XFH_OK || xfh_memcpy_h2d(d, v.data(), v.size() * sizeof(T)) != XFH_OK) exit(3);
    return (T*)d;
}
struct KF { std::vector<float> xy, ur, z, T, O; };

static void put(FILE* o, const std::vector<ORB_SLAM3::XFnewMapPoint>& v, const std::vector<int>& hdr) {
    const int n = (int)v.size();
    fwrite(&n, 4, 1, o);
    for (const auto& q : v) {
        const int i[4] = {q.idx1, q.neighbour, q.idx2, q.stereo ? 1 : 0};
        fwrite(i, 4, 4, o); fwrite(q.x3D, 4, 3, o); fwrite(q.normal, 4, 3, o); fwrite(&q.minDistance, 4, 1, o); fwrite(&q.maxDistance, 4, 1, o); fwrite(q.fuseDistances, 4, 3, o);
    }
    fwrite(hdr.data(), 4, hdr.size(), o);
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    int h[4]; float cf[9];
    if (!f || !rd(f, h, 4) || !rd(f, cf, 9)) return 2;
    const int B = h[0], n1 = h[1], n2 = h[2], st = h[3];
    std::vector<KF> kf(B + 1);
    for (int k = 0; k <= B; ++k) {
        const int n = k == 0 ? n1 : n2;
        kf[k].xy.resize((size_t)n * 2); kf[k].ur.resize(st ? n : 0); kf[k].z.resize(st ? n : 0); kf[k].T.resize(12); kf[k].O.resize(3);
        if (!rd(f, kf[k].xy.data(), kf[k].xy.size()) || !rd(f, kf[k].ur.data(), kf[k].ur.size()) || !rd(f, kf[k].z.data(), kf[k].z.size()) || !rd(f, kf[k].T.data(), 12) ||
            !rd(f, kf[k].O.data(), 3)) return 2;
    }
    std::vector<int> m((size_t)B * n1);
    if (!rd(f, m.data(), m.size())) return 2;
    fclose(f);
    try {
        xfh_config cfg; xfh_config_default(&cfg);
        cfg.nfeatures = 1; cfg.max_height = 32; cfg.max_width = 32;
        xfh_ctx* ctx = nullptr;
        if (xfh_create(&cfg, &ctx) != XFH_OK) return 4;
        xfh_camera cam; memset(&cam, 0, sizeof cam);
        cam.fx = cf[0]; cam.fy = cf[1]; cam.cx = cf[2]; cam.cy = cf[3]; cam.bf = cf[4]; cam.width = 640; cam.height = 480;
        auto view = [&](const KF& k) { return ORB_SLAM3::XFtriKeyFrame{k.xy.data(), nullptr, st ? k.ur.data() : nullptr, st ? k.z.data() : nullptr, k.T.data(), k.O.data()}; };
        FILE* o = fopen(argv[2], "wb");
        {
            ORB_SLAM3::XFmatcher matcher(ctx, 0.6f, false);
            std::vector<ORB_SLAM3::XFnewMapPoint> vNew;
            std::vector<ORB_SLAM3::XFtriKeyFrame> nb;
            for (int b = 0; b < B; ++b) nb.push_back(view(kf[b + 1]));
            const int nh = matcher.triangulate(cam, n1, n2, view(kf[0]), nb, m, vNew, cf[5], cf[6], cf[7], cf[8]);
            if (nh != (int)vNew.size()) return 6;
            put(o, vNew, matcher.lastTriangulateHeader());
            // the device form: the neighbours' arrays one behind the other
            KF all;
            for (int b = 1; b <= B; ++b) {
                all.xy.insert(all.xy.end(), kf[b].xy.begin(), kf[b].xy.end()); all.ur.insert(all.ur.end(), kf[b].ur.begin(), kf[b].ur.end());
                all.z.insert(all.z.end(), kf[b].z.begin(), kf[b].z.end()); all.T.insert(all.T.end(), kf[b].T.begin(), kf[b].T.end());
                all.O.insert(all.O.end(), kf[b].O.begin(), kf[b].O.end());
            }
            auto dev = [&](const KF& k) { return ORB_SLAM3::XFtriKeyFrame{up(k.xy), nullptr, st ? up(k.ur) : nullptr, st ? up(k.z) : nullptr, up(k.T), up(k.O)}; };
            const ORB_SLAM3::XFtriKeyFrame d1 = dev(kf[0]), d2 = dev(all);
            int* dm = up(m);
            const int nd = matcher.triangulate(cam, B, n1, n2, d1, d2, dm, vNew, cf[5], cf[6], cf[7], cf[8]);
            if (nd != nh || matcher.lastTriangulateCount() != nd) return 6;
            put(o, vNew, matcher.lastTriangulateHeader());
            std::vector<float> back((size_t)nd * 3);
            if (nd && xfh_memcpy_d2h(back.data(), matcher.deviceNewPoints(), back.size() * 4) != XFH_OK) return 5;
            fwrite(back.data(), 4, back.size(), o);
            bool threw = false;                                            // what does not fit is refused
            try { matcher.triangulate(cam, B, XFH_GRID_MAX_N + 1, n2, d1, d2, dm, vNew); } catch (const std::exception&) { threw = true; }
            if (!threw) return 6;
            for (const ORB_SLAM3::XFtriKeyFrame* k : {&d1, &d2})
                for (const float* p : {k->keysUn, k->uright, k->depth, k->Tcw, k->Ow}) if (p) xfh_dev_free((void*)p);
            xfh_dev_free(dm);
        }
        fclose(o);
        xfh_destroy(ctx);
    } catch (const std::exception& e) { fprintf(stderr, "%s\n", e.what()); return 5; }
    return 0;
}
